"""CPU tests of what tests/test_gpu_hermitian.py compares the Hermitian cost kind against (tests/hermitian_ref.py), of
problems.phase_synchronization, and of the refusals solvers.ManiSDP_onlyunitdiag raises for a complex C before the library is
loaded."""
import numpy as np
import pytest
import scipy.sparse as sp

import hermitian_ref as HR


def _relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("storage", HR.STORAGES)
def test_restatement_derivatives_agree_with_central_differences(storage):
    n, p = 203, 3
    C = HR.instance(storage, n)
    Y = HR.table_point(n, p)
    assert np.allclose(np.sum(np.abs(Y) ** 2, axis=1), 1.0, atol=1e-14)
    U = HR.table_direction(n, p)
    U = U - Y * np.real(np.sum(U * np.conj(Y), axis=1, keepdims=True))        # tangent: Re<u_i, y_i> = 0

    def retr(t):
        Z = Y + t * U
        return Z / np.sqrt(np.sum(np.abs(Z) ** 2, axis=1, keepdims=True))

    def inner(a, b):
        return float(np.real(np.sum(np.conj(a) * b)))

    G, H = HR.rgrad(C, Y), HR.hessvec(C, Y, U)
    t = 1e-4
    fp, fm, f0 = HR.cost(C, retr(t)), HR.cost(C, retr(-t)), HR.cost(C, Y)
    d1 = (fp - fm) / (2 * t)
    d2 = (fp - 2 * f0 + fm) / (t * t)
    # central differences: O(t^2) truncation, O(eps |f| / t^2) rounding in the second one (|f| ~ 1e2: 1e-6)
    assert abs(d1 - inner(G, U)) < 1e-6 * max(1.0, abs(inner(G, U)))
    assert abs(d2 - inner(H, U)) < 1e-4 * max(1.0, abs(inner(H, U)))
    # the gradient and the Hess-vec are tangent
    assert np.max(np.abs(np.real(np.sum(G * np.conj(Y), axis=1)))) < 1e-13
    assert np.max(np.abs(np.real(np.sum(H * np.conj(Y), axis=1)))) < 1e-12


@pytest.mark.parametrize("storage", HR.STORAGES)
def test_operator_is_the_embedding_and_the_oracle_problem_is_the_restatement(storage):
    from oracle import manisdp_ref as R
    n, p = 203, 5
    C = HR.instance(storage, n)
    Y, U = HR.table_point(n, p), HR.table_direction(n, p)
    Ct = HR.embed(C)
    assert abs(Ct - Ct.T).nnz == 0
    CY = C @ Y
    emb = Ct @ np.vstack([Y.real, Y.imag])
    assert np.max(np.abs(emb[:n] - CY.real)) <= 1e-14 * max(1.0, np.max(np.abs(CY)))
    assert np.max(np.abs(emb[n:] - CY.imag)) <= 1e-14 * max(1.0, np.max(np.abs(CY)))
    assert np.max(np.abs(HR.complex_view(HR.Op(C) @ HR.real_view(Y)) - CY)) <= 1e-14 * max(1.0, np.max(np.abs(CY)))
    # the oracle's closures on the real view are the complex restatement
    prob = R._OnlyUnitDiagProblem(HR.Op(C), n, 2 * p, q1="correct")
    Yr, Ur = HR.real_view(Y), HR.real_view(U)
    assert abs(prob.cost(Yr) - HR.cost(C, Y)) <= 1e-13 * abs(HR.cost(C, Y))
    assert _relerr(HR.complex_view(prob.grad(Yr)), HR.rgrad(C, Y)) < 1e-13
    assert _relerr(HR.complex_view(prob.hess(Yr, Ur)), HR.hessvec(C, Y, U)) < 1e-13
    # the embedded point doubles the cost
    Ye = HR.embed_point(Y)
    assert abs(0.5 * np.sum((Ct @ Ye) * Ye) - 2.0 * HR.cost(C, Y)) <= 1e-12 * abs(HR.cost(C, Y))
    # conj(C) is another problem
    assert _relerr(HR.hessvec(C.conj(), Y, U), HR.hessvec(C, Y, U)) > 1e-3


def test_phase_synchronization_definition():
    from manisdp_matlab_amd import problems
    n, degree = 60, 6
    C, z = problems.phase_synchronization(n, degree, 0.0, np.random.default_rng(3))
    assert sp.issparse(C) and C.format == "csr" and C.dtype == np.complex128
    assert abs(C - C.conj().T).nnz == 0 and not C.diagonal().any()
    assert C.nnz == n * degree
    assert np.allclose(np.abs(z), 1.0, atol=1e-15)
    assert abs(np.real(np.conj(z) @ (C @ z)) + C.nnz) < 1e-10 and C.nnz == 360
    # the draw order: z, then the real parts of the noise, then the imaginary parts
    g = np.random.default_rng(3)
    z_ref = np.exp(2j * np.pi * g.random(n))
    m = n * degree // 2
    w = (g.standard_normal(m) + 1j * g.standard_normal(m)) / np.sqrt(2.0)
    assert np.array_equal(z, z_ref)
    Cn, zn = problems.phase_synchronization(n, degree, 2.0, np.random.default_rng(3))
    assert np.array_equal(zn, z_ref)
    # edge e = (d - 1) n + i joins i -> (i + d^2 + 1) mod n and carries w[e]
    for d, i in ((1, 0), (2, 7), (3, 59)):
        j = (i + d * d + 1) % n
        e = (d - 1) * n + i
        assert abs(Cn[i, j] + (z_ref[i] * np.conj(z_ref[j]) + 2.0 * w[e])) < 1e-14
        assert Cn[j, i] == np.conj(Cn[i, j])


def test_restatement_solves_a_small_phase_synchronization():
    from manisdp_matlab_amd import problems
    from oracle import manisdp_ref as R
    C, _ = problems.phase_synchronization(60, 6, 1.0, np.random.default_rng(7))
    g = np.random.default_rng(1)
    Y0 = g.standard_normal((60, 2)) + 1j * g.standard_normal((60, 2))
    Y0 /= np.sqrt(np.sum(np.abs(Y0) ** 2, axis=1, keepdims=True))
    Y, obj, data = HR.solve(C, Y0)
    assert data["status"] == 0 and data["dinf"] < 1e-8
    _, obj_e, data_e = R.ManiSDP_onlyunitdiag(HR.embed(C), {"Y0": HR.embed_point(Y0[:, :1])}, q1="correct")
    assert data_e["status"] == 0
    assert abs(obj - 0.5 * obj_e) < 1e-6 * abs(obj)


def test_solver_refuses_before_the_library_loads(monkeypatch):
    from manisdp_matlab_amd import _lib, problems, solvers

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", no_load)
    C, _ = problems.phase_synchronization(60, 6, 1.0, np.random.default_rng(7))
    bad = C.tolil(); bad[0, 3] = bad[0, 3] + 0.5; bad = bad.tocsr()
    with pytest.raises(ValueError, match="Hermitian"):
        solvers.ManiSDP_onlyunitdiag(bad, {}, verbose=False)
    with pytest.raises(ValueError, match="Hermitian"):
        solvers.ManiSDP_onlyunitdiag(bad.toarray(), {}, verbose=False)         # a small dense complex array takes the same path
    diag = C.tolil(); diag[5, 5] = 1.0 + 0.25j; diag = diag.tocsr()
    with pytest.raises(ValueError, match="Hermitian"):
        solvers.ManiSDP_onlyunitdiag(diag, {}, verbose=False)
    with pytest.raises(ValueError, match="Hermitian"):
        solvers.ManiSDP_onlyunitdiag(C, {"round": {"trials": 64, "sweeps": 1, "seed": 0}}, verbose=False)
    with pytest.raises(ValueError, match="Hermitian"):
        solvers.ManiSDP_onlyunitdiag(C, {"comm": ("local", 1, 0, 99)}, verbose=False)
    with pytest.raises(ValueError, match="Hermitian"):
        solvers.ManiSDP_onlyunitdiag(C, {"line_search": 1}, verbose=False)
    with pytest.raises(ValueError, match="Hermitian"):
        solvers.ManiSDP_onlyunitdiag(C, {"device_factor": True}, verbose=False)
    with pytest.raises(ValueError, match="Hermitian"):
        _lib.Handle.onlyunitdiag_hermitian(bad)
