"""CPU tests of what tests/test_gpu_phase_round.py compares msdp_round_phases against (tests/phase_round_ref.py): the
restatement's fixed points are 1-opt local minima and never beat the brute-force minimum, its sweeps never raise a value, the
decision margins of every instance the GPU tests use are wide enough for a device that sums in another order to decide alike,
the fp64 / long double distance the M = 0 sweeps are held to; problems.mpsk_synchronization and problems.phase_error; and the
refusals solvers.ManiSDP_onlyunitdiag raises for the new options before the library is loaded."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import hermitian_ref as HR
import phase_round_ref as PR


def _small(seed):
    """A dense Hermitian C of order 6 with entries in Z/4 + i Z/4, a point of width 2 and 64 rows R."""
    g = np.random.default_rng(seed)
    A = g.integers(-3, 4, size=(6, 6)) / 4.0 + 1j * g.integers(-3, 4, size=(6, 6)) / 4.0
    C = np.triu(A, 1)
    C = C + C.conj().T + np.diag(g.integers(-3, 4, size=6) / 4.0)
    Y, R = PR.inputs(6, 2, 64, seed)
    return sp.csr_matrix(C), Y, R


def test_table_is_exact_where_it_can_be():
    assert np.array_equal(PR.table(2), [[1, 0], [-1, 0]])
    assert np.array_equal(PR.table(4), [[1, 0], [0, 1], [-1, 0], [0, -1]])
    t = PR.table(8)
    assert np.array_equal(t[::2], PR.table(4)) and np.allclose(t[1], np.sqrt(0.5), atol=1e-16)
    assert np.allclose(np.hypot(PR.table(64)[:, 0], PR.table(64)[:, 1]), 1.0, atol=1e-15)


@pytest.mark.parametrize("M", [2, 4])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fixed_points_are_local_minima_and_nothing_beats_brute_force(M, seed):
    C, Y, R = _small(seed)
    Cd = C.toarray()
    tab = PR.table(M)
    pts = tab[:, 0] + 1j * tab[:, 1]
    allz = np.array(list(itertools.product(pts, repeat=6)))                       # M^6 points
    brute = np.min(np.real(np.sum(np.conj(allz) * (allz @ Cd.T), axis=1)))
    r = PR.round_phases(C, Y, R, M, 50)
    assert np.all(r["info"][1] == 0) and np.all(r["info"][0] < 50)              # every word reached a fixed point
    Z = r["phases"].transpose(1, 0, 2).reshape(6, -1)
    val = lambda z: float(np.real(np.conj(z) @ (Cd @ z)))
    assert np.all(r["values"] >= brute) and np.all(r["values0"] >= brute)         # entries in Z/4, exact table: exact sums
    for t in range(Z.shape[1]):
        z = Z[:, t]
        assert val(z) == r["values"][t]
        for i in range(6):
            for c in pts:
                y = z.copy(); y[i] = c
                assert val(y) >= val(z), (t, i)                                    # 1-opt: no single change lowers the value


@pytest.mark.parametrize("M", [0, 2, 4, 8])
def test_values_never_rise_from_sweep_to_sweep(M):
    C = HR.instance("hub", 203) if M != 8 else PR.generic_instance(HR.instance("hub", 203))
    Y, R = PR.inputs(203, 3, 64, 41)
    r = PR.round_phases(C, Y, R, M, 6, trace=True)
    scale = np.abs(C).sum()
    for a, b in zip(r["trace"], r["trace"][1:]):
        assert np.all(b <= a + (0.0 if M in (2, 4) else 1e-13 * scale))          # exact sums for M = 2, 4; rounding otherwise
    assert np.array_equal(r["trace"][0], r["values0"]) and np.array_equal(r["trace"][-1], r["values"])
    assert np.all(r["values"] < r["values0"])


@pytest.mark.parametrize("case", PR.EXACT_CASES)
def test_margins_of_the_exact_cases(case):
    """M = 2, 4 on entries in Z/4: the rounding is the only inexact step, and its margin is above 1e-9 max|w|."""
    storage, n, T, p, M, seed = case
    r = PR.round_phases(HR.instance(storage, n), *PR.inputs(n, p, T, seed), M, 0)
    print(case, "rounding margin %.2e of max|w| = %.3f" % (r["margin_round"] / r["scale_round"], r["scale_round"]))
    assert r["margin_round"] > PR.MARGIN_REL * r["scale_round"]


def real_case_inputs(case):
    storage, n, T, p, seed = case
    Y, R = PR.inputs(n, p, T, seed)
    Yr = np.ascontiguousarray(Y.real / np.linalg.norm(Y.real, axis=1, keepdims=True))
    return sp.csr_matrix(HR.instance(storage, n).real), Yr, np.ascontiguousarray(R.real)


@pytest.mark.parametrize("case", PR.REAL_CASES)
def test_margins_of_the_real_cross_check(case):
    A, Yr, Rr = real_case_inputs(case)
    r = PR.round_phases(A.astype(np.complex128), Yr + 0j, Rr + 0j, 2, 0)
    assert r["margin_round"] > PR.MARGIN_REL * r["scale_round"]
    # margin of sign(Y r) itself: |Y r| is half the gap between the two candidates
    assert np.min(np.abs(Yr @ Rr.T)) > PR.MARGIN_REL * np.max(np.abs(Yr @ Rr.T))


@pytest.mark.parametrize("case", PR.TOL_CASES)
def test_margins_and_reference_distance_of_the_tolerance_cases(case):
    """M = 0 / M = 8: the rounding margins on the table instance; the M = 8 sweep margins on the generic instance (with entries
    in Z/4 the candidates tie exactly, see phase_round_ref.generic_instance); and the distance between the fp64 restatement and
    the same in long double after 1 and 3 sweeps of M = 0, the yardstick of the GPU test (DESIGN.md section 4 quotes it)."""
    storage, n, T, p, seed = case
    C = HR.instance(storage, n)
    Y, R = PR.inputs(n, p, T, seed)
    r0, r8 = PR.round_phases(C, Y, R, 0, 0), PR.round_phases(C, Y, R, 8, 0)
    assert r0["margin_round"] > PR.MARGIN_REL * r0["scale_round"] and r8["margin_round"] > PR.MARGIN_REL * r8["scale_round"]
    g8 = PR.round_phases(PR.generic_instance(C), Y, R, 8, PR.M8_SWEEPS)
    print(case, "M = 8 generic: rounding margin %.2e, sweep margin %.2e of the scale, sweeps %s" % (
        g8["margin_round"] / g8["scale_round"], g8["margin_sweep"] / g8["scale_sweep"], g8["info"][0].tolist()))
    assert g8["margin_round"] > PR.MARGIN_REL * g8["scale_round"] and g8["margin_sweep"] > PR.MARGIN_REL * g8["scale_sweep"]
    assert np.all(g8["info"][1] == 0)
    for s in PR.CIRCLE_SWEEPS:
        a, b = PR.round_phases(C, Y, R, 0, s), PR.round_phases(C, Y, R, 0, s, dtype=np.longdouble)
        dist = np.max(np.abs(a["phases"] - b["phases"]))
        print(case, "M = 0, %d sweeps: fp64 to long double %.3e" % (s, dist))
        assert 0 < dist < 1e-10                                                   # a rounding-level distance, not a different path


def test_mpsk_synchronization_and_phase_error():
    from manisdp_matlab_amd import problems
    n, degree, M = 60, 6, 4
    C, z = problems.mpsk_synchronization(n, degree, 0.0, M, np.random.default_rng(3))
    assert sp.issparse(C) and C.format == "csr" and C.dtype == np.complex128
    assert abs(C - C.conj().T).nnz == 0 and not C.diagonal().any() and C.nnz == n * degree
    g = np.random.default_rng(3)
    k = g.integers(M, size=n)
    assert np.array_equal(z, np.exp(2j * np.pi * k / M))                           # the draw order: the symbols first ...
    m = n * degree // 2
    w = (g.standard_normal(m) + 1j * g.standard_normal(m)) / np.sqrt(2.0)
    Cn, zn = problems.mpsk_synchronization(n, degree, 2.0, M, np.random.default_rng(3))
    assert np.array_equal(zn, z)
    for d, i in ((1, 0), (2, 7), (3, 59)):                                         # ... then the noise of phase_synchronization
        j = (i + d * d + 1) % n
        assert abs(Cn[i, j] + (z[i] * np.conj(z[j]) + 2.0 * w[(d - 1) * n + i])) < 1e-14
    assert abs(np.real(np.conj(z) @ (C @ z)) + C.nnz) < 1e-10
    # phase_synchronization itself is untouched: same generator state, same graph
    Cp, _ = problems.phase_synchronization(n, degree, 0.0, np.random.default_rng(3))
    assert np.array_equal(Cp.indices, C.indices) and np.array_equal(Cp.indptr, C.indptr)
    with pytest.raises(ValueError):
        problems.mpsk_synchronization(n, degree, 0.0, 1, np.random.default_rng(3))
    # the error is 0 at z = g z_true (to the rounding of one complex product)
    assert problems.phase_error(z, z, M) == 0.0 and problems.phase_error(z, z, 0) < 1e-15
    assert problems.phase_error(1j * z, z, M) < 1e-15 and problems.phase_error(-z, z, 2) < 1e-15
    assert problems.phase_error(np.exp(0.37j) * z, z, 0) < 1e-15
    assert abs(problems.phase_error(np.exp(0.37j) * z, z, M) - abs(np.exp(0.37j) - 1)) < 1e-15   # no M-th root undoes 0.37 rad
    y = z.copy(); y[5] = -y[5]
    assert abs(problems.phase_error(y, z, 2) - 2.0) < 1e-15                        # one wrong symbol: g = +-1 leave an error of 2 ...
    assert abs(problems.phase_error(y, z, M) - np.sqrt(2.0)) < 1e-15               # ... and g = +-i spread it to sqrt(2) everywhere


def test_solve_instances_of_the_gpu_test():
    s = PR.solve_instance("sync")
    assert s["data"]["status"] == 0 and s["data"]["rank"] == 1 and s["data"]["dinf"] < 1e-8
    m = PR.solve_instance("mpsk")
    assert m["data"]["status"] == 0 and m["data"]["dinf"] < 1e-8 and m["M"] == 4
    assert np.allclose(m["z"] ** 4, 1.0, atol=1e-14)
    s3 = PR.solve_instance("sync3")
    assert s3["data"]["status"] == 0 and s3["data"]["iters"] >= 2 and s3["data"]["rank"] > 1


def test_solver_refuses_the_new_options_before_the_library_loads(monkeypatch):
    from manisdp_matlab_amd import _lib, problems, solvers

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", no_load)
    Cc, _ = problems.phase_synchronization(60, 6, 1.0, np.random.default_rng(7))
    Cr = sp.csr_matrix(HR.instance("grid", 203).real)
    bad_rounds = [7, {"M": 1}, {"M": 65}, {"M": 2.0}, {"M": True}, {"trials": 100}, {"trials": 2048}, {"trials": 0},
                  {"sweeps": -1}, {"seed": -1}, {"sweeps": 1.5}, {"trails": 64}]
    for C in (Cc, Cr):
        for bad in bad_rounds:
            with pytest.raises(ValueError, match="round_phases"):
                solvers.ManiSDP_onlyunitdiag(C, {"round_phases": bad}, verbose=False)
        for bad in ("gpu", 1, True):
            with pytest.raises(ValueError, match="hermitian_factor"):
                solvers.ManiSDP_onlyunitdiag(C, {"hermitian_factor": bad}, verbose=False)
    # well-formed, but a real C: the options are the complex problem's
    with pytest.raises(ValueError, match="complex Hermitian"):
        solvers.ManiSDP_onlyunitdiag(Cr, {"round_phases": {"M": 4, "trials": 64, "sweeps": 1, "seed": 0}}, verbose=False)
    with pytest.raises(ValueError, match="complex Hermitian"):
        solvers.ManiSDP_onlyunitdiag(Cr, {"hermitian_factor": "device"}, verbose=False)
    # the refusals the kind already had stay
    with pytest.raises(ValueError, match="Hermitian"):
        solvers.ManiSDP_onlyunitdiag(Cc, {"round": {"trials": 64, "sweeps": 1, "seed": 0}, "hermitian_factor": "device"}, verbose=False)
    with pytest.raises(ValueError, match="Hermitian"):
        solvers.ManiSDP_onlyunitdiag(Cc, {"device_factor": True, "round_phases": {"M": 0}}, verbose=False)
