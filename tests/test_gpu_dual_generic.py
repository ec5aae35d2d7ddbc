"""GPU tests of the generic dual approach (MSDP_KIND_DUAL, solvers.ManiDSDP; reference src/dual/ManiDSDP.m) against the
NumPy restatement in dual_generic_ref.py.  Operators agree to 1e-11 relative (fp64, other summation orders); full solves
reach the optimum of the primal moment relaxation of the same quartic (strong duality, GPU solvers.ManiSDP) to 1e-7."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden_path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dual_generic_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu


def _relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _coe(d):
    from manisdp_matlab_amd import problems
    if d == 10:
        return np.loadtxt(golden_path("qs_c_10_1.txt.gz"), delimiter=",").ravel()
    return np.random.default_rng(5).standard_normal(problems.get_basis(d, 4).shape[1])


def _qssos(d):
    from manisdp_matlab_amd import problems
    A, b, c, K, dAAt = problems.qssos(d, _coe(d))
    maxb = float(np.max(np.abs(b)))
    return A, b / maxb, c, K, dAAt, maxb


def _overlapping(n=9, m=14, nf=2, seed=4):
    """Small random symmetric constraint matrices whose supports overlap (G = D\\A*A' != I), a free part and a cost."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(m):
        Mk = np.zeros((n, n))
        for _ in range(4):
            i, j = rng.integers(0, n, 2)
            v = rng.standard_normal()
            Mk[i, j] += v; Mk[j, i] += v
        rows.append(Mk.ravel(order="F"))
    Apsd = sp.csr_matrix(np.array(rows))
    B = sp.csr_matrix(rng.standard_normal((m, nf)) * (rng.random((m, nf)) < 0.5))
    C = rng.standard_normal((n, n)); C = 0.3 * (C + C.T)
    A = sp.hstack([B, Apsd]).tocsr()
    c = np.concatenate([rng.standard_normal(nf), C.ravel(order="F")])
    b = rng.standard_normal(m)
    dAAt = np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel()
    return A, b, c, {"f": nf, "s": n}, dAAt


def _split(A, c, K):
    nf = K["f"]
    Ac = sp.csc_matrix(A)
    return sp.csr_matrix(Ac[:, nf:]), Ac[:, :nf], c[nf:], c[:nf]


def _case(name):
    if name == "qssos10":
        A, b, c, K, dAAt, _ = _qssos(10)
        return A, b, c, K, dAAt, True
    if name == "nofree":
        A, b, c, K, dAAt, _ = _qssos(6)
        n = K["s"]
        Apsd = sp.csc_matrix(A)[:, K["f"]:]
        C = np.random.default_rng(2).standard_normal((n, n)); C = 0.1 * (C + C.T)
        return Apsd, b, C.ravel(order="F"), {"f": 0, "s": n}, dAAt, True
    A, b, c, K, dAAt = _overlapping()
    return A, b, c, K, dAAt, False


@pytest.mark.parametrize("case,p", [("qssos10", 7), ("nofree", 5), ("overlap", 4)])
def test_dual_generic_operators(lib, case, p):
    A, b, c, K, dAAt, g_identity = _case(case)
    n, nf = K["s"], K["f"]
    Apsd, B, cp, cf = _split(A, c, K)
    prob = G.DualGenericProblem(Apsd, B, b, cp, cf, dAAt, n, p, q1="correct")
    h = lib.Handle.dual(Apsd, b, cp, dAAt, B if nf else None, cf, pcap=max(32, p))
    assert h.dual_g_identity() == g_identity
    rng = np.random.default_rng(p)
    # outer step at a random point with nonzero w and sigma (x starts at 0): moves the device-resident x
    sigma0, w0 = 0.37, rng.standard_normal(nf)
    prob.sigma, prob.w = sigma0, w0.copy()
    Y0 = rng.standard_normal((n, p))
    h.dual_set_penalty(sigma0, w0 if nf else None)
    h.set_point(Y0)
    _check_outer_step(h, prob, Y0, b, cp, cf, nf)
    # cost / gradient / Hess-vec / line-search cost at another point, with the updated x and other w, sigma
    sigma, w = 2.3, rng.standard_normal(nf)
    prob.sigma, prob.w = sigma, w.copy()
    Y, U = rng.standard_normal((n, p)), rng.standard_normal((n, p))
    h.dual_set_penalty(sigma, w if nf else None)
    h.set_point(Y)
    f_ref = prob.cost(Y)
    assert abs(h.cost() - f_ref) <= 1e-11 * max(1.0, abs(f_ref))
    assert _relerr(h.rgrad(), prob.grad(Y)) < 1e-11
    assert _relerr(h.hessvec(U), prob.hess(Y, U)) < 1e-11
    V = rng.standard_normal((n, p))
    f_t = prob.co(Y + 0.3 * V)
    assert abs(h.linesearch_cost(V, 0.3) - f_t) <= 1e-11 * max(1.0, abs(f_t))
    # a second outer step, now with nonzero x: the x/sigma add-back in |As|^2 and x <- X - bA with the previous x
    h.set_point(Y)
    _check_outer_step(h, prob, Y, b, cp, cf, nf)
    h.close()


def _check_outer_step(h, prob, Y, b, cp, cf, nf):
    """msdp_dual_outer_step at Y against :66-77 of the restatement (updates prob.x, prob.w)."""
    n = prob.n
    sigma = prob.sigma
    by, cex, as2, Af, _ = h.dual_outer_step()
    S = Y @ Y.T
    sc = S.ravel(order="F") - cp
    y = prob.iAt @ sc
    As = prob.At @ y - sc
    Af_ref = prob.B.T @ y - cf
    assert abs(by - b @ y) <= 1e-11 * max(1.0, abs(b @ y))
    assert abs(as2 - As @ As) <= 1e-11 * max(1.0, As @ As)
    if nf:
        assert _relerr(Af, Af_ref) < 1e-11
    prob.x = prob.x + sigma * (prob.iAB @ (Af_ref - prob.w / sigma) + prob.At @ (prob.iAt @ (As - prob.x / sigma)) - As)   # :73
    prob.w = prob.w - sigma * Af_ref                                                                                        # :74
    X_ref = (prob.x + prob.bA).reshape((n, n), order="F")                                                                    # :75
    assert _relerr(h.get_dual_slack(), X_ref) < 1e-11
    assert abs(cex - cp @ X_ref.ravel(order="F")) <= 1e-11 * max(1.0, np.abs(X_ref).sum())
    assert _relerr(h.dual_get_y(), y) < 1e-11


@pytest.mark.parametrize("maxinner", [1, 3, 20])
def test_dual_generic_single_rtr(lib, maxinner):
    """One trustregions() call against the restatement's closures (q1 = 'correct'): the same iterations, Hess-vecs,
    accepted / rejected steps, cost and end point."""
    from oracle.manopt_rtr import trustregions
    A, b, c, K, dAAt, _ = _qssos(6)
    n, nf, p = K["s"], K["f"], 5
    Apsd, B, cp, cf = _split(A, c, K)
    prob = G.DualGenericProblem(Apsd, B, b, cp, cf, dAAt, n, p, q1="correct")
    rng = np.random.default_rng(1)
    prob.sigma, prob.w = 0.1, 0.01 * rng.standard_normal(nf)
    h = lib.Handle.dual(Apsd, b, cp, dAAt, B, cf)
    Y = rng.standard_normal((n, p))
    h.dual_set_penalty(prob.sigma, prob.w)
    h.set_point(Y)
    st = h.rtr(lib.default_opts(maxiter=4, maxinner=maxinner, tolgradnorm=1e-8))
    Yr, fr, info = trustregions(prob, Y.copy(), 4, maxinner, 1e-8)
    assert st.hessvecs == info.hessvecs
    assert st.iters == info.iters
    assert st.accepted == info.accepted and st.rejected == info.rejected
    assert abs(st.cost - fr) <= 1e-10 * max(1.0, abs(fr))
    assert abs(st.gradnorm - info.gradnorm) <= 1e-8 * max(1.0, info.gradnorm)
    assert _relerr(h.get_point(), Yr) < 1e-8
    h.close()


def _unitdiag_case():
    from manisdp_matlab_amd import problems
    from oracle import manisdp_ref as R
    rng = np.random.default_rng(7)
    d = 8
    Q = rng.standard_normal((d, d)); Q = (Q + Q.T) / 2
    A, b, c, K, dAAt, _ = problems.bqpsos_dual_problem(Q, rng.standard_normal(d), d)
    Apsd, B, cp, cf = _split(A, c, K)
    return A, b, c, K, dAAt, Apsd, B, cp, cf, R


@pytest.mark.parametrize("kind", ["dual", "dual_unitdiag"])
def test_dual_rtr_after_sigma_change(lib, kind):
    """Two trustregions() calls on one handle at the same width, an outer step and a new sigma between them: the second
    call's Hess-vecs use the new sigma (the captured tCG launches are rebuilt), so the RTR matches the restatement again."""
    from oracle.manopt_rtr import trustregions
    rng = np.random.default_rng(3)
    if kind == "dual":
        A, b, c, K, dAAt, _ = _qssos(6)
        Apsd, B, cp, cf = _split(A, c, K)
        n, nf, p = K["s"], K["f"], 5
        prob = G.DualGenericProblem(Apsd, B, b, cp, cf, dAAt, n, p, q1="correct")
        h = lib.Handle.dual(Apsd, b, cp, dAAt, B, cf)
        Y = rng.standard_normal((n, p))
        sigmas = (0.1, 0.4)
    else:
        A, b, c, K, dAAt, Apsd, B, cp, cf, R = _unitdiag_case()
        n, nf, p = K["s"], K["f"], 6
        prob = R._DualUnitDiagProblem(Apsd, B, b, cp, cf, dAAt, n, p)
        h = lib.Handle.dual_unitdiag(Apsd, b, cp, dAAt, B, cf)
        Y = rng.standard_normal((n, p)); Y /= np.linalg.norm(Y, axis=1, keepdims=True)
        sigmas = (1e-3, 4e-3)
    w = np.zeros(nf)
    for k, sigma in enumerate(sigmas):
        prob.sigma, prob.w = sigma, w.copy()
        h.dual_set_penalty(sigma, w)
        h.set_point(Y)
        st = h.rtr(lib.default_opts(maxiter=4, maxinner=20, tolgradnorm=1e-8))
        Yr, fr, info = trustregions(prob, Y.copy(), 4, 20, 1e-8)
        assert (st.hessvecs, st.accepted, st.rejected) == (info.hessvecs, info.accepted, info.rejected), k
        assert abs(st.cost - fr) <= 1e-10 * max(1.0, abs(fr)), k
        assert abs(st.gradnorm - info.gradnorm) <= 1e-8 * max(1.0, info.gradnorm), k
        Y = h.get_point()
        assert _relerr(Y, Yr) < 1e-8, k
        if k == 0:                                         # outer step on the device and in the restatement
            _, _, _, Af, _ = h.dual_outer_step()
            S = Y @ Y.T
            sc = S.ravel(order="F") - cp
            y = prob.iAt @ sc
            As = prob.At @ y - sc
            if kind == "dual":
                prob.x = prob.x + sigma * (prob.iAB @ (Af - w / sigma) + prob.At @ (prob.iAt @ (As - prob.x / sigma)) - As)
            else:
                prob.x = prob.x - sigma * As               # ManiDSDP_unitdiag.m:77
            w = w - sigma * Af
    h.close()


_PRIMAL = {}


def _primal_optimum(d):
    """GPU solvers.ManiSDP on the moment relaxation qsmom(d, coe) of the same quartic."""
    if d not in _PRIMAL:
        from manisdp_matlab_amd import problems, solvers
        At, b, c, K = problems.qsmom(d, _coe(d))
        b = np.asarray(b.todense()).ravel() if hasattr(b, "todense") else np.asarray(b, float)
        c = np.asarray(c.todense()).ravel() if hasattr(c, "todense") else np.asarray(c, float).ravel()
        _, f, data = solvers.ManiSDP(At, b, c, K, {"tol": 1e-8}, verbose=False)
        assert data["status"] == 0
        _PRIMAL[d] = f
    return _PRIMAL[d]


@pytest.mark.parametrize("d,line_search,eig", [(10, 1, "host"), (10, 0, "host"), (10, 1, "device"), (10, 0, "device"),
                                               (20, 1, "host")])
def test_dual_generic_solve_reaches_primal_optimum(lib, d, line_search, eig):
    """example/dual/example_qsphere_dual.m:1-21 (theta = 1e-1, tau2 = 0.5, b/maxb): status 0, eta < 1e-8 and the optimum
    of the primal moment relaxation."""
    from manisdp_matlab_amd import solvers
    A, b, c, K, dAAt, maxb = _qssos(d)
    o = {"tol": 1e-8, "dAAt": dAAt, "theta": 1e-1, "tau2": 0.5, "line_search": line_search, "eig": eig}
    X, obj, data = solvers.ManiDSDP(A, b, c, K, o, verbose=False)
    assert data["g_identity"]
    assert data["status"] == 0 and max(data["gap"], data["pinf"], data["dinf"]) < 1e-8
    f = _primal_optimum(d)
    assert abs(obj * maxb - f) <= 1e-7 * max(1.0, abs(f))
    assert X.shape == (K["s"], K["s"]) and data["y"].shape == b.shape and data["w"].shape == (K["f"],)


def test_dual_generic_width_limit(lib):
    """A factor wider than the dual kinds' 128 columns is an error, not a fault or a wrong answer."""
    A, b, c, K, dAAt, _ = _qssos(6)
    Apsd, B, cp, cf = _split(A, c, K)
    h = lib.Handle.dual(Apsd, b, cp, dAAt, B, cf)
    h.dual_set_penalty(0.1, np.zeros(K["f"]))
    h.set_point(np.random.default_rng(0).standard_normal((K["s"], 130)))
    with pytest.raises(lib.MsdpError):
        h.cost()
    h.close()
