"""GPU tests of the multiblock dual approach (MSDP_KIND_DUAL_MULTIBLOCK, solvers.ManiDSDP_multiblock; reference
src/dual/ManiDSDP_multiblock.m) against the NumPy restatement in dual_multiblock_ref.py.  Operators agree to 1e-11 relative
(fp64, other summation orders); full solves reach the optimum of the primal multiblock solve of the moment relaxation of the
same instance (strong duality, GPU solvers.ManiSDP_multiblock) to 1e-6."""
import os
import sys
import time

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dual_multiblock_ref as R  # noqa: E402
from oracle.manisdp_ref import BlockVec  # noqa: E402

pytestmark = pytest.mark.gpu


def _relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


NSET = [4, 6, 1, 5]          # block 2 lies below min_facsize (p = n = 1)


def _random_instance(nob, nf, m=24, seed=3):
    """Random symmetric constraint matrices, each over one or two blocks, a free part and a PSD cost."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum([n * n for n in NSET])])
    rows = []
    for k in range(m):
        v = np.zeros(off[-1])
        for blk in rng.choice(len(NSET), size=2, replace=True):
            n = NSET[blk]
            Mk = np.zeros((n, n))
            for _ in range(3):
                i, j = rng.integers(0, n, 2)
                a = rng.standard_normal()
                Mk[i, j] += a; Mk[j, i] += a
            v[off[blk]:off[blk + 1]] += Mk.ravel(order="F")
        rows.append(v)
    Apsd = sp.csr_matrix(np.array(rows))
    B = sp.csr_matrix(rng.standard_normal((m, nf)) * (rng.random((m, nf)) < 0.6)) if nf else None
    cp = np.concatenate([(lambda C: 0.2 * (C + C.T))(rng.standard_normal((n, n))).ravel(order="F") for n in NSET])
    cf = rng.standard_normal(nf)
    b = rng.standard_normal(m)
    dAAt = np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel()
    return Apsd, B, b, cp, cf, dAAt


def _pack(blocks, pmax):
    r0 = np.concatenate([[0], np.cumsum(NSET)])
    Y = np.zeros((r0[-1], pmax))
    for i, Yi in enumerate(blocks):
        Y[r0[i]:r0[i + 1], :Yi.shape[1]] = Yi
    return Y


def _unpack(Y, p):
    r0 = np.concatenate([[0], np.cumsum(NSET)])
    return [Y[r0[i]:r0[i + 1], :p[i]] for i in range(len(NSET))]


def _point(rng, p, nob):
    out = []
    for i, (n, pi) in enumerate(zip(NSET, p)):
        Yi = rng.standard_normal((n, pi))
        out.append(Yi / np.linalg.norm(Yi, axis=1, keepdims=True) if i < nob else Yi)
    return BlockVec(out)


def _check_outer(h, prob):
    Yd = h.get_point()
    Y = BlockVec(_unpack(Yd, [prob.M.pset[i] for i in range(len(NSET))]))
    by, cex, as2, Af, z = h.dual_outer_step()
    by_r, cex_r, as2_r, Af_r, z_r, X_r, y_r = prob.outer(Y)
    assert abs(by - by_r) <= 1e-11 * max(1.0, abs(by_r))
    assert abs(cex - cex_r) <= 1e-11 * max(1.0, abs(cex_r))
    assert abs(as2 - as2_r) <= 1e-11 * max(1.0, as2_r)
    if prob.nf:
        assert _relerr(Af, Af_r) < 1e-11
    assert z.shape == z_r.shape and (z.size == 0 or _relerr(z, z_r) < 1e-11)
    r0 = np.concatenate([[0], np.cumsum(NSET)])
    for i, Xi in enumerate(X_r):
        assert _relerr(h.get_dual_slack_block(r0[i], NSET[i]), Xi) < 1e-11, i
    assert _relerr(h.dual_get_y(), y_r) < 1e-11


@pytest.mark.parametrize("nob", [4, 0, 2])
@pytest.mark.parametrize("nf", [0, 2])
def test_dual_multiblock_operators(lib, nob, nf):
    """cost, rgrad, Hess-vec, proj, retr and the line-search cost against the restatement, block widths 3 / 5 / 1 / 2 (pad
    to 5), then the outer step with nonzero x and w."""
    Apsd, B, b, cp, cf, dAAt = _random_instance(nob, nf)
    p = [3, 5, 1, 2]
    pmax = max(p)
    prob = R.DualMultiblockProblem(Apsd, B, b, cp, cf, dAAt, NSET, nob)
    prob.set_widths(p)
    h = lib.Handle.dual_multiblock(Apsd, b, cp, dAAt, NSET, nob, B, cf if nf else None)
    rng = np.random.default_rng(10 * nob + nf)
    # first outer step at a random point (x = 0, w != 0): moves the device-resident x
    prob.sigma, prob.w = 0.37, rng.standard_normal(nf)
    h.dual_set_penalty(prob.sigma, prob.w if nf else None)
    Y0 = _point(rng, p, nob)
    h.set_point(_pack(Y0.b, pmax))
    _check_outer(h, prob)
    # operators at another point, with the updated x and another w, sigma
    prob.sigma, prob.w = 2.3, rng.standard_normal(nf)
    h.dual_set_penalty(prob.sigma, prob.w if nf else None)
    Y = _point(rng, p, nob)
    h.set_point(_pack(Y.b, pmax))
    f = prob.cost(Y)
    assert abs(h.cost() - f) <= 1e-11 * max(1.0, abs(f))
    G = prob.grad(Y)
    assert _relerr(h.rgrad(), _pack(G.b, pmax)) < 1e-11
    Z = BlockVec([rng.standard_normal(yi.shape) for yi in Y.b])
    assert _relerr(h.proj(_pack(Z.b, pmax)), _pack(prob.M.proj(Y, Z).b, pmax)) < 1e-12
    U = prob.M.proj(Y, Z)
    Hd = h.hessvec(_pack(U.b, pmax))
    Hr = _pack(prob.hess(Y, U).b, pmax)
    assert _relerr(Hd, Hr) < 1e-11
    assert np.all(Hd[_pack([np.ones_like(yi) for yi in Y.b], pmax) == 0] == 0)     # pad columns stay zero
    assert _relerr(h.retr(_pack(U.b, pmax)), _pack(prob.M.retr(Y, U).b, pmax)) < 1e-12
    V = BlockVec([rng.standard_normal(yi.shape) for yi in Y.b])
    trial = BlockVec([(yi + 0.3 * vi) / (np.linalg.norm(yi + 0.3 * vi, axis=1, keepdims=True) if i < nob else 1.0)
                      for i, (yi, vi) in enumerate(zip(Y.b, V.b))])
    ft = prob.co(trial)
    assert abs(h.linesearch_cost(_pack(V.b, pmax), 0.3) - ft) <= 1e-11 * max(1.0, abs(ft))
    # second outer step, now with nonzero x
    h.set_point(_pack(Y.b, pmax))
    _check_outer(h, prob)
    h.close()


@pytest.mark.parametrize("maxinner", [1, 3, 20])
def test_dual_multiblock_single_rtr(lib, maxinner):
    """One trustregions() call against the restatement's closures: the same iterations, Hess-vecs, accepted / rejected steps
    and cost."""
    from oracle.manopt_rtr import trustregions
    Apsd, B, b, cp, cf, dAAt = _random_instance(2, 2, seed=5)
    p = [2, 3, 1, 2]
    prob = R.DualMultiblockProblem(Apsd, B, b, cp, cf, dAAt, NSET, 2)
    prob.set_widths(p)
    rng = np.random.default_rng(1)
    prob.sigma, prob.w = 0.5, 0.1 * rng.standard_normal(2)
    h = lib.Handle.dual_multiblock(Apsd, b, cp, dAAt, NSET, 2, B, cf)
    Y = _point(rng, p, 2)
    h.dual_set_penalty(prob.sigma, prob.w)
    h.set_point(_pack(Y.b, 3))
    st = h.rtr(lib.default_opts(maxiter=4, maxinner=maxinner, tolgradnorm=1e-8, Delta_bar=prob.M.typicaldist()))
    Yr, fr, info = trustregions(prob, Y.copy(), 4, maxinner, 1e-8)
    assert st.hessvecs == info.hessvecs
    assert st.iters == info.iters
    assert st.accepted == info.accepted and st.rejected == info.rejected
    assert abs(st.cost - fr) <= 1e-10 * max(1.0, abs(fr))
    assert _relerr(h.get_point(), _pack(Yr.b, 3)) < 1e-8
    h.close()


def test_dual_multiblock_rtr_after_sigma_change(lib):
    """An RTR call after an outer step and a sigma change on one handle equals the same call on a fresh handle."""
    Apsd, B, b, cp, cf, dAAt = _random_instance(4, 1, seed=8)
    p = [2, 3, 1, 2]
    rng = np.random.default_rng(2)
    Y = _point(rng, p, 4)
    h = lib.Handle.dual_multiblock(Apsd, b, cp, dAAt, NSET, 4, B, cf)
    h.dual_set_penalty(0.2, np.zeros(1))
    h.set_point(_pack(Y.b, 3))
    h.rtr(lib.default_opts(maxiter=4, maxinner=20, tolgradnorm=1e-8))
    _, _, _, Af, _ = h.dual_outer_step()
    w = -0.2 * Af
    h.dual_set_penalty(0.8, w)
    Y1 = h.get_point()
    h.set_point(Y1)
    st1 = h.rtr(lib.default_opts(maxiter=4, maxinner=20, tolgradnorm=1e-8))
    # fresh handle with the same multipliers: replay the first outer step there
    h2 = lib.Handle.dual_multiblock(Apsd, b, cp, dAAt, NSET, 4, B, cf)
    h2.dual_set_penalty(0.2, np.zeros(1))
    h2.set_point(Y1)
    h2.dual_outer_step()
    h2.dual_set_penalty(0.8, w)
    h2.set_point(Y1)
    st2 = h2.rtr(lib.default_opts(maxiter=4, maxinner=20, tolgradnorm=1e-8))
    assert (st1.hessvecs, st1.accepted, st1.rejected) == (st2.hessvecs, st2.accepted, st2.rejected)
    assert abs(st1.cost - st2.cost) <= 1e-12 * max(1.0, abs(st2.cost))
    assert np.array_equal(h.get_point(), h2.get_point())
    h.close(); h2.close()


def test_dual_multiblock_width_limit(lib):
    """A factor wider than 128 columns is an error with a message, not a fault or a wrong answer."""
    Apsd, B, b, cp, cf, dAAt = _random_instance(4, 0)
    h = lib.Handle.dual_multiblock(Apsd, b, cp, dAAt, NSET, 0)
    h.dual_set_penalty(0.1)
    h.set_point(np.random.default_rng(0).standard_normal((sum(NSET), 130)))
    with pytest.raises(lib.MsdpError, match="exceeds the supported maximum"):
        h.cost()
    h.close()


# ------------------------------------------------------------------ full solves against the primal multiblock optimum
_PRIMAL = {}


def _bqp(t, q):
    from manisdp_matlab_amd import problems
    cliques, n = problems.chain_cliques(t, q)
    coe = np.random.default_rng(1).standard_normal(len(problems.bqp_sparse_monomials(cliques)))   # example_bqp_sparse.py
    return cliques, n, coe


def _bqp_primal(t, q):
    key = ("bqp", t, q)
    if key not in _PRIMAL:
        from manisdp_matlab_amd import problems, solvers
        cliques, n, coe = _bqp(t, q)
        At, b, c, K = problems.bqpmom_sparse(n, cliques, coe)
        _, f, data = solvers.ManiSDP_multiblock(At, b, c, K, {"tol": 1e-8, "line_search": 1, "tau1": 1}, verbose=False)
        assert data["status"] == 0
        _PRIMAL[key] = f
    return _PRIMAL[key]


def _bqp_dual(t, q, extra=None):
    from manisdp_matlab_amd import problems, solvers
    cliques, n, coe = _bqp(t, q)
    A, b, c, K, dAAt = problems.bqpsos_sparse(n, cliques, problems.bqpsos_sparse_coe(cliques, coe))
    K["nob"] = len(K["s"])
    maxb = float(np.max(np.abs(b)))
    o = {"dAAt": dAAt, "tol": 1e-8}
    o.update(extra or {})
    t0 = time.time()
    X, obj, data = solvers.ManiDSDP_multiblock(A, b / maxb, c, K, o, verbose=False)
    return obj * maxb, data, time.time() - t0, K


def test_dual_multiblock_bqp_example(lib):
    """example/dual/example_bqp_dual_sparse.m at its own size (t = 10, q = 20, K.nob = nb): status 0, eta < 1e-8 and the
    optimum of ManiSDP_multiblock on the moment side."""
    f, data, secs, K = _bqp_dual(10, 20)
    print("\nBQP t = 10 dual multiblock solve: %.2f s, optimum %.8f" % (secs, f))
    assert data["status"] == 0 and max(data["gap"], data["pinf"], data["dinf"]) < 1e-8
    fp = _bqp_primal(10, 20)
    assert abs(f - fp) <= 1e-6 * max(1.0, abs(fp))
    assert len(data["X"]) == len(K["s"]) and data["w"].shape == (1,)


@pytest.mark.parametrize("mode", ["device", "host"])
def test_dual_multiblock_block_eig_modes(lib, mode):
    """Device and host eig(X_i) on 16 blocks both reach eta < 1e-8 with the same optimum (iterates may differ: eigenvectors
    differ by sign or rotation inside eigenspaces)."""
    f, data, _, K = _bqp_dual(16, 8, {"block_eig": mode})
    assert len(K["s"]) == 16
    assert data["status"] == 0 and max(data["gap"], data["pinf"], data["dinf"]) < 1e-8
    fp = _bqp_primal(16, 8)
    assert abs(f - fp) <= 1e-6 * max(1.0, abs(fp))


def test_dual_multiblock_qsphere_example(lib):
    """example/dual/example_qsphere_dual_sparse.m at its own size (t = 4 cliques of 10, K.nob = 0) with its options:
    status 0, eta < 1e-8, and the optimum of ManiSDP_multiblock on qsmom_sparse of the same quartic."""
    from manisdp_matlab_amd import problems, solvers
    cliques, n = problems.chain_cliques(4, 10)
    coe = np.random.default_rng(1).standard_normal(len(problems.quartic_sparse_monomials(cliques)))
    A, b, c, K, dAAt = problems.qssos_sparse(n, cliques, problems.qssos_sparse_coe(cliques, coe))
    K["nob"] = 0
    maxb = float(np.max(np.abs(b)))
    o = {"dAAt": dAAt, "tol": 1e-8, "gama": 2, "alpha": 0.01, "sigma0": 1e-2, "theta": 1e-2, "delta": 6, "line_search": 0}
    t0 = time.time()
    _, obj, data = solvers.ManiDSDP_multiblock(A, b / maxb, c, K, o, verbose=False)
    print("\nquartic t = 4 dual multiblock solve: %.2f s" % (time.time() - t0))
    assert data["status"] == 0 and max(data["gap"], data["pinf"], data["dinf"]) < 1e-8
    At, bp, cp, Kp = problems.qsmom_sparse(n, cliques, coe)
    _, fp, dp = solvers.ManiSDP_multiblock(At, bp, cp, Kp, {"tol": 1e-8, "line_search": 1, "tau1": 1}, verbose=False)
    assert dp["status"] == 0
    assert abs(obj * maxb - fp) <= 1e-6 * max(1.0, abs(fp))


def test_dual_multiblock_large_bqp(lib):
    """t = 100 cliques of 20 (100 blocks of order 211), K.nob = nb: status 0 and the primal multiblock optimum."""
    f, data, secs, _ = _bqp_dual(100, 20)
    print("\nBQP t = 100 dual multiblock solve: %.2f s, %d iterations" % (secs, data["iters"]))
    assert data["status"] == 0 and max(data["gap"], data["pinf"], data["dinf"]) < 1e-8
    fp = _bqp_primal(100, 20)
    assert abs(f - fp) <= 1e-6 * max(1.0, abs(fp))
