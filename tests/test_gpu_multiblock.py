"""GPU parity for the multiblock entry point: ManiSDP_multiblock.m + multiblockmanifold.m
(product of oblique and Euclidean factors; the reference attaches it through the MEX helpers of src/C-files).

Operators through the C ABI against the oracle's restatement of the closures (ManiSDP_multiblock.m:208-249) on a
three-block problem with a Euclidean block, unequal widths and a constraint that couples two blocks; full solves against
SDPLIB known answers (a direct sum of two maxcut problems has the sum of their optima) and against the oracle."""
import json

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden_path

pytestmark = pytest.mark.gpu


def _relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(params=["embedded", "blocked"], autouse=True)
def storage(request, monkeypatch):
    """Every test of this module runs on both representations of the direct sum: the N x N embedding of rounds 2-3 and the
    per-block storage of round 4 (msdp_affine_setup_blocked: memory and work ~ sum n_i^2), which is the default from 16 blocks
    or N = 4096 on."""
    monkeypatch.setenv("MSDP_MULTIBLOCK_BLOCKED", "1" if request.param == "blocked" else "0")
    return request.param


def _dual_slack(h, r0, nset, storage):
    """S as a dense N x N array: in one piece from the embedded form, block by block from the per-block storage."""
    if storage == "embedded":
        return h.get_dual_slack()
    N = int(r0[-1])
    S = np.zeros((N, N))
    for i, n in enumerate(nset):
        S[r0[i]:r0[i + 1], r0[i]:r0[i + 1]] = h.get_dual_slack_block(int(r0[i]), int(n))
    return S


def _random_multiblock(nset, m, seed):
    """SeDuMi data over the concatenated vecs of the blocks: symmetric constraint matrices with a few entries each,
    some of them touching two blocks, dense symmetric costs."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum([n * n for n in nset])])
    rows, cols, vals = [], [], []
    for k in range(m):
        for _ in range(rng.integers(1, 4)):
            i = int(rng.integers(0, len(nset)))
            n = nset[i]
            a, bb = int(rng.integers(0, n)), int(rng.integers(0, n))
            v = rng.standard_normal()
            for (u, w) in {(a, bb), (bb, a)}:
                rows.append(off[i] + u + w * n); cols.append(k); vals.append(v)
    At = sp.coo_matrix((vals, (rows, cols)), shape=(off[-1], m)).tocsc()
    At.sum_duplicates()
    c = []
    for n in nset:
        G = rng.standard_normal((n, n))
        c.append(((G + G.T) / 2).ravel(order="F"))
    return At, rng.standard_normal(m), np.concatenate(c)


def test_multiblock_operators(lib, storage):
    from oracle import manisdp_ref as R
    from manisdp_matlab_amd.solvers import _pack_blocks
    nset, nob, p = [30, 17, 24], 2, [4, 3, 5]
    At, b, c = _random_multiblock(nset, 40, seed=1)
    r0 = np.concatenate([[0], np.cumsum(nset)])
    N, pmax = int(r0[-1]), max(p)
    rng = np.random.default_rng(2)
    M = R.MultiBlockManifold(p, nset, nob)
    Y = M.rand(rng)
    U = R.BlockVec([rng.standard_normal((n, pi)) for n, pi in zip(nset, p)])
    y = 0.1 * rng.standard_normal(b.size)
    sigma = 0.7
    prob = R._MultiBlockProblem(At, b, c, nset, nob)
    prob.M = M
    prob.y, prob.sigma = y, sigma
    f_ref = prob.cost(Y); G_ref = prob.grad(Y); H_ref = prob.hess(Y, U)
    h = lib.Handle.multiblock(At, b, c, nset, nob)
    assert h.get_kind() == lib.KIND_MULTIBLOCK and h.n == N
    h.set_multipliers(y, sigma)
    h.set_point(_pack_blocks(Y.b, r0, N, pmax))
    pack = lambda V: _pack_blocks(V.b, r0, N, pmax)         # noqa: E731
    assert abs(h.cost() - f_ref) <= 1e-11 * max(1.0, abs(f_ref))
    assert _relerr(h.rgrad(), pack(G_ref)) < 1e-11
    assert _relerr(h.hessvec(pack(U)), pack(H_ref)) < 1e-11
    assert _relerr(h.proj(pack(U)), pack(M.proj(Y, U))) < 1e-13
    assert _relerr(h.retr(pack(U)), pack(M.retr(Y, U))) < 1e-13
    # the zero padding of the narrower blocks stays zero under every operator
    for A_ in (h.rgrad(), h.hessvec(pack(U)), h.retr(pack(U))):
        for i in range(len(nset)):
            assert np.all(A_[r0[i]:r0[i + 1], p[i]:] == 0.0)
    # AL bookkeeping: obj, A x, z (zero on the Euclidean block), S blocks (ManiSDP_multiblock.m:65-84)
    obj, Ax = h.al_primal(b.size)
    x = prob._x(Y)
    assert abs(obj - c @ x) <= 1e-11 * max(1.0, abs(c @ x)) and _relerr(Ax, prob.A @ x) < 1e-11
    z = h.al_dual(y)
    S = _dual_slack(h, r0, nset, storage)
    cy = c - prob.At @ y
    for i, n in enumerate(nset):
        Si = cy[prob.off[i]:prob.off[i + 1]].reshape((n, n), order="F")
        if i < nob:
            zi = np.sum((Y.b[i] @ Y.b[i].T) * Si, axis=0)
            Si = Si - np.diag(zi)
            assert _relerr(z[r0[i]:r0[i + 1]], zi) < 1e-11
        else:
            assert np.all(z[r0[i]:r0[i + 1]] == 0.0)
        assert _relerr(S[r0[i]:r0[i + 1], r0[i]:r0[i + 1]], Si) < 1e-11
    # one tCG through the device RTR agrees with the oracle's (Hess-vec count, stop code, cost)
    from oracle import manopt_rtr
    st = h.rtr(lib.default_opts(maxiter=1, maxinner=12, tolgradnorm=1e-9, Delta_bar=M.typicaldist()))
    _, f1, info = manopt_rtr.trustregions(prob, Y, 1, 12, 1e-9)
    assert st.hessvecs == info.hessvecs and st.last_stop_inner == info.stop_inner[-1]
    assert abs(st.cost - f1) <= 1e-10 * max(1.0, abs(f1))
    h.close()


def _maxcut_block(name):
    from manisdp_matlab_amd import problems
    At, b, c, K = problems.from_sdpa(golden_path(name + ".dat-s.gz"))
    return At, np.asarray(b, float), np.asarray(c.todense()).ravel(), K["s"]


def _direct_sum(nob):
    At1, b1, c1, n1 = _maxcut_block("mcp100")
    At2, b2, c2, n2 = _maxcut_block("mcp124-1")
    c = np.concatenate([c1, c2])
    if nob == 2:
        # the manifold enforces every diagonal; SeDuMi data still needs one constraint: X1(1,1) = 1
        At = sp.csc_matrix((np.ones(1), ([0], [0])), shape=(n1 * n1 + n2 * n2, 1)); b = np.ones(1)
    else:
        At = sp.vstack([sp.csc_matrix((n1 * n1, At2.shape[1])), sp.csc_matrix(At2)]).tocsc(); b = b2
    return At, b, c, {"s": [n1, n2], "nob": nob}


def test_multiblock_direct_sum_known_answer(lib):
    """mcp100 (+) mcp124-1 as ONE two-block SDP with both unit diagonals in the product manifold (nob = 2): the optimum
    is the sum of the two SDPLIB values (data/sdplib/README:76-77); the oracle certifies the same."""
    from manisdp_matlab_amd import solvers
    from oracle import manisdp_ref as R
    known = json.load(open(golden_path("known_answers.json")))
    At, b, c, K = _direct_sum(2)
    Y, obj, d = solvers.ManiSDP_multiblock(At, b, c, K, {}, verbose=False)
    assert d["status"] == 0 and max(d["gap"], d["pinf"], d["dinf"]) < 1e-8
    want = -(known["mcp100"] + known["mcp124-1"])
    assert abs(obj - want) <= 1e-6 * abs(want)
    for Yi in Y:
        assert np.abs(np.diag(Yi @ Yi.T) - 1).max() < 1e-12
    Yr, objr, dr = R.ManiSDP_multiblock(At, b, c, K, {})
    assert dr["status"] == 0 and abs(obj - objr) <= 1e-6 * abs(objr)


def test_multiblock_mixed_manifold_follows_the_oracle(lib):
    """nob = 1: the second block is Euclidean and its X_ii = 1 are ordinary affine constraints -- the mixed product
    manifold of multiblockmanifold.m.  On this instance the reference's scheme levels off between 1e-7 and 1e-6 for
    every option set tried (oracle and GPU alike), so the test pins the path instead of the end point: from the same
    start the device solver and the oracle produce the same outer iterates (objective, residues, factor widths) for the
    first twelve AL iterations, and a longer run ends near the known optimum."""
    from manisdp_matlab_amd import solvers
    from oracle import manisdp_ref as R
    known = json.load(open(golden_path("known_answers.json")))
    At, b, c, K = _direct_sum(1)
    n1, n2 = K["s"]
    rng = np.random.default_rng(0)
    Y0 = [rng.standard_normal((n1, 1)), rng.standard_normal((n2, 1))]
    Y0[0] /= np.linalg.norm(Y0[0], axis=1, keepdims=True)
    _, _, d = solvers.ManiSDP_multiblock(At, b, c, K, {"AL_maxiter": 12, "Y0": [y.copy() for y in Y0]}, verbose=False)
    _, _, dr = R.ManiSDP_multiblock(At, b, c, K, {"AL_maxiter": 12, "Y0": R.BlockVec([y.copy() for y in Y0])})
    assert len(d["log"]) == len(dr["log"]) == 12
    for g, r in zip(d["log"], dr["log"]):
        assert g[0] == r[0] and g[6] == r[6]                               # iteration, p_max
        assert abs(g[1] - r[1]) <= 1e-7 * abs(r[1])                        # obj
        for q in (2, 3, 4, 5):                                             # gap, pinf, dinf, gradnorm
            assert abs(g[q] - r[q]) <= 1e-5 * max(abs(r[q]), 1e-8)
    Y, obj, d = solvers.ManiSDP_multiblock(At, b, c, K, {"AL_maxiter": 60}, verbose=False)
    want = -(known["mcp100"] + known["mcp124-1"])
    assert max(d["gap"], d["pinf"], d["dinf"]) < 1e-4 and abs(obj - want) <= 1e-5 * abs(want)
    assert np.abs(np.diag(Y[0] @ Y[0].T) - 1).max() < 1e-12               # the oblique block stays on its manifold


SPARSE_OPTS = {"tol": 1e-8, "line_search": 1, "tau1": 1}          # example_bqp_sparse.m:25-29


@pytest.mark.parametrize("t,q", [(4, 5), (6, 8)])
def test_multiblock_sparse_bqp_matches_oracle(lib, t, q):
    """The workload ManiSDP_multiblock was written for: the sparse second-order moment relaxation of a BQP with chain
    cliques (example_bqp_sparse.m, bqpmom_sparse.m), one unit-diagonal block per clique coupled through the shared moments.
    Same optimum as the oracle, KKT 1e-8, and a lower bound on f over sign vectors (tight on the small chain)."""
    import itertools
    from manisdp_matlab_amd import problems as P, solvers
    from oracle import manisdp_ref as R
    cl, n = P.chain_cliques(t, q)
    mons = P.bqp_sparse_monomials(cl)
    coe = np.random.default_rng(1).standard_normal(len(mons))
    At, b, c, K = P.bqpmom_sparse(n, cl, coe)
    Y, obj, d = solvers.ManiSDP_multiblock(At, b, c, K, dict(SPARSE_OPTS), verbose=False)
    assert d["status"] == 0 and max(d["gap"], d["pinf"], d["dinf"]) < 1e-8
    Yr, objr, dr = R.ManiSDP_multiblock(At, b, c, K, dict(SPARSE_OPTS))
    assert dr["status"] == 0 and abs(obj - objr) <= 1e-7 * abs(objr)
    f = lambda x: sum(cv * np.prod([x[a] for a in mon]) for mon, cv in zip(mons, coe))      # noqa: E731
    if n <= 14:
        best = min(f(x) for x in itertools.product([-1.0, 1.0], repeat=n))
        assert abs(obj - best) <= 1e-7 * abs(best)
    else:
        rng = np.random.default_rng(2)
        assert all(obj <= f(rng.choice([-1.0, 1.0], n)) + 1e-7 for _ in range(50))


@pytest.mark.parametrize("opts", [{"tol": 1e-8}, {"tol": 1e-4, "theta": 1e-4, "tau1": 1e-3, "tau2": 1e-2, "line_search": 0, "alpha": 0.01}])
def test_multiblock_sparse_quartic_matches_oracle(lib, opts):
    """Sparse quartic on clique spheres (example_qsphere_sparse.m, qsmom_sparse.m): K.nob = 0, every block on the Euclidean
    factor of the product manifold.  Defaults to KKT 1e-8, and the example's own options (:25-31, tol 1e-4)."""
    from manisdp_matlab_amd import problems as P, solvers
    from oracle import manisdp_ref as R
    cl, n = P.chain_cliques(4, 5)
    mons = P.quartic_sparse_monomials(cl)
    coe = np.random.default_rng(1).standard_normal(len(mons))
    At, b, c, K = P.qsmom_sparse(n, cl, coe)
    Y, obj, d = solvers.ManiSDP_multiblock(At, b, c, K, dict(opts), verbose=False)
    Yr, objr, dr = R.ManiSDP_multiblock(At, b, c, K, dict(opts))
    assert d["status"] == 0 and dr["status"] == 0
    assert max(d["gap"], d["pinf"], d["dinf"]) < opts["tol"]
    assert abs(obj - objr) <= 10 * opts["tol"] * max(1.0, abs(objr))


def test_dual_slack_block_getter(lib, storage, monkeypatch):
    """msdp_get_dual_slack_block: the diagonal blocks the multiblock host loop reads, against the full N x N download of the
    embedded form (which the per-block storage does not offer: its blocks are checked against the embedded handle's)."""
    At, b, c = _random_multiblock([30, 17, 24], 40, seed=1)
    nset = [30, 17, 24]
    r0 = np.concatenate([[0], np.cumsum(nset)])
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((sum(nset), 4)); Y[:47] /= np.linalg.norm(Y[:47], axis=1, keepdims=True)
    y0, y1 = 0.1 * rng.standard_normal(b.size), 0.1 * rng.standard_normal(b.size)

    def prepared():
        h = lib.Handle.multiblock(At, b, c, nset, 2)
        h.set_multipliers(y0, 0.5)
        h.set_point(Y)
        h.cost()
        h.al_dual(y1)
        return h

    h = prepared()
    blocks = [h.get_dual_slack_block(r0[i], nb) for i, nb in enumerate(nset)]
    if storage == "embedded":
        S = h.get_dual_slack()
        for i, nb in enumerate(nset):
            assert np.array_equal(blocks[i], S[r0[i]:r0[i + 1], r0[i]:r0[i + 1]])
    else:
        monkeypatch.setenv("MSDP_MULTIBLOCK_BLOCKED", "0")
        he = prepared()
        S = he.get_dual_slack()
        he.close()
        for i, nb in enumerate(nset):
            ref = S[r0[i]:r0[i + 1], r0[i]:r0[i + 1]]
            assert np.abs(blocks[i] - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
        with pytest.raises(lib.MsdpError):
            h.get_dual_slack()
        with pytest.raises(lib.MsdpError):
            h.get_dual_slack_block(10, 30)          # not a block of the direct sum
    with pytest.raises(lib.MsdpError):
        h.get_dual_slack_block(60, 20)
    h.close()


def test_block_skip_gives_the_same_results(lib):
    """The contraction of the multiblock kind trims every k slice to the diagonal blocks of its row tile (exact zeros
    elsewhere): cost, gradient, Hess-vec and a trustregions() call against the untrimmed kernels -- many small blocks, so
    that most (row tile, k slice) pairs are skipped, unequal block sizes, blocks that straddle tile boundaries."""
    rng = np.random.default_rng(5)
    nset = [int(v) for v in rng.integers(20, 90, size=24)]
    At, b, c = _random_multiblock(nset, 300, seed=3)
    N, p = sum(nset), 6
    Y = rng.standard_normal((N, p)); Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    U = rng.standard_normal((N, p))
    y = 0.1 * rng.standard_normal(b.size)
    out = []
    for skip in (1, 0):
        h = lib.Handle.multiblock(At, b, c, nset, len(nset))
        h.set_option("block_skip", skip)
        h.set_multipliers(y, 0.5)
        h.set_point(Y)
        f, G, H = h.cost(), h.rgrad(), h.hessvec(h.proj(U))
        st = h.rtr(lib.default_opts(maxiter=4, maxinner=20, tolgradnorm=1e-9))
        out.append((f, G, H, st.cost, st.gradnorm, st.hessvecs, h.get_point()))
        h.close()
    for x, yv in zip(*out):
        assert np.array_equal(np.asarray(x), np.asarray(yv))


def _stacked_maxcut(nblk, n, seed):
    """Direct sum of `nblk` scaled copies of one random MaxCut-like block of order n (unit diagonal everywhere, one trivial
    constraint <E_00, X_1> = 1 as in _direct_sum): the optimum is sum s_i * opt(block)."""
    rng = np.random.default_rng(seed)
    C0 = rng.standard_normal((n, n)); C0 = (C0 + C0.T) / 2; np.fill_diagonal(C0, 0.0)
    scale = 1.0 + (np.arange(nblk) % 2)
    c = np.concatenate([(s * C0).reshape(-1) for s in scale])
    At = sp.csc_matrix(([1.0], ([0], [0])), shape=(nblk * n * n, 1))
    return C0, scale, At, np.array([1.0]), c


def test_dense_slack_entry_points_refuse_a_blocked_handle(lib, storage, monkeypatch):
    """a per-block handle keeps S as the concatenation of its diagonal blocks (sum n_i * nS_i doubles); the entry
    points that read an N x nS matrix must refuse it instead of reading past the buffer (msdp_block_eigs is the per-block call)."""
    if storage == "embedded":
        pytest.skip("per-block storage only")
    monkeypatch.setenv("MSDP_MULTIBLOCK_BLOCKED", "1")
    rng = np.random.default_rng(5)
    nset = [12, 30, 7, 22]
    At, b, c = _random_multiblock(nset, 40, seed=6)
    N, p = sum(nset), 4
    Y = rng.standard_normal((N, p)); Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    y = 0.1 * rng.standard_normal(b.size)
    h = lib.Handle.multiblock(At, b, c, nset, len(nset))
    h.set_multipliers(y, 0.5)
    h.set_point(Y)
    f0 = h.cost()
    h.al_dual(y)
    with pytest.raises(lib.MsdpError, match="msdp_block_eigs"):
        h.escape_eigs_dual(2)
    with pytest.raises(lib.MsdpError, match="get_dual_slack_block"):
        h.get_dual_slack()
    h.set_option("dense_sym", 2)                                    # must not reserve an N x N plan either
    h.set_point(Y)
    assert abs(h.cost() - f0) <= 1e-13 * max(1.0, abs(f0))
    h.close()


def test_blocked_storage_matches_the_embedding(lib, storage, monkeypatch):
    """The two representations of one direct sum: cost, gradient, Hess-vec, A(YY'), the dual step and a trustregions() call
    agree to rounding (different summation orders, so not bit for bit)."""
    if storage == "embedded":
        pytest.skip("one comparison, run from the blocked leg")
    rng = np.random.default_rng(2)
    nset = [int(v) for v in rng.integers(5, 70, size=9)]
    At, b, c = _random_multiblock(nset, 120, seed=4)
    N, p = sum(nset), 5
    nob = 6
    r0 = np.concatenate([[0], np.cumsum(nset)])
    Y = rng.standard_normal((N, p)); Y[:r0[nob]] /= np.linalg.norm(Y[:r0[nob]], axis=1, keepdims=True)
    U = rng.standard_normal((N, p))
    y = 0.1 * rng.standard_normal(b.size)
    out = []
    for mode in ("1", "0"):
        monkeypatch.setenv("MSDP_MULTIBLOCK_BLOCKED", mode)
        h = lib.Handle.multiblock(At, b, c, nset, nob)
        h.set_multipliers(y, 0.5)
        h.set_point(Y)
        f, G, H = h.cost(), h.rgrad(), h.hessvec(h.proj(U))
        ax = h.al_primal(b.size)
        z = h.al_dual(y)
        Sb = [h.get_dual_slack_block(r0[i], n) for i, n in enumerate(nset)]
        st = h.rtr(lib.default_opts(maxiter=3, maxinner=15, tolgradnorm=1e-9))
        out.append([f, G, H, np.concatenate([[ax[0]], ax[1]]), z, np.concatenate([s.ravel() for s in Sb]),
                    st.cost, h.get_point()])
        h.close()
    for i, (x, r) in enumerate(zip(*out)):
        x, r = np.asarray(x, dtype=float), np.asarray(r, dtype=float)
        tol = 1e-12 if i < 6 else 1e-8
        assert np.abs(x - r).max() <= tol * max(1.0, np.abs(r).max()), i


def test_thousand_blocks_of_order_60(lib, storage):
    """N = 60 000 in 1000 blocks.  The embedding would need an N x N contraction (28.8 GB dense); the
    per-block storage holds sum n_i^2 = 3.6e6 entries, is created in < 2 s, and the reference's multiblock loop solves it to
    the sum of the per-block optima."""
    if storage == "embedded":
        pytest.skip("the embedding refuses N = 60 000 with a dense cost (N^2 doubles)")
    import time
    from manisdp_matlab_amd import solvers
    nblk, n = 1000, 60
    C0, scale, At, b, c = _stacked_maxcut(nblk, n, seed=0)
    lib.load()
    free0 = lib.mem_info()[0]
    t0 = time.perf_counter()
    h = lib.Handle.multiblock(At, b, c, [n] * nblk, nblk)
    t_create = time.perf_counter() - t0
    held = free0 - lib.mem_info()[0]
    h.close()
    assert t_create < 2.0, t_create
    # sum n_i^2 doubles = 28.8 MB of S, plus the factor-sized work arrays and the slabs: two orders below the embedding's 28.8 GB
    assert held < 1.5e9, held
    opts = dict(tol=1e-7, p0=[4] * nblk, AL_maxiter=60, seed=0)
    Y, obj, d = solvers.ManiSDP_multiblock(At, b, c, dict(s=[n] * nblk, nob=nblk), dict(opts), verbose=False)
    # one block on its own: X_11 = 1 is implied by the unit diagonal, so the block optimum is the plain MaxCut-like SDP
    _, obj1, d1 = solvers.ManiSDP_onlyunitdiag(C0, dict(tol=1e-9, p0=4, seed=0), verbose=False)
    assert d1["status"] == 0
    ref = scale.sum() * obj1
    assert max(d["gap"], d["pinf"], d["dinf"]) < 1e-6, d
    assert abs(obj - ref) <= 1e-5 * abs(ref), (obj, ref)
    assert len(Y) == nblk and all(Yi.shape[0] == n for Yi in Y)


def test_block_eigs_match_lapack(lib, storage):
    """msdp_block_eigs (one workgroup per block, msdp_blockjacobi.hip), both methods -- tridiagonalisation + bisection + inverse
    iteration and cyclic Jacobi -- against numpy.linalg.eigh on the blocks of a dual slack: orders 1..97 incl. odd ones, 23 blocks;
    eigenvalues to 1e-13 |S_i|, eigenvectors as residuals and orthonormality (the device's basis and LAPACK's differ by signs).
    Clustered, singular and larger blocks: tests/test_gpu_block_eigs.py."""
    rng = np.random.default_rng(11)
    nset = [1, 2, 3, 97, 64, 31] + [int(v) for v in rng.integers(4, 60, size=17)]
    At, b, c = _random_multiblock(nset, 200, seed=8)
    N, p = sum(nset), 4
    r0 = np.concatenate([[0], np.cumsum(nset)])
    h = lib.Handle.multiblock(At, b, c, nset, 10)
    Y = rng.standard_normal((N, p)); Y[:r0[10]] /= np.linalg.norm(Y[:r0[10]], axis=1, keepdims=True)
    h.set_multipliers(0.1 * rng.standard_normal(b.size), 0.5)
    h.set_point(Y)
    h.cost()
    h.al_dual(0.3 * rng.standard_normal(b.size))
    k = 8
    for method in (2, 1):                      # 2: tridiagonalisation + bisection + inverse iteration (the default up to k = 8); 1: Jacobi
      w, V = h.block_eigs(r0[:-1], nset, k, method=method)
      assert w.shape == (N,) and V.shape == (N, k)
      for i, n in enumerate(nset):
          S = h.get_dual_slack_block(r0[i], n)
          S = 0.5 * (S + S.T)
          wr = np.linalg.eigvalsh(S)
          scale = max(1.0, np.abs(wr).max())
          wi = w[r0[i]:r0[i + 1]]
          assert np.all(np.diff(wi) >= 0)
          assert np.abs(wi - wr).max() <= 1e-13 * scale * n
          kk = min(k, n)
          Vi = V[r0[i]:r0[i + 1], :kk]
          assert np.abs(S @ Vi - Vi * wi[:kk]).max() <= 1e-12 * scale * n
          assert np.abs(Vi.T @ Vi - np.eye(kk)).max() <= 1e-12
          assert not np.any(V[r0[i]:r0[i + 1], kk:])                       # columns beyond the block's order
      w2, V2 = h.block_eigs(r0[:-1], nset, k, method=method)             # deterministic
      assert np.array_equal(w, w2) and np.array_equal(V, V2)
    with pytest.raises(lib.MsdpError):
        h.block_eigs(r0[:-1], nset, 9, method=2)                         # the tridiagonal method returns at most 8 vectors
    w9, V9 = h.block_eigs(r0[:-1], nset, 9)                              # ... the default falls back to Jacobi
    assert V9.shape == (N, 9) and np.abs(w9 - w).max() <= 1e-11 * max(1.0, np.abs(w).max())
    with pytest.raises(lib.MsdpError):
        h.block_eigs([0], [N + 1], 1)
    if storage == "blocked":
        with pytest.raises(lib.MsdpError):
            h.block_eigs([2], [2], 1)                                    # rows 2..3 straddle two blocks of the handle
    h.close()


def test_multiblock_solve_with_device_block_eigs(lib, storage):
    """options.block_eig: the reference's host loop of eig(S{i}) against all blocks in one device launch -- same optimum and KKT
    residuals within tol (the iterates differ: Jacobi's eigenvectors are LAPACK's up to signs), on a chain of 18 cliques of 5
    variables (18 blocks of order 16: "auto" takes the device from 16 blocks on)."""
    from manisdp_matlab_amd import problems as P, solvers
    cl, n = P.chain_cliques(18, 5)
    coe = np.random.default_rng(2).standard_normal(len(P.bqp_sparse_monomials(cl)))
    At, b, c, K = P.bqpmom_sparse(n, cl, coe)
    out = {}
    for mode in ("host", "device", "auto"):
        Y, obj, d = solvers.ManiSDP_multiblock(At, b, c, K, {"tol": 1e-8, "line_search": 1, "tau1": 1, "block_eig": mode}, verbose=False)
        assert d["status"] == 0 and max(d["gap"], d["pinf"], d["dinf"]) < 1e-8
        assert len(d["S"]) == len(K["s"]) and d["S"][0].shape == (K["s"][0], K["s"][0])
        out[mode] = obj
    assert abs(out["device"] - out["host"]) <= 1e-6 * abs(out["host"])
    assert abs(out["auto"] - out["host"]) <= 1e-6 * abs(out["host"])


def test_blocked_gram_route_matches_the_sddmm(lib, storage):
    """Per-block storage: A(Y U') through the Gram matrices of the blocks (k_block_gram + k_gram_apply, taken from a panel width on
    where the row gathers of the SDDMM cost four times the Gram matrix) against the SDDMM (option affine_route = 1): cost, gradient,
    Hess-vec, A(YY') at widths 4, 18 and 40."""
    if storage == "embedded":
        pytest.skip("the route of the per-block storage")
    rng = np.random.default_rng(5)
    nset = [int(v) for v in rng.integers(3, 50, size=20)]
    At, b, c = _random_multiblock(nset, 400, seed=6)
    N, nob = sum(nset), 12
    r0 = np.concatenate([[0], np.cumsum(nset)])
    y = 0.1 * rng.standard_normal(b.size)
    for p in (4, 18, 40):
        Y = rng.standard_normal((N, p)); Y[:r0[nob]] /= np.linalg.norm(Y[:r0[nob]], axis=1, keepdims=True)
        U = rng.standard_normal((N, p))
        out = []
        for route in (2, 1):
            h = lib.Handle.multiblock(At, b, c, nset, nob, pcap=p)
            h.set_option("affine_route", route)
            h.set_multipliers(y, 0.7)
            h.set_point(Y)
            f, G, H = h.cost(), h.rgrad(), h.hessvec(h.proj(U))
            obj, Ax = h.al_primal(b.size)
            out.append((f, G, H, Ax, obj))
            h.close()
        for x, r in zip(*out):
            x, r = np.asarray(x, float), np.asarray(r, float)
            assert np.abs(x - r).max() <= 1e-12 * max(1.0, np.abs(r).max())
