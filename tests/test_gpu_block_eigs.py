"""msdp_block_eigs (msdp_blockjacobi.hip: k_block_tridiag, k_block_jacobi) on the spectra it meets in a solve and at its limits:
rank-deficient, clustered, multiple, graded and structured blocks at orders up to 256, its argument checks, block subsets, many
blocks in one launch, and the sources it reads (planted Euclidean blocks, oblique blocks, the dual multiblock handle, the end state
of a real solve).  Both multiblock solvers take dinf, the negative counts and the escape directions from this call and have no
other check of lambda_min, so an error here goes unnoticed downstream.

Planting.  A multiblock handle with nob = 0 has S = mat(c - At*y); with y = 0 the blocks of S are the blocks of c, so a test
chooses every block.  Each block is read back with get_dual_slack_block and must equal the planted matrix bit for bit; the
reference is computed from what was read back.  Generators, references (mpmath at 40 digits, closed forms, LAPACK) and the
per-block assertions are in block_eigs_ref.py; tests/test_block_eigs_ref_host.py shows that LAPACK uses less than a tenth of the
eigenvalue tolerance.  The tolerances are those of test_gpu_multiblock.py::test_block_eigs_match_lapack.

The subspace check (block_eigs_ref.check_block) is vacuous when the bottom set J is the whole block.  That is asserted not to happen
in families 1 to 4.  It happens by construction where all eigenvalues agree (zero block, a * I), where the call asks for as many
vectors as the block has rows (orders 1, 2, 3 with k = 8), and it may happen in family 6 and on the Laplacian."""
import os
import sys
import time

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_eigs_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MP_ORDERS = {1: (33, 65, 129), 2: (33, 65), 3: (33, 65), 4: (33, 65), 6: (33, 65)}     # as tests/test_block_eigs_ref_host.py


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(params=["embedded", "blocked"], autouse=True)
def storage(request, monkeypatch):
    """Both representations of the direct sum, as in test_gpu_multiblock.py: the N x N embedding and the per-block storage."""
    monkeypatch.setenv("MSDP_MULTIBLOCK_BLOCKED", "1" if request.param == "blocked" else "0")
    return request.param


# ---------------------------------------------------------------------------------------------------------------- planting
def _handle(lib, mats):
    """A multiblock handle, all blocks Euclidean, whose cost blocks are `mats`; one trivial constraint <E_00, X_1> = 1."""
    nset = [int(M.shape[0]) for M in mats]
    for M in mats:
        assert np.array_equal(M, M.T)
    c = np.concatenate([M.ravel(order="F") for M in mats])
    At = sp.csc_matrix(([1.0], ([0], [0])), shape=(c.size, 1))
    h = lib.Handle.multiblock(At, np.ones(1), c, nset, 0)
    return h, np.concatenate([[0], np.cumsum(nset)]).astype(np.int64), nset


def _arm(h, N, seed=0):
    """Any point, y = 0: leaves S_i = mat(c_i) on the device."""
    h.set_multipliers(np.zeros(1), 1.0)
    h.set_point(np.random.default_rng(seed).standard_normal((N, 1)))
    h.cost()
    z = h.al_dual(np.zeros(1))
    assert not np.any(z)


def _plant(lib, mats):
    h, r0, nset = _handle(lib, mats)
    _arm(h, int(r0[-1]))
    blocks = [h.get_dual_slack_block(int(r0[i]), n) for i, n in enumerate(nset)]
    for i, (B, M) in enumerate(zip(blocks, mats)):
        assert np.array_equal(B, M), f"block {i}: the slack is not the planted matrix"
    return h, r0, nset, blocks


def _batches(items, storage, order=lambda it: it.n):
    """Per-block storage takes everything in one handle; the embedding takes at most 15 blocks with N < 4096."""
    if storage == "blocked":
        return [list(items)]
    out, cur, rows = [], [], 0
    for it in items:
        if len(cur) == 15 or rows + order(it) >= 4096:
            out.append(cur); cur, rows = [], 0
        cur.append(it); rows += order(it)
    if cur:
        out.append(cur)
    return out


def _rows(r0, i):
    return slice(int(r0[i]), int(r0[i + 1]))


def _family1_block(n, rng, nz=None):
    """One rank-deficient PSD block of order n (family 1): nz exact zeros (default: drawn from the family's list)."""
    if nz is None:
        nz = int(rng.choice(R.deficiencies(n))) if n >= 2 else 0
    return R.dense(np.concatenate([np.zeros(nz), R.upper_part(n - nz, rng)]), rng), nz


def _check_all(blocks, r0, w, V, k, label, nz=None):
    """check_block on every block of a call against LAPACK; the subspace check is vacuous exactly where the call asks for as many
    vectors as the block has rows."""
    for i, S in enumerate(blocks):
        n = S.shape[0]
        vac = R.check_block(S, w[_rows(r0, i)], V[_rows(r0, i)], k, nzero=(nz[i] if nz else 0), label=f"{label} block {i} (n={n})")
        if k:
            assert vac == (min(k, n) == n), f"{label} block {i} (n={n})"


# ---------------------------------------------------------------------------------------------------------- matrix families
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_block_eigs_on_planted_families(lib, storage, fam):
    """Families 1 to 6 of block_eigs_ref.py at orders 63 .. 256 on both sides of 64 and 128 (family 5 also at 1, 2, 3), the tridiagonal
    method with k = 8 and Jacobi with k = 8 and 9: ascending eigenvalues within 1e-13 n scale of the reference, residuals within
    1e-12 n scale, |V'V - I| <= 1e-12, zero columns beyond a block's order, the returned vectors inside the eigenspace of the bottom
    set to 1e-12 n scale / gap, exact negative counts (family 2), repeated calls bitwise equal, method 0 bitwise equal to method 2
    (k = 8) and to method 1 (k = 9)."""
    cases = R.family_cases(fam, mp_orders=MP_ORDERS.get(fam, ()))
    t_ref = 0.0
    for batch in _batches(cases, storage):
        h, r0, nset, blocks = _plant(lib, [c.S for c in batch])
        t0 = time.perf_counter()
        refs = [R.reference_eigvals(c, S) for c, S in zip(batch, blocks)]
        t_ref += time.perf_counter() - t0
        got = {}
        for method, k in ((2, 8), (1, 8), (1, 9)):
            w, V = h.block_eigs(r0[:-1], nset, k, method=method)
            assert w.shape == (r0[-1],) and V.shape == (r0[-1], k)
            got[method, k] = (w, V)
            for i, (c, S) in enumerate(zip(batch, blocks)):
                vac = R.check_block(S, w[_rows(r0, i)], V[_rows(r0, i)], k, refs[i], floor=c.floor, nneg=c.nneg, nzero=c.nzero,
                                    vacuous_ok=c.vacuous_ok, label=f"{c.name} method {method} k {k} {storage}")
                if fam in (1, 2, 3, 4):
                    assert not vac, c.name
            if k == 8:
                w2, V2 = h.block_eigs(r0[:-1], nset, k, method=method)
                assert np.array_equal(w, w2) and np.array_equal(V, V2), f"method {method}: two calls differ"
        for k, same in ((8, 2), (9, 1)):
            w0, V0 = h.block_eigs(r0[:-1], nset, k)
            assert np.array_equal(w0, got[same, k][0]) and np.array_equal(V0, got[same, k][1]), f"method 0, k = {k}"
        h.close()
    print(f"\nfamily {fam} ({storage}): {len(cases)} blocks, references {t_ref:.1f} s")


# ------------------------------------------------------------------------------------------------------ arguments and sources
def test_block_eigs_vector_counts(lib, storage):
    """k in {0, 1, 2, 7, 8} on the tridiagonal method and {0, 1, 9, 33, 64} on Jacobi, blocks of order 1, 2, 3 (k > n_i) beside
    large ones in one call.  k = 0 returns V of shape (N, 0) and the eigenvalues of the k = 1 call, bit for bit."""
    rng = np.random.default_rng(21)
    orders = [1, 2, 3, 64, 129, 40, 256, 211]
    mats, nz = zip(*[_family1_block(n, rng, nz=(min(8, n - 1) if n > 1 else 0)) for n in orders])
    h, r0, nset, blocks = _plant(lib, mats)
    N = int(r0[-1])
    for method, ks in ((2, (0, 1, 2, 7, 8)), (1, (0, 1, 9, 33, 64))):
        ws = {}
        for k in ks:
            w, V = h.block_eigs(r0[:-1], nset, k, method=method)
            assert w.shape == (N,) and V.shape == (N, k)
            _check_all(blocks, r0, w, V, k, f"method {method} k {k}", nz)
            ws[k] = w
        assert np.array_equal(ws[0], ws[1])
    h.close()


def test_block_eigs_refusals(lib, storage):
    """Every bad call is refused on the host with its error class and message, and the same handle then answers a valid call with
    the result it gave before."""
    rng = np.random.default_rng(22)
    mats, _ = zip(*[_family1_block(n, rng) for n in (5, 257, 12)])
    h, r0, nset = _handle(lib, mats)
    N = int(r0[-1])
    ok = ([0, int(r0[2])], [5, 12])
    h.set_point(rng.standard_normal((N, 1)))
    with pytest.raises(lib.MsdpError, match=r"error -4: block_eigs: call msdp_al_dual first"):          # MSDP_ESTATE
        h.block_eigs(*ok, 2)
    _arm(h, N)
    blocks = [h.get_dual_slack_block(0, 5), h.get_dual_slack_block(int(r0[2]), 12)]
    assert np.array_equal(blocks[0], mats[0]) and np.array_equal(blocks[1], mats[2])
    rr = np.array([0, 5, 17])
    w, V = h.block_eigs(*ok, 2)
    _check_all(blocks, rr, w, V, 2, "first valid call")
    bad = [
        ((*ok, 65), {}, r"error -1: block_eigs: bad argument"),                                          # MSDP_EINVAL
        ((*ok, -1), {}, r"error -1: block_eigs: bad argument"),
        ((*ok, 2), {"method": 3}, r"error -1: block_eigs: bad argument"),
        ((*ok, 9), {"method": 2}, r"error -6: block_eigs: the tridiagonal method returns at most 8"),   # MSDP_EUNSUPPORTED
        (([0, 5], [5, 257], 2), {}, r"error -6: block_eigs: block orders up to 256 \(block 1 has 257\)"),
        (([], [], 2), {}, r"error -1: block_eigs: bad argument"),                                        # nb = 0
        (([N - 1], [2], 1), {}, r"error -1: block_eigs: block 0 outside the matrix"),
        (([-1], [2], 1), {}, r"error -1: block_eigs: block 0 outside the matrix"),
        (([0], [0], 1), {}, r"error -6: block_eigs: block orders up to 256"),
    ]
    for args, kw, msg in bad:
        with pytest.raises(lib.MsdpError, match=msg):
            h.block_eigs(*args, **kw)
        w2, V2 = h.block_eigs(*ok, 2)
        assert np.array_equal(w, w2) and np.array_equal(V, V2), msg
    h.close()


def test_block_eigs_follow_the_order_of_the_call(lib, storage):
    """A subset of the handle's blocks in reverse order, one of them named twice: the rows of w and V follow the call, and every
    block's result equals, bit for bit, what the call over all blocks gave for it."""
    rng = np.random.default_rng(23)
    mats, _ = zip(*[_family1_block(n, rng) for n in (3, 65, 128, 17, 129, 40)])
    h, r0, nset, blocks = _plant(lib, mats)
    pick = [4, 2, 0, 2]
    pr0 = np.concatenate([[0], np.cumsum([nset[i] for i in pick])])
    for method, k in ((2, 8), (1, 9)):
        w, V = h.block_eigs(r0[:-1], nset, k, method=method)
        ws, Vs = h.block_eigs([r0[i] for i in pick], [nset[i] for i in pick], k, method=method)
        assert ws.shape == (pr0[-1],) and Vs.shape == (pr0[-1], k)
        _check_all([blocks[i] for i in pick], pr0, ws, Vs, k, f"subset, method {method}")
        for q, i in enumerate(pick):
            assert np.array_equal(ws[_rows(pr0, q)], w[_rows(r0, i)]) and np.array_equal(Vs[_rows(pr0, q)], V[_rows(r0, i)]), (method, q)
    h.close()


def test_block_eigs_three_hundred_blocks(lib, storage):
    """Per-block storage, 300 rank-deficient blocks of orders drawn from 1 .. 256 (1, 255 and 256 among them) in one launch per
    method; then fewer and smaller blocks on the same handle (the workspace is kept), then all of them with Jacobi (it grows), the
    small set again, and the first call once more, bit for bit."""
    if storage == "embedded":
        pytest.skip("per-block storage only: the embedding takes at most 15 blocks")
    rng = np.random.default_rng(24)
    orders = [1, 255, 256] + [int(v) for v in rng.integers(1, 257, size=297)]
    mats, nz = zip(*[_family1_block(n, rng) for n in orders])
    h, r0, nset, blocks = _plant(lib, mats)
    small = [i for i, n in enumerate(nset) if n <= 64][:40]
    sr0 = np.concatenate([[0], np.cumsum([nset[i] for i in small])])

    def all_blocks(method):
        t0 = time.perf_counter()
        w, V = h.block_eigs(r0[:-1], nset, 8, method=method)
        print(f"\n300 blocks, method {method}: {time.perf_counter() - t0:.3f} s")
        _check_all(blocks, r0, w, V, 8, f"300 blocks, method {method}", nz)
        return w, V

    def small_blocks(method):
        w, V = h.block_eigs([r0[i] for i in small], [nset[i] for i in small], 8, method=method)
        _check_all([blocks[i] for i in small], sr0, w, V, 8, f"40 small blocks, method {method}", [nz[i] for i in small])

    w, V = all_blocks(2)
    small_blocks(2)
    all_blocks(1)
    small_blocks(1)
    w2, V2 = h.block_eigs(r0[:-1], nset, 8, method=2)
    assert np.array_equal(w, w2) and np.array_equal(V, V2)
    h.close()


def test_block_eigs_of_a_sub_range(lib, storage):
    """The embedding takes any diagonal sub-matrix of S (soff = row0 * nS + row0): a range that straddles two planted blocks gives
    the eigen-decomposition of that sub-matrix.  The per-block storage refuses a range that is not one of its blocks."""
    rng = np.random.default_rng(25)
    mats, _ = zip(*[_family1_block(n, rng) for n in (20, 31, 9)])
    h, r0, nset, blocks = _plant(lib, mats)
    lo, n = 12, 25                                                   # rows 12 .. 36: the end of block 0 and the start of block 1
    if storage == "blocked":
        with pytest.raises(lib.MsdpError):
            h.block_eigs([lo], [n], 4)
    else:
        S = h.get_dual_slack()[lo:lo + n, lo:lo + n]
        want = np.zeros((n, n))
        want[:8, :8] = mats[0][12:, 12:]
        want[8:, 8:] = mats[1][:17, :17]
        assert np.array_equal(S, want)
        for method in (2, 1):
            w, V = h.block_eigs([lo], [n], 4, method=method)
            R.check_block(S, w, V, 4, label=f"sub-range, method {method}")
    w, V = h.block_eigs(r0[:-1], nset, 4)                            # the handle's own blocks, after the refusal too
    _check_all(blocks, r0, w, V, 4, "own blocks")
    h.close()


def test_block_eigs_oblique_blocks_of_large_order(lib, storage):
    """The natural input of test_block_eigs_match_lapack -- S_i = mat(c - At y)_i - diag(z_i) at a random point with random
    multipliers -- at the orders it leaves out: 129, 211 (oblique) and 256 (Euclidean)."""
    from test_gpu_multiblock import _random_multiblock
    rng = np.random.default_rng(26)
    nset, nob = [129, 211, 256], 2
    At, b, c = _random_multiblock(nset, 200, seed=9)
    r0 = np.concatenate([[0], np.cumsum(nset)])
    N = int(r0[-1])
    h = lib.Handle.multiblock(At, b, c, nset, nob)
    Y = rng.standard_normal((N, 4)); Y[:r0[nob]] /= np.linalg.norm(Y[:r0[nob]], axis=1, keepdims=True)
    h.set_multipliers(0.1 * rng.standard_normal(b.size), 0.5)
    h.set_point(Y)
    h.cost()
    z = h.al_dual(0.3 * rng.standard_normal(b.size))
    assert np.all(z[:r0[nob]] != 0.0) and not np.any(z[r0[nob]:])
    blocks = [h.get_dual_slack_block(int(r0[i]), n) for i, n in enumerate(nset)]
    for method, k in ((2, 8), (1, 8)):
        w, V = h.block_eigs(r0[:-1], nset, k, method=method)
        _check_all(blocks, r0, w, V, k, f"oblique, method {method}")
        w2, V2 = h.block_eigs(r0[:-1], nset, k, method=method)
        assert np.array_equal(w, w2) and np.array_equal(V, V2)
    h.close()


@pytest.mark.parametrize("nob", [4, 2])
def test_block_eigs_of_the_dual_multiblock_handle(lib, storage, nob, monkeypatch):
    """The dual multiblock handle as the source: after msdp_dual_outer_step at a random point the call reads X_i = mat(x + bA)_i -
    diag(z_i); orders 4, 150, 1, 33, all blocks with unit diagonal (nob = nb) and the first two only."""
    import test_gpu_dual_multiblock as D
    monkeypatch.setattr(D, "NSET", [4, 150, 1, 33])
    nset, p = D.NSET, [3, 5, 1, 2]
    Apsd, B, b, cp, cf, dAAt = D._random_instance(nob, 2)
    h = lib.Handle.dual_multiblock(Apsd, b, cp, dAAt, nset, nob, B, cf)
    rng = np.random.default_rng(27 + nob)
    r0 = np.concatenate([[0], np.cumsum(nset)])
    with pytest.raises(lib.MsdpError, match=r"error -4: block_eigs"):
        h.block_eigs(r0[:-1], nset, 2)
    for sigma in (0.37, 2.3):                                         # the second step starts from a nonzero x
        h.dual_set_penalty(sigma, rng.standard_normal(2))
        h.set_point(D._pack(D._point(rng, p, nob).b, max(p)))
        h.dual_outer_step()
    blocks = [h.get_dual_slack_block(int(r0[i]), n) for i, n in enumerate(nset)]
    assert all(np.abs(Bk).max() > 0 for Bk in blocks if Bk.shape[0] > 1)          # (an oblique block of order 1 is x - z = 0)
    for method, k in ((2, 8), (1, 8), (1, 9)):
        w, V = h.block_eigs(r0[:-1], nset, k, method=method)
        _check_all(blocks, r0, w, V, k, f"dual handle nob {nob}, method {method}")
    h.close()


# ------------------------------------------------------------------------------------------------------------ a real end state
END_STATE_CLIQUES, END_STATE_Q = 6, 16


def test_block_eigs_at_the_end_state_of_a_solve(lib, storage):
    """The slack at the end of a real solve: a bqpmom_sparse chain of 6 cliques of 16 variables (6 blocks of order 137) solved with
    block_eig = "host" to tol 1e-8; the state is re-created at the returned point and multipliers and both methods (k = 8) are
    compared with eigh of the fetched blocks -- eigenvalues, residuals, orthonormality, the bottom subspace, and dinf from the
    device's extreme eigenvalues against dinf from LAPACK's to 1e-13 n.  The solve time is printed; it is not a pass criterion."""
    from manisdp_matlab_amd import problems as P, solvers
    cl, nvar = P.chain_cliques(END_STATE_CLIQUES, END_STATE_Q)
    coe = np.random.default_rng(1).standard_normal(len(P.bqp_sparse_monomials(cl)))
    At, b, c, K = P.bqpmom_sparse(nvar, cl, coe)
    t0 = time.perf_counter()
    Y, obj, d = solvers.ManiSDP_multiblock(At, b, c, K, {"tol": 1e-8, "line_search": 1, "tau1": 1, "block_eig": "host"}, verbose=False)
    print(f"\nend state: {len(K['s'])} blocks of order {max(K['s'])}, solve {time.perf_counter() - t0:.2f} s, "
          f"dinf {d['dinf']:.2e}, widths {d['p']}")
    assert d["status"] == 0 and max(d["gap"], d["pinf"], d["dinf"]) < 1e-8
    nset = [int(v) for v in K["s"]]
    r0 = np.concatenate([[0], np.cumsum(nset)])
    N, pmax = int(r0[-1]), max(d["p"])
    h = lib.Handle.multiblock(sp.csc_matrix(At), solvers._dense_vec(b), solvers._dense_vec(c), nset, int(K["nob"]), pcap=max(32, pmax + 2))
    h.set_multipliers(d["y"], 1.0)
    h.set_point(solvers._pack_blocks(Y, r0, N, pmax))
    h.cost()
    h.al_dual(d["y"])
    blocks = [h.get_dual_slack_block(int(r0[i]), n) for i, n in enumerate(nset)]
    dinf_host = max(solvers._dinf_abs(wr[0], wr[-1]) for wr in (np.linalg.eigvalsh(0.5 * (S + S.T)) for S in blocks))
    for method in (2, 1):
        w, V = h.block_eigs(r0[:-1], nset, 8, method=method)
        _check_all(blocks, r0, w, V, 8, f"end state, method {method}")
        dinf_dev = max(solvers._dinf_abs(w[r0[i]], w[r0[i + 1] - 1]) for i in range(len(nset)))
        assert abs(dinf_dev - dinf_host) <= 1e-13 * max(nset), (method, dinf_dev, dinf_host)
    h.close()
