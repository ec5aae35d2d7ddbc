"""msdp_block_eigs_large (msdp_blocktridiag.hip: k_block_tridiag_group) -- eig(S_i) of blocks of order 257 .. 1024, a group of
workgroups per block: the planted families of block_eigs_ref.py at 257, 513 and 1024, orders on both sides of the row and workgroup
splits beside small blocks, vector counts, the bitwise properties (repeatable; independent of the other blocks of the call and of
the number of workgroups a block is given), agreement with msdp_block_eigs where both apply, refusals, more blocks than one launch
holds, the natural sources (oblique / Euclidean blocks at a random point, the dual multiblock handle) and a real solve with blocks
of order 277.  Planting, references, tolerances and the per-block assertions are those of tests/test_gpu_block_eigs.py and
tests/block_eigs_ref.py (EIG_TOL 1e-13 n scale, RES_TOL 1e-12 n scale, ORTH_TOL 1e-12): they scale with n and are used unchanged."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_eigs_ref as R  # noqa: E402
from test_gpu_block_eigs import _batches, _check_all, _family1_block, _handle, _arm, _plant, _rows  # noqa: E402

pytestmark = pytest.mark.gpu

LARGE_ORDERS = [257, 513, 1024]


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(params=["embedded", "blocked"], autouse=True)
def storage(request, monkeypatch):
    """Both representations of the direct sum, as in test_gpu_block_eigs.py."""
    monkeypatch.setenv("MSDP_MULTIBLOCK_BLOCKED", "1" if request.param == "blocked" else "0")
    return request.param


@pytest.mark.parametrize("fam", [1, 2, 3, 4, 6])
def test_large_block_eigs_on_planted_families(lib, storage, fam):
    """Families 1, 2, 3, 4 and 6 at orders 257, 513 and 1024 with k = 8: everything check_block asks (eigenvalues, residuals,
    orthonormality, the bottom subspace -- not vacuous in families 1 to 4 --, exact negative / zero counts, zero columns beyond the
    order), and two calls bitwise equal."""
    cases = R.family_cases(fam, mp_orders=(), orders=LARGE_ORDERS)
    assert sorted({c.S.shape[0] for c in cases}) == LARGE_ORDERS
    for batch in _batches(cases, storage, order=lambda c: c.S.shape[0]):
        h, r0, nset, blocks = _plant(lib, [c.S for c in batch])
        w, V = h.block_eigs_large(r0[:-1], nset, 8)
        assert w.shape == (r0[-1],) and V.shape == (r0[-1], 8)
        for i, (c, S) in enumerate(zip(batch, blocks)):
            vac = R.check_block(S, w[_rows(r0, i)], V[_rows(r0, i)], 8, R.reference_eigvals(c, S), floor=c.floor, nneg=c.nneg, nzero=c.nzero,
                                vacuous_ok=c.vacuous_ok, label=f"{c.name} {storage}")
            if fam in (1, 2, 3, 4):
                assert not vac, c.name
        w2, V2 = h.block_eigs_large(r0[:-1], nset, 8)
        assert np.array_equal(w, w2) and np.array_equal(V, V2), "two calls differ"
        h.close()


SPLIT_ORDERS = [257, 1, 300, 3, 511, 512, 64, 513, 211, 1023, 1024]


def _split_sets(storage):
    """The orders of SPLIT_ORDERS: one handle with per-block storage; the embedding takes N < 4096 per handle."""
    if storage == "blocked":
        return [SPLIT_ORDERS]
    return [[257, 1, 300, 3, 511, 512, 64, 513, 211], [1023, 1, 3, 64, 211, 1024]]


def test_large_block_eigs_across_the_splits(lib, storage):
    """Family-1 blocks at 257, 300, 511, 512, 513, 1023 and 1024 -- both sides of the 64-lane row chunks, of a multiple of the group
    size and of the largest order -- beside blocks of order 1, 3, 64 and 211 in the same call."""
    rng = np.random.default_rng(31)
    for orders in _split_sets(storage):
        mats, nz = zip(*[_family1_block(n, rng, nz=(min(8, n - 1) if n > 1 else 0)) for n in orders])
        h, r0, nset, blocks = _plant(lib, mats)
        w, V = h.block_eigs_large(r0[:-1], nset, 8)
        _check_all(blocks, r0, w, V, 8, f"splits {storage}", nz)
        h.close()


def test_large_block_eigs_vector_counts(lib, storage):
    """k in {0, 1, 7, 8}; k = 0 returns V of shape (N, 0) and the eigenvalues of the k = 1 call bit for bit."""
    rng = np.random.default_rng(32)
    orders = [2, 300, 64, 513]
    mats, nz = zip(*[_family1_block(n, rng, nz=(min(8, n - 1) if n > 1 else 0)) for n in orders])
    h, r0, nset, blocks = _plant(lib, mats)
    N, ws = int(r0[-1]), {}
    for k in (0, 1, 7, 8):
        w, V = h.block_eigs_large(r0[:-1], nset, k)
        assert w.shape == (N,) and V.shape == (N, k)
        _check_all(blocks, r0, w, V, k, f"k {k}", nz)
        ws[k] = w
    assert np.array_equal(ws[0], ws[1])
    h.close()


def test_large_block_eigs_bitwise_properties(lib, storage):
    """Two identical calls agree; a subset in reverse order with one block named twice gives, per block, the bits of the full call;
    one large block alone in a call gives the bits it had among many; and so does every number of workgroups per block (option
    "blk_groups": 1, 2, 3, 7, 16 against the default)."""
    rng = np.random.default_rng(33)
    orders = [300, 64, 513, 257, 1024, 40]
    mats, _ = zip(*[_family1_block(n, rng) for n in orders])
    h, r0, nset, blocks = _plant(lib, mats)
    w, V = h.block_eigs_large(r0[:-1], nset, 8)
    _check_all(blocks, r0, w, V, 8, "full call")
    w2, V2 = h.block_eigs_large(r0[:-1], nset, 8)
    assert np.array_equal(w, w2) and np.array_equal(V, V2)

    def same_bits(pick, label):
        pr0 = np.concatenate([[0], np.cumsum([nset[i] for i in pick])])
        ws, Vs = h.block_eigs_large([r0[i] for i in pick], [nset[i] for i in pick], 8)
        assert ws.shape == (pr0[-1],) and Vs.shape == (pr0[-1], 8)
        for q, i in enumerate(pick):
            assert np.array_equal(ws[_rows(pr0, q)], w[_rows(r0, i)]) and np.array_equal(Vs[_rows(pr0, q)], V[_rows(r0, i)]), (label, q, i)

    same_bits([4, 2, 0, 2, 1], "subset")
    for i in (4, 0, 3):
        same_bits([i], "alone")
    for G in (1, 2, 3, 7, 16):
        h.set_option("blk_groups", G)
        same_bits(list(range(len(nset))), f"blk_groups {G}")
        assert h.block_eigs_large_info()[1] == sum(G if n > 256 else 1 for n in nset)
    h.set_option("blk_groups", 0)
    h.close()


def test_large_block_eigs_agree_with_the_one_workgroup_kernel(lib, storage):
    """Orders 129, 211 and 256 (one workgroup here too), against msdp_block_eigs(method = 2): both pass check_block, eigenvalues
    within EIG_TOL n scale of each other (not bitwise: the reductions run in another order)."""
    rng = np.random.default_rng(34)
    mats, nz = zip(*[_family1_block(n, rng) for n in (129, 211, 256)])
    h, r0, nset, blocks = _plant(lib, mats)
    w, V = h.block_eigs_large(r0[:-1], nset, 8)
    wo, Vo = h.block_eigs(r0[:-1], nset, 8, method=2)
    _check_all(blocks, r0, w, V, 8, "large", nz)
    _check_all(blocks, r0, wo, Vo, 8, "one workgroup", nz)
    for i, n in enumerate(nset):
        scale = R.scale_of(wo[_rows(r0, i)])
        assert np.abs(w[_rows(r0, i)] - wo[_rows(r0, i)]).max() <= R.EIG_TOL * n * scale, n
    h.close()


def test_large_block_eigs_refusals(lib, storage):
    """Every bad call is refused on the host with its error class and a message that names the limit and the block; the same handle
    then answers a valid call with the bits it gave before."""
    rng = np.random.default_rng(35)
    mats, _ = zip(*[_family1_block(n, rng) for n in (5, 1025, 300, 12)])
    h, r0, nset = _handle(lib, mats)
    N = int(r0[-1])
    ok = ([int(r0[2]), 0], [300, 5])
    h.set_point(rng.standard_normal((N, 1)))
    with pytest.raises(lib.MsdpError, match=r"error -4: block_eigs_large: call msdp_al_dual first"):        # MSDP_ESTATE
        h.block_eigs_large(*ok, 2)
    _arm(h, N)
    blocks = [h.get_dual_slack_block(int(r0[2]), 300), h.get_dual_slack_block(0, 5)]
    rr = np.array([0, 300, 305])
    w, V = h.block_eigs_large(*ok, 2)
    _check_all(blocks, rr, w, V, 2, "first valid call")
    bad = [
        ((*ok, 9), r"error -6: block_eigs_large: at most 8 eigenvectors per block \(9 asked for\)"),        # MSDP_EUNSUPPORTED
        (([0, int(r0[1])], [5, 1025], 2), r"error -6: block_eigs_large: block orders up to 1024 \(block 1 has 1025\)"),
        (([0, 0], [5, 0], 1), r"error -1: block_eigs_large: block 1 has order 0"),                          # MSDP_EINVAL
        ((*ok, -1), r"error -1: block_eigs_large: bad argument"),
        (([], [], 2), r"error -1: block_eigs_large: bad argument"),
        (([N - 1], [2], 1), r"error -1: block_eigs_large: block 0 outside the matrix"),
        (([-1], [2], 1), r"error -1: block_eigs_large: block 0 outside the matrix"),
    ]
    if storage == "blocked":
        bad.append((([3], [300], 1), r"error -1: block_eigs_large: rows 3\.\.303 \(block 0\) are not one block of this handle"))   # straddles blocks 0 and 1
    for args, msg in bad:
        with pytest.raises(lib.MsdpError, match=msg):
            h.block_eigs_large(*args)
        w2, V2 = h.block_eigs_large(*ok, 2)
        assert np.array_equal(w, w2) and np.array_equal(V, V2), msg
    h.close()


def test_large_block_eigs_more_blocks_than_one_launch(lib, storage):
    """Per-block storage, 40 blocks of orders drawn from 257 .. 400: nine to thirteen workgroups each, more than are resident together
    -- the call runs as consecutive launches (asserted through msdp_block_eigs_large_info) and every block is correct."""
    if storage == "embedded":
        pytest.skip("per-block storage only: the embedding takes at most 15 blocks")
    rng = np.random.default_rng(36)
    orders = [257, 400] + [int(v) for v in rng.integers(257, 401, size=38)]
    mats, nz = zip(*[_family1_block(n, rng) for n in orders])
    h, r0, nset, blocks = _plant(lib, mats)
    t0 = time.perf_counter()
    w, V = h.block_eigs_large(r0[:-1], nset, 8)
    launches, wgs = h.block_eigs_large_info()
    print(f"\n40 blocks of order 257 .. 400: {time.perf_counter() - t0:.3f} s, {launches} launches, {wgs} workgroups")
    assert wgs == sum(min(16, (n + 31) // 32) for n in nset) and wgs > 256
    assert launches > 1
    _check_all(blocks, r0, w, V, 8, "40 blocks", nz)
    h.close()


def test_large_block_eigs_of_oblique_and_euclidean_blocks(lib, storage):
    """The natural input -- S_i = mat(c - At y)_i - diag(z_i) at a random point with random multipliers -- at orders 300 (oblique) and
    513 (Euclidean)."""
    from test_gpu_multiblock import _random_multiblock
    rng = np.random.default_rng(37)
    nset, nob = [300, 513], 1
    At, b, c = _random_multiblock(nset, 200, seed=11)
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
    w, V = h.block_eigs_large(r0[:-1], nset, 8)
    _check_all(blocks, r0, w, V, 8, "oblique / Euclidean")
    w2, V2 = h.block_eigs_large(r0[:-1], nset, 8)
    assert np.array_equal(w, w2) and np.array_equal(V, V2)
    h.close()


@pytest.mark.parametrize("nob", [4, 2])
def test_large_block_eigs_of_the_dual_multiblock_handle(lib, storage, nob, monkeypatch):
    """The dual multiblock handle as the source, after msdp_dual_outer_step at a random point: orders 4, 300, 1, 33."""
    import test_gpu_dual_multiblock as D
    monkeypatch.setattr(D, "NSET", [4, 300, 1, 33])
    nset, p = D.NSET, [3, 5, 1, 2]
    Apsd, B, b, cp, cf, dAAt = D._random_instance(nob, 2)
    h = lib.Handle.dual_multiblock(Apsd, b, cp, dAAt, nset, nob, B, cf)
    rng = np.random.default_rng(38 + nob)
    r0 = np.concatenate([[0], np.cumsum(nset)])
    with pytest.raises(lib.MsdpError, match=r"error -4: block_eigs_large"):
        h.block_eigs_large(r0[:-1], nset, 2)
    for sigma in (0.37, 2.3):
        h.dual_set_penalty(sigma, rng.standard_normal(2))
        h.set_point(D._pack(D._point(rng, p, nob).b, max(p)))
        h.dual_outer_step()
    blocks = [h.get_dual_slack_block(int(r0[i]), n) for i, n in enumerate(nset)]
    assert all(np.abs(Bk).max() > 0 for Bk in blocks if Bk.shape[0] > 1)
    w, V = h.block_eigs_large(r0[:-1], nset, 8)
    _check_all(blocks, r0, w, V, 8, f"dual handle nob {nob}")
    h.close()


def test_multiblock_solve_with_blocks_of_order_277(lib, storage):
    """bqpmom_sparse on chain_cliques(4, 23): 4 oblique blocks of order 277, m = 111 431.  block_eig = "device" ends with status 0 and
    max(gap, pinf, dinf) < 1e-8, its optimum within 1e-6 relative of the "host" solve (the criterion of
    test_multiblock_solve_with_device_block_eigs).  Both solve times are printed; they are not a pass criterion."""
    from manisdp_matlab_amd import problems as P, solvers
    cl, nvar = P.chain_cliques(4, 23)
    coe = np.random.default_rng(1).standard_normal(len(P.bqp_sparse_monomials(cl)))
    At, b, c, K = P.bqpmom_sparse(nvar, cl, coe)
    assert [int(v) for v in K["s"]] == [277] * 4 and At.shape[1] == 111431
    res = {}
    for be in ("device", "host"):
        t0 = time.perf_counter()
        Y, obj, d = solvers.ManiSDP_multiblock(At, b, c, K, {"tol": 1e-8, "line_search": 1, "tau1": 1, "block_eig": be}, verbose=False)
        print(f"\nblock_eig = {be} ({storage}): {time.perf_counter() - t0:.2f} s, obj {obj:.10f}, gap {d['gap']:.1e}, pinf {d['pinf']:.1e}, "
              f"dinf {d['dinf']:.1e}, status {d['status']}")
        res[be] = (obj, d)
    for be in ("device", "host"):
        obj, d = res[be]
        assert d["status"] == 0 and max(d["gap"], d["pinf"], d["dinf"]) < 1e-8, (be, d["status"], d["gap"], d["pinf"], d["dinf"])
    assert abs(res["device"][0] - res["host"][0]) <= 1e-6 * abs(res["host"][0])
