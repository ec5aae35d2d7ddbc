"""msdp_block_reshape (msdp_blockreshape.hip: k_breshape_decide, k_breshape_apply) -- rank cut and escape widening of all blocks of a
multiblock factor in one call, against the NumPy restatement in block_reshape_ref.py.

Factors are planted (Y_i = A diag(s) B' with singular values a factor 10 and more from theta e_1 on either side), w and V are supplied
by the test, so the expected counts are exact and X_i = Y_i^new Y_i^new' is unique; it is compared within block_reshape_ref.X_TOL
(ten times what the float64 restatement itself deviates from an extended-precision evaluation of the same cases; the host test file
measures that).  msdp_get_point after the call is the only read-back of a point."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_reshape_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

PRIMAL = dict(theta=1e-2, strict=False, delta=8, alpha=0.1, min_facsize=2)
DUAL = dict(PRIMAL, theta=1e-3, strict=True)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(params=["embedded", "blocked"])
def storage(request, monkeypatch):
    monkeypatch.setenv("MSDP_MULTIBLOCK_BLOCKED", "1" if request.param == "blocked" else "0")
    return request.param


def _handle(lib, nset, nob, pcap=32, seed=0):
    """A primal multiblock handle with random symmetric cost blocks and one trivial constraint <E_00, X_1> = 1."""
    rng = np.random.default_rng(seed)
    mats = [(lambda M: 0.5 * (M + M.T))(rng.standard_normal((n, n))) for n in nset]
    c = np.concatenate([M.ravel(order="F") for M in mats])
    At = sp.csc_matrix(([1.0], ([0], [0])), shape=(c.size, 1))
    h = lib.Handle.multiblock(At, np.ones(1), c, nset, nob, pcap=pcap)
    h.set_multipliers(np.zeros(1), 1.0)
    return h, mats


def _dual_handle(lib, nset, nob, monkeypatch, pcap=32):
    import test_gpu_dual_multiblock as D
    monkeypatch.setattr(D, "NSET", list(nset))
    Apsd, B, b, cp, cf, dAAt = D._random_instance(nob, 2)
    return lib.Handle.dual_multiblock(Apsd, b, cp, dAAt, nset, nob, B, cf, pcap=pcap)


def _layout(cases):
    nset = [c.n for c in cases]
    r0 = np.concatenate([[0], np.cumsum(nset)]).astype(np.int64)
    p = [c.p for c in cases]
    Y = np.zeros((int(r0[-1]), max(p)))
    for i, c in enumerate(cases):
        Y[r0[i]:r0[i + 1], :c.p] = c.Y
    return nset, r0, p, Y, np.concatenate([c.w for c in cases]), np.vstack([c.V for c in cases])


def _call(h, cases, rule, mode, set_point=True):
    nset, r0, p, Y, w, V = _layout(cases)
    if set_point:
        h.set_point(Y)
    out = h.block_reshape(r0[:-1], nset, p, w, V, rule["theta"], rule["strict"], rule["delta"], rule["alpha"], rule["min_facsize"], mode)
    return out, h.get_point(), r0, Y


def _check(h, cases, nob, rule, mode, out, Ynew, r0, Yold, label=""):
    """Counts, X_i, exact zeros beyond every new width, the handle's width, U, untouched blocks bitwise."""
    p_out, r_out, nne_out, U = out
    refs = [R.reshape_block(c.Y, c.w, c.V, mode=mode, oblique=i < nob, **rule) for i, c in enumerate(cases)]
    assert h.p == Ynew.shape[1] == max(ref["p_out"] for ref in refs), label
    assert (U is None) == (mode == 0)
    for i, (c, ref) in enumerate(zip(cases, refs)):
        tag = f"{label} block {i} (n={c.n}, p={c.p})"
        assert (int(p_out[i]), int(nne_out[i])) == (ref["p_out"], ref["nne"]), tag
        if c.n >= rule["min_facsize"] and c.p > 1:
            assert int(r_out[i]) == ref["r"], tag
        rows = slice(int(r0[i]), int(r0[i + 1]))
        Yi = Ynew[rows, :ref["p_out"]]
        assert not np.any(Ynew[rows, ref["p_out"]:]), tag
        if c.n < rule["min_facsize"]:
            assert np.array_equal(Yi, Yold[rows, :c.p]), tag
        X = Yi @ Yi.T
        err, nrm = np.linalg.norm(X - ref["X"]), np.linalg.norm(ref["X"])
        assert err <= R.X_TOL * nrm, (tag, err / nrm if nrm else err)
        if mode == 1:
            assert np.array_equal(U[rows, :ref["p_out"]], ref["U"]) and not np.any(U[rows, ref["p_out"]:]), tag
            assert not np.any(Yi[:, ref["p_out"] - ref["nne"]:]), tag
    return refs


@pytest.mark.parametrize("nob", [0, 4, 7])
@pytest.mark.parametrize("mode", [0, 1])
def test_seven_orders_and_widths_in_one_handle(lib, storage, nob, mode):
    """Orders 1, 2, 3, 63, 64, 65, 257 with widths 1, 2, 8, 9, 32, 33, 64 in one handle, min_facsize 2 (order 1 untouched) and 1."""
    cases = R.seven_blocks(np.random.default_rng(81))
    h, _ = _handle(lib, [c.n for c in cases], nob, pcap=80)
    for mf in (2, 1):
        rule = dict(PRIMAL, min_facsize=mf)
        out, Ynew, r0, Yold = _call(h, cases, rule, mode)
        _check(h, cases, nob, rule, mode, out, Ynew, r0, Yold, f"{storage} nob {nob} mode {mode} min_facsize {mf}")
    h.close()


def test_strict_rank_on_the_dual_handle(lib, monkeypatch):
    """The dual multiblock handle with the dual kinds' rule (theta 1e-3, strict >): a mixed set, both modes."""
    rng = np.random.default_rng(82)
    cases = [R.Case(n, p, keep, nneg, 8, rng) for n, p, keep, nneg in ((12, 5, 2, 1), (33, 9, 9, 0), (1, 1, 1, 2), (20, 2, 1, 9))]
    for nob in (4, 2):
        h = _dual_handle(lib, [c.n for c in cases], nob, monkeypatch)
        for mode in (0, 1):
            out, Ynew, r0, Yold = _call(h, cases, DUAL, mode)
            _check(h, cases, nob, DUAL, mode, out, Ynew, r0, Yold, f"dual nob {nob} mode {mode}")
        h.close()


@pytest.mark.parametrize("nob", [0, 3])
@pytest.mark.parametrize("mode", [0, 1])
def test_uncut_wide_blocks_grow_past_column_64(lib, storage, nob, mode):
    """Blocks of width 57, 60 and 64 at full rank with 8 and more negative eigenvalues: nothing is cut and the new widths are 65, 68
    and 72 -- the escape columns land beyond column 63, where one lane per column would end.  Handle with room for 80 columns."""
    cases = R.wide_uncut_blocks()
    h, _ = _handle(lib, [c.n for c in cases], nob, pcap=80)
    out, Ynew, r0, Yold = _call(h, cases, PRIMAL, mode)
    assert [int(v) for v in out[0]] == [65, 68, 72] and [int(v) for v in out[2]] == [8, 8, 8] and h.p == 72
    _check(h, cases, nob, PRIMAL, mode, out, Ynew, r0, Yold, f"wide uncut {storage} nob {nob} mode {mode}")
    if mode == 0:
        for i, c in enumerate(cases):                               # the escape columns themselves, beyond column 63
            blk = Ynew[int(r0[i]):int(r0[i + 1])]
            assert np.all(np.linalg.norm(blk[:, 64:int(out[0][i])], axis=0) > 0), i
    # the same blocks on a handle without that room: refused, point unchanged
    h32, _ = _handle(lib, [c.n for c in cases], nob, pcap=64)
    nset, r0, p, Y, w, V = _layout(cases)
    h32.set_point(Y)
    with pytest.raises(lib.MsdpError, match=r"error -6: block_reshape: new width 72 exceeds the allocated width 64"):
        h32.block_reshape(r0[:-1], nset, p, w, V, 1e-2, 0, 8, 0.1, 2, mode)
    assert h32.p == 64 and np.array_equal(h32.get_point(), Y)
    h.close(); h32.close()


@pytest.mark.parametrize("strict", [False, True])
def test_every_branch_of_the_rule(lib, storage, strict):
    """n < min_facsize untouched bitwise; p = 1 (no cut); the zero Euclidean block -- e = 0: strict counts nothing and r is forced
    to 1, non-strict counts every e >= 0 and keeps the width, as the host loop does; nneg = 0 on an oblique block (nne = 1) and on a
    Euclidean one (nne = 0); nneg > delta; p + nne > n -> nne = 0; the width of the handle shrinking and growing."""
    rng = np.random.default_rng(81)
    R.seven_blocks(rng)                                              # (the generator state the reference measurement used)
    B = R.branch_blocks(rng)
    rule = dict(PRIMAL, strict=strict)
    order = ["nneg0", "small", "p1", "zero", "many", "full", "shrink"]   # nneg0 first: oblique; its Euclidean twin below
    twin = R.Case(10, 4, 2, 0, 8, np.random.default_rng(83))
    cases = [B[k] for k in order] + [twin]
    h, _ = _handle(lib, [c.n for c in cases], 1)
    out, Ynew, r0, Yold = _call(h, cases, rule, 0)
    refs = _check(h, cases, 1, rule, 0, out, Ynew, r0, Yold, f"branches strict {strict}")
    by = dict(zip(order + ["twin"], refs))
    assert by["nneg0"]["nne"] == 1 and by["twin"]["nne"] == 0
    assert by["small"]["p_out"] == 1 and by["p1"]["r"] == 1 and by["p1"]["nne"] == 2
    assert by["zero"]["r"] == (1 if strict else 3) and by["zero"]["nne"] == 0
    assert by["many"]["nne"] == 8 and by["full"]["nne"] == 0 and by["full"]["p_out"] == 6
    assert by["shrink"]["r"] == 2
    assert h.p == 11 > 10                                            # grew overall: 'many' 3 -> 11
    # shrinking overall: the wide block alone decides the width
    cases2 = [B["shrink"], B["p1"]]
    h2, _ = _handle(lib, [c.n for c in cases2], 0)
    out, Ynew, r0, Yold = _call(h2, cases2, rule, 0)
    _check(h2, cases2, 0, rule, 0, out, Ynew, r0, Yold, "shrink")
    assert h2.p == 3 < 10
    h.close(); h2.close()


def test_mode_one_direction_and_line_search_cost(lib, storage):
    """mode 1: U = [0, V(:, :nne)] bit for bit, the point is the cut factor with zero columns (both in _check), and
    linesearch_cost(U, a) on it equals the value at the pair the host loop builds.  The two points differ by a rotation of the cut
    columns, X and the retraction's X are the same up to X_TOL; the cost is <C, X> + (sigma / 2) |A(X) - b|^2 with one constraint
    that reads an entry of absolute value <= 1 (sigma = 1, y = 0), so the values agree within X_TOL (sum |C_i| n_i + 1) -- ten
    times that is allowed for the retraction's own rounding."""
    from manisdp_matlab_amd import solvers
    rng = np.random.default_rng(84)
    cases = [R.Case(n, p, keep, nneg, 8, rng) for n, p, keep, nneg in ((20, 6, 3, 2), (9, 3, 1, 0), (31, 8, 8, 5), (14, 2, 2, 1))]
    nob = 2
    for c in cases[:nob]:                                            # points of the manifold: unit rows on the oblique blocks
        c.Y /= np.linalg.norm(c.Y, axis=1, keepdims=True)
    nset = [c.n for c in cases]
    h, mats = _handle(lib, nset, nob)
    out, Ynew, r0, Yold = _call(h, cases, PRIMAL, 1)
    for i, c in enumerate(cases):                                    # (the normalisation moved the spectra: the decisions must still be clear)
        e = np.linalg.svd(c.Y, compute_uv=False)
        assert R.decision_margin(e, PRIMAL["theta"]) >= 10.0
    _check(h, cases, nob, PRIMAL, 1, out, Ynew, r0, Yold, "mode 1")
    U = out[3]
    v_dev = [h.linesearch_cost(U, a) for a in (0.7, 0.1)]
    o = dict(solvers.DEFAULTS["multiblock"], line_search=1)
    geo = solvers._Blocks(None, o, nset, nob, strict_rank=False)
    Yh, Uh, ph = geo.reshape([c.Y for c in cases], [c.p for c in cases], None, ([c.w for c in cases], [c.V for c in cases]))
    assert ph == [int(v) for v in out[0]]
    h.set_point(solvers._pack_blocks(Yh, r0, int(r0[-1]), max(ph)))
    v_host = [h.linesearch_cost(solvers._pack_blocks(Uh, r0, int(r0[-1]), max(ph)), a) for a in (0.7, 0.1)]
    bound = 10 * R.X_TOL * (sum(np.linalg.norm(M) * M.shape[0] for M in mats) + 1)         # |X_i|_F <= n_i: unit diagonal, or singular values <= 1
    for a, b in zip(v_dev, v_host):
        print(f"\nline-search cost: device pair {a!r}, host pair {b!r}, bound {bound:.1e}")
        assert abs(a - b) <= bound
    h.close()


def test_three_hundred_blocks_reproducible_and_independent(lib, monkeypatch):
    """300 blocks of orders 1 .. 64 in one call (per-block storage): correct, the same bits on a second run, and a block's bits equal
    what a handle holding only that block gives."""
    monkeypatch.setenv("MSDP_MULTIBLOCK_BLOCKED", "1")
    rng = np.random.default_rng(81)
    R.seven_blocks(rng); R.branch_blocks(rng)
    cases = R.many_blocks(rng)
    nob = 150
    h, _ = _handle(lib, [c.n for c in cases], nob)
    out, Ynew, r0, Yold = _call(h, cases, PRIMAL, 0)
    _check(h, cases, nob, PRIMAL, 0, out, Ynew, r0, Yold, "300 blocks")
    out2, Ynew2, _, _ = _call(h, cases, PRIMAL, 0)
    assert np.array_equal(Ynew, Ynew2) and all(np.array_equal(a, b) for a, b in zip(out[:3], out2[:3]))
    h.close()
    cut = [i for i, c in enumerate(cases) if c.p > 1 and int(out[1][i]) < c.p]
    for i in (cut[0], cut[len(cut) // 2], 2, 3, 299):                # cut blocks, orders 63 and 64, the last one
        c = cases[i]
        ha, _ = _handle(lib, [c.n], 1 if i < nob else 0)
        oa, Ya, _, _ = _call(ha, [c], PRIMAL, 0)
        assert int(oa[0][0]) == int(out[0][i])
        assert np.array_equal(Ya, Ynew[int(r0[i]):int(r0[i + 1]), :ha.p]), i
        ha.close()


def test_refusals_leave_the_point_and_the_handle_as_they_were(lib, storage):
    rng = np.random.default_rng(85)
    cases = [R.Case(40, 30, 30, 8, 8, rng), R.Case(12, 4, 2, 1, 8, rng), R.Case(25, 7, 3, 0, 8, rng)]
    nset, r0, p, Y, w, V = _layout(cases)
    h, _ = _handle(lib, nset, 1, pcap=32)
    args = lambda **kw: {**dict(row0=r0[:-1], nblk=nset, p=p, w=w, V=V, theta=1e-2, strict=0, delta=8, alpha=0.1, min_facsize=2, mode=0), **kw}
    with pytest.raises(lib.MsdpError, match=r"error -4: block_reshape: no resident point"):      # MSDP_ESTATE
        h.block_reshape(**args())
    h.set_point(Y)
    ok = [R.Case(40, 20, 5, 2, 8, rng)] + cases[1:]
    bad = [
        (args(), r"error -6: block_reshape: new width 38 exceeds the allocated width 32"),        # MSDP_EUNSUPPORTED: growth
        (args(row0=r0[:2], nblk=nset[:2], p=p[:2], w=w[:r0[2]], V=V[:r0[2]]), r"error -1: block_reshape: 2 blocks given, the handle has 3"),
        (args(row0=[0, 40, 53], nblk=[40, 13, 24], w=w, V=V), r"error -1: block_reshape: block 1 is not block 1 of the handle"),
        (args(delta=9), r"error -1: block_reshape: bad argument"),                                 # delta > k
        (args(mode=2), r"error -1: block_reshape: bad argument"),
        (args(p=[30, 31, 7]), r"error -1: block_reshape: width 31 of block 1 outside 1..p = 30"),
    ]
    for kw, msg in bad:
        h.set_point(Y)
        with pytest.raises(lib.MsdpError, match=msg):
            h.block_reshape(**kw)
        assert h.p == 30 and np.array_equal(h.get_point(), Y), msg
        out, Ynew, r0k, Yold = _call(h, ok, PRIMAL, 0)
        _check(h, ok, 1, PRIMAL, 0, out, Ynew, r0k, Yold, "valid call after " + msg)
    h.close()
    # a width above the call's limit (64), on a handle that has room for it
    wide = [R.Case(80, 65, 3, 1, 8, rng), R.Case(5, 2, 1, 1, 8, rng)]
    nset, r0, p, Y, w, V = _layout(wide)
    h, _ = _handle(lib, nset, 0, pcap=80)
    h.set_point(Y)
    with pytest.raises(lib.MsdpError, match=r"error -6: block_reshape: block widths up to 64 \(block 0 has 65\)"):
        h.block_reshape(r0[:-1], nset, p, w, V, 1e-2, 0, 8, 0.1, 2, 0)
    assert h.p == 65 and np.array_equal(h.get_point(), Y)
    narrow = [R.Case(80, 64, 3, 1, 8, rng), wide[1]]
    out, Ynew, r0k, Yold = _call(h, narrow, PRIMAL, 0)
    _check(h, narrow, 0, PRIMAL, 0, out, Ynew, r0k, Yold, "width 64 after the refusal")
    h.close()


# ---------------------------------------------------------------------------------------------------------------- solves
def _solve_both(lib, monkeypatch, run):
    """run(block_reshape) -> (obj, data) under "host" and "device"; the uploads of the factor are counted."""
    res = {}
    real = lib.Handle.set_point
    for mode in ("host", "device"):
        calls = []
        monkeypatch.setattr(lib.Handle, "set_point", lambda self, Y, _c=calls: (_c.append(1), real(self, Y))[1])
        obj, d = run(mode)
        assert d["status"] == 0, mode
        res[mode] = (obj, d, len(calls))
    monkeypatch.setattr(lib.Handle, "set_point", real)
    (fh, dh, nh), (fd, dd, nd) = res["host"], res["device"]
    print(f"\nhost: {fh:.10f} in {dh['iters']} iterations, {nh} uploads; device: {fd:.10f} in {dd['iters']} iterations, {nd} uploads")
    assert abs(fd - fh) <= 1e-6 * abs(fh)
    assert nd == 1 and nh == dh["iters"]
    assert all(Yi.shape == (n, pi) for Yi, n, pi in zip(dd["Y"], [Y.shape[0] for Y in dh["Y"]], dd["p"]))


def test_solve_direct_sum_of_two_sdplib_blocks(lib, monkeypatch):
    from manisdp_matlab_amd import solvers
    from test_gpu_multiblock import _direct_sum
    At, b, c, K = _direct_sum(2)
    _solve_both(lib, monkeypatch, lambda m: solvers.ManiSDP_multiblock(At, b, c, K, {"block_reshape": m}, verbose=False)[1:])


def test_solve_twenty_blocks(lib, monkeypatch):
    from manisdp_matlab_amd import problems as P, solvers
    cl, n = P.chain_cliques(20, 5)
    coe = np.random.default_rng(2).standard_normal(len(P.bqp_sparse_monomials(cl)))
    At, b, c, K = P.bqpmom_sparse(n, cl, coe)
    assert len(K["s"]) == 20
    opts = {"tol": 1e-8, "line_search": 1, "tau1": 1}
    _solve_both(lib, monkeypatch, lambda m: solvers.ManiSDP_multiblock(At, b, c, K, dict(opts, block_reshape=m), verbose=False)[1:])


def test_solve_dual_chain_bqp(lib, monkeypatch):
    import test_gpu_dual_multiblock as D

    def run(m):
        f, data, _, K = D._bqp_dual(4, 8, {"block_reshape": m})
        assert len(K["s"]) == 4
        return f, data
    _solve_both(lib, monkeypatch, run)


def test_solve_falls_back_to_the_host_for_wide_blocks(lib, monkeypatch):
    """p0 = 66 on two blocks of order 80: the first reshape is refused (width above 64, MSDP_EUNSUPPORTED), that iteration runs the
    host loop -- which cuts the rank -- and re-enters through set_point; the later iterations run on the device again.  Same optimum
    as "host", and the uploads are the first one and one per refused iteration."""
    from manisdp_matlab_amd import solvers
    from test_gpu_multiblock import _stacked_maxcut
    nblk, n = 2, 80
    C0, scale, At, b, c = _stacked_maxcut(nblk, n, seed=4)
    K = dict(s=[n] * nblk, nob=nblk)
    refused = []
    real = lib.Handle.block_reshape

    def counting(self, *a, **k):
        try:
            return real(self, *a, **k)
        except lib.MsdpError as e:
            refused.append(e.code)
            raise
    monkeypatch.setattr(lib.Handle, "block_reshape", counting)
    res = {}
    real_set = lib.Handle.set_point
    for mode in ("host", "device"):
        calls = []
        monkeypatch.setattr(lib.Handle, "set_point", lambda self, Y, _c=calls: (_c.append(Y.shape[1]), real_set(self, Y))[1])
        _, obj, d = solvers.ManiSDP_multiblock(At, b, c, K, dict(tol=1e-8, p0=[66] * nblk, block_reshape=mode), verbose=False)
        assert d["status"] == 0, mode
        res[mode] = (obj, d, list(calls))
    (fh, dh, ch), (fd, dd, cd) = res["host"], res["device"]
    print(f"\nhost {fh:.10f} in {dh['iters']} iterations; device {fd:.10f} in {dd['iters']} iterations, uploads of widths {cd}, refusals {refused}")
    assert abs(fd - fh) <= 1e-6 * abs(fh)
    assert refused and set(refused) == {lib.EUNSUPPORTED}
    assert len(cd) == 1 + len(refused) < dd["iters"] and cd[0] == 66
