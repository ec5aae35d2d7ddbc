"""The block kinds' factor on the device between two trustregions() calls, and their rounding (msdp_blockfactor.hip:
Handle.blockfactor_gram / blockfactor_rotate / blockfactor_append / round_blocks, options["block_factor"] and
options["round_blocks"] of ManiSDP_onlyunitblockdiag and ManiSDP_posegraph) against the restatement of
tests/block_factor_ref.py: every dispatched <LPR, NCH> instance of both kinds and both d, near-degenerate and degenerate blocks,
the refusals, no stale state across width changes, whole solves of the two settings, and the rounding."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import block_factor_ref as F
import blockdiag_ref as BD
import posegraph_ref as BP

pytestmark = pytest.mark.gpu

# one width per dispatched <LPR, NCH> instance and the odd widths beside them (ld = 2 .. 256); d and d + 1 are added per shape
WIDTHS = (5, 8, 9, 16, 17, 32, 33, 64, 100, 130, 256)
# kind -> (n, d) -> degree of the instance
SHAPES = {"stiefel": {(101, 2): 6, (67, 3): 6, (343, 3): 6}, "pose": {(41, 2): 4, (67, 3): 6, (343, 3): 6}}
CASES = [(kind, n, d) for kind in SHAPES for (n, d) in SHAPES[kind]]


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _ref(kind):
    return BP if kind == "pose" else BD


def _efree(kind):
    return 1 if kind == "pose" else 0


def _cost_matrix(kind, n, d):
    deg = SHAPES[kind].get((n, d), 6)
    return BP.instance(n, d, deg, 0.3)[0] if kind == "pose" else BD.instance(n, d, deg, 1.0)[0]


def _handle(lib, kind, n, d, pcap=256):
    C = _cost_matrix(kind, n, d)
    return (lib.Handle.posegraph if kind == "pose" else lib.Handle.onlyunitblockdiag)(C, d, pcap=pcap), C


def _widths(d):
    return sorted({d, d + 1} | {p for p in WIDTHS if p >= d})


def _orth(Y, d, efree):
    R = F.blocks(Y, d, efree)[:, :d]
    return float(np.max(np.abs(F.block_gram(R) - np.eye(d))))


def _check_reshaped(kind, d, Yd, plain, tag, worst):
    """The device's point Yd against the plain product / concatenation `plain` re-orthonormalised by the restatement."""
    ef = _efree(kind)
    assert Yd.shape == plain.shape, tag
    P3, D3 = F.blocks(plain, d, ef), F.blocks(Yd, d, ef)
    kappa = F.cond(F.block_gram(P3[:, :d]))
    assert _orth(Yd, d, ef) <= 1e-12, tag
    ratio = float(np.max(np.max(np.abs(D3[:, :d] - F.polar_svd(P3[:, :d])), axis=(1, 2)) / (F.EPS * kappa)))
    worst[0] = max(worst[0], ratio)
    assert ratio <= 64.0, (tag, ratio, float(kappa.max()))
    if ef:
        assert np.max(np.abs(D3[:, d] - P3[:, d])) <= 1e-14 * max(np.max(np.abs(P3[:, d])), 1e-300), tag


# ------------------------------------------------------------------ Gram matrix, rotate, append over every instance
@pytest.mark.parametrize("kind,n,d", CASES)
def test_gram_rotate_append_against_restatement(lib, kind, n, d):
    B, ef = _ref(kind), _efree(kind)
    h, C = _handle(lib, kind, n, d)
    g = np.random.default_rng(11 + n + d)
    worst = [0.0]
    try:
        for p in _widths(d):
            Y = B.point(n, d, p)
            h.set_point(Y)
            G, Gr = h.blockfactor_gram(), F.gram(Y)
            assert np.max(np.abs(G - Gr)) <= 1e-12 * np.max(np.abs(Gr)), p
            for r in sorted({r for r in (d, (p + 1) // 2, p - 1) if d <= r <= p}):
                Q = np.linalg.qr(g.standard_normal((p, p)))[0][:, :r]
                h.set_point(Y)
                assert h.blockfactor_rotate(Q) == 0, (p, r)
                assert h.p == r
                Yd = h.get_point()
                _check_reshaped(kind, d, Yd, Y @ Q, ("rotate", p, r), worst)
                if r % 2:                                  # the pad column of the new point is zero: the device's cost is that of Yd
                    cr = B.cost(C, Yd, d)
                    assert abs(h.cost() - cr) <= 1e-12 * abs(cr), (p, r)
            for k in (1, d, 2 * d):
                if p + k > 256:
                    continue
                V = g.standard_normal((Y.shape[0], k))
                h.set_point(Y)
                assert h.blockfactor_append(V, 0.5) == 0, (p, k)
                assert h.p == p + k
                Yd = h.get_point()
                _check_reshaped(kind, d, Yd, np.hstack([Y, 0.5 * V]), ("append", p, k), worst)
                if (p + k) % 2:
                    cr = B.cost(C, Yd, d)
                    assert abs(h.cost() - cr) <= 1e-12 * abs(cr), (p, k)
    finally:
        h.close()
    print("%s n %d d %d: max |P - P_svd| / (eps cond(G_i)) = %.2f" % (kind, n, d, worst[0]))


# ------------------------------------------------------------------ near-degenerate and degenerate blocks
@pytest.mark.parametrize("kind,n,d", [("stiefel", 101, 2), ("stiefel", 67, 3), ("pose", 41, 2), ("pose", 67, 3)])
def test_near_degenerate_block_is_re_orthonormalised(lib, kind, n, d):
    B, ef = _ref(kind), _efree(kind)
    p = 8
    Y = np.array(B.point(n, d, p))
    Y[3 * (d + ef) + 1] *= 1e-4                            # rows of block 3 scaled by diag(1, 1e-4[, 1]): cond(G) = 1e8
    V = np.random.default_rng(2).standard_normal((Y.shape[0], 1))
    h, _ = _handle(lib, kind, n, d, pcap=32)
    try:
        h.set_point(Y)                                     # (set_point does not check orthonormality)
        assert h.blockfactor_append(V, 1e-9) == 0
        Yd = h.get_point()
        worst = [0.0]
        _check_reshaped(kind, d, Yd, np.hstack([Y, 1e-9 * V]), "near-degenerate", worst)
        print("%s d %d: orthonormality %.2e, ratio %.2f at cond 1e8" % (kind, d, _orth(Yd, d, ef), worst[0]))
    finally:
        h.close()


@pytest.mark.parametrize("kind,n,d", [("stiefel", 101, 2), ("stiefel", 67, 3), ("pose", 41, 2), ("pose", 67, 3)])
def test_degenerate_block_is_counted_and_nothing_changes(lib, kind, n, d):
    B, ef = _ref(kind), _efree(kind)
    p, r = d + 3, d
    Y = np.array(B.point(n, d, p))
    Y[:d] = np.eye(d, p)                                   # block 0 = the first d unit vectors
    Q = np.eye(p)[:, 1:r + 1]                              # e_2 .. e_{r+1}: row 1 of Y_0 Q is exactly zero
    assert not np.any((Y @ Q)[0])
    h, _ = _handle(lib, kind, n, d, pcap=32)
    try:
        h.set_point(Y)
        f0 = h.cost()
        ndeg = h.blockfactor_rotate(Q)
        assert ndeg >= 1
        assert h.p == p and h.get_point().shape == Y.shape
        assert np.array_equal(h.get_point(), Y)
        assert np.isfinite(h.cost()) and h.cost() == f0
        # the handle goes on: a rotation that keeps the block's rows is taken
        Q2 = np.eye(p)[:, :p - 1]
        assert h.blockfactor_rotate(Q2) == 0 and h.p == p - 1
        assert _orth(h.get_point(), d, ef) <= 1e-12
        # ... and a zero block in the widening counts too (zero rows stay zero under [Y, alpha V] with V_0 = 0)
        Z = np.array(B.point(n, d, p))
        Z[:d] = 0.0
        V = np.random.default_rng(3).standard_normal((Z.shape[0], 1))
        V[:d] = 0.0
        h.set_point(Z)
        assert h.blockfactor_append(V, 0.5) >= 1 and h.p == p
        assert np.array_equal(h.get_point(), Z)
    finally:
        h.close()


# ------------------------------------------------------------------ refusals
def test_refusals(lib):
    n, d, p = 67, 3, 6
    h, C = _handle(lib, "stiefel", n, d, pcap=8)
    hp, _ = _handle(lib, "pose", n, d, pcap=8)
    hs = lib.Handle.onlyunitdiag(sp.csr_matrix(C))
    raw = lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    try:
        for hh, N in ((h, n * d), (hp, n * (d + 1))):       # no resident point
            for call in (lambda: hh.blockfactor_gram(), lambda: hh.blockfactor_rotate(np.eye(p)[:, :d]),
                         lambda: hh.blockfactor_append(np.ones((N, 1)), 0.5), lambda: hh.round_blocks(np.eye(p)[:, :d])):
                with pytest.raises(lib.MsdpError) as e:
                    call()
                assert e.value.code == lib.ESTATE
        Y, Yp = BD.point(n, d, p), BP.point(n, d, p)
        h.set_point(Y)
        hp.set_point(Yp)
        for hh, Y0 in ((h, Y), (hp, Yp)):
            for r in (d - 1, p + 1):
                with pytest.raises(lib.MsdpError, match="blockfactor_rotate") as e:
                    hh.p = p + 1 if r > p else p           # (the wrapper checks Q against its own width: reach the library)
                    hh.blockfactor_rotate(np.ones((hh.p, r)))
                assert e.value.code == lib.EINVAL
                hh.p = p
            with pytest.raises(lib.MsdpError, match="allocated capacity") as e:
                hh.blockfactor_append(np.ones((Y0.shape[0], 3)), 0.5)
            assert e.value.code == lib.EUNSUPPORTED
            assert hh.p == p and np.array_equal(hh.get_point(), Y0)
        # rounding with / without t on the wrong kind
        W = np.ascontiguousarray(np.eye(p)[:, :d])
        R, t = np.zeros((n, d, d)), np.zeros((n, d))
        fl, nd = ctypes.c_int32(), ctypes.c_int32()
        assert raw.msdp_blockfactor_round(h._h, W.ctypes.data_as(dp), R.ctypes.data_as(dp), t.ctypes.data_as(dp),
                                          ctypes.byref(fl), ctypes.byref(nd)) == lib.EINVAL
        assert raw.msdp_blockfactor_round(hp._h, W.ctypes.data_as(dp), R.ctypes.data_as(dp), None,
                                          ctypes.byref(fl), ctypes.byref(nd)) == lib.EINVAL
        # the oblique kind: the four calls name themselves
        hs.set_point(BD.point(n, d, 4))
        for name, call in (("blockfactor_gram", lambda: hs.blockfactor_gram()), ("blockfactor_rotate", lambda: hs.blockfactor_rotate(np.eye(4)[:, :3])),
                           ("blockfactor_append", lambda: hs.blockfactor_append(np.ones((n * d, 1)), 0.5)),
                           ("blockfactor_round", lambda: hs.round_blocks(np.eye(4)[:, :1]))):
            with pytest.raises(lib.MsdpError, match=name) as e:
                call()
            assert e.value.code == lib.EUNSUPPORTED
        assert np.isfinite(hs.cost())
    finally:
        h.close(); hp.close(); hs.close()


# ------------------------------------------------------------------ no stale state across a width change
def _reshape_on_device(h, Y0, p_to, g):
    p = Y0.shape[1]
    h.set_point(Y0)
    if p_to < p:
        assert h.blockfactor_rotate(np.linalg.qr(g.standard_normal((p, p)))[0][:, :p_to]) == 0
    else:
        assert h.blockfactor_append(g.standard_normal((Y0.shape[0], p_to - p)), 0.5) == 0
    assert h.p == p_to


@pytest.mark.parametrize("kind,option", [("stiefel", None), ("stiefel", "block_persist"), ("pose", None), ("pose", "block_persist"),
                                         ("pose", "precon")])
def test_no_stale_state_after_a_width_change(lib, kind, option):
    B = _ref(kind)
    c = B.COUNT_CASE
    n, d = c["n"], c["d"]
    C = B.count_case()[0]
    make = lib.Handle.posegraph if kind == "pose" else lib.Handle.onlyunitblockdiag
    opts = lib.default_opts(maxiter=c["maxiter"], maxinner=c["maxinner"], tolgradnorm=c["tolgradnorm"])
    g = np.random.default_rng(21)
    for p_from, p_to in ((9, 8), (17, 16), (16, 17)):      # across ld, LPR and the persistent plan's slot count
        ha, hb = make(C, d, pcap=32), make(C, d, pcap=32)
        try:
            for hh in (ha, hb):
                if option:
                    hh.set_option(option, 1)
            # A has run at the old width first: chunk graphs, plan and vectors of that width exist when the width changes
            ha.set_point(B.point(n, d, p_from))
            ha.rtr(lib.default_opts(maxiter=2, maxinner=c["maxinner"], tolgradnorm=c["tolgradnorm"]))
            _reshape_on_device(ha, B.point(n, d, p_from), p_to, g)
            if option == "block_persist" and ha.block_persist_plan()["eligible"]:
                assert ha.tcg_path() == 1, (p_from, p_to)
            hb.set_point(ha.get_point())
            sa, sb = ha.rtr(opts), hb.rtr(opts)
            ca = (sa.iters, sa.hessvecs, sa.accepted, sa.rejected, sa.last_stop_inner)
            cb = (sb.iters, sb.hessvecs, sb.accepted, sb.rejected, sb.last_stop_inner)
            print("%s %s %d -> %d: %s cost %.12f" % (kind, option, p_from, p_to, ca, sa.cost))
            assert ca == cb, (p_from, p_to)
            assert sa.cost == sb.cost, (p_from, p_to)
            assert np.array_equal(ha.get_point(), hb.get_point())
            if option == "block_persist" and ha.block_persist_plan()["eligible"]:
                assert ha.tcg_path() == 1 and hb.tcg_path() == 1
        finally:
            ha.close(); hb.close()


# ------------------------------------------------------------------ whole solves, host against device
STIEFEL_OPTIMA = {(67, 3, 2.0): -794.4145229643, (101, 2, 1.5): -852.1849789459}      # the restatement's (blockdiag_ref.solve from p0 = d)


def _check_device_solve(data_h, data_d, d, efree, Yd, fires=True):
    for data in (data_h, data_d):
        assert data["status"] == 0
        assert data["factor_seconds"] > 0.0
        if fires:
            assert data["iters"] >= 2
    assert data_h["factor_device_calls"] == 0 and data_h["factor_host_fallbacks"] == 0
    assert data_d["factor_host_fallbacks"] == 0
    if fires or data_d["iters"] - data_d.get("reruns", 0) >= 2:
        assert data_d["factor_device_calls"] >= 1
    else:
        assert data_d["factor_device_calls"] == 0
    assert _orth(Yd, d, efree) <= 1e-12


@pytest.mark.parametrize("n,d,sigma", [(67, 3, 2.0), (101, 2, 1.5)])
@pytest.mark.parametrize("eig", ["host", "device"])
def test_stiefel_solves_host_against_device(lib, n, d, sigma, eig):
    from manisdp_matlab_amd import solvers
    C = BD.instance(n, d, 6, sigma)[0]
    Y0 = BD.random_point(n, d, d, np.random.default_rng(1))
    ref = STIEFEL_OPTIMA[(n, d, sigma)]
    out = {}
    for mode in ("host", "device"):
        out[mode] = solvers.ManiSDP_onlyunitblockdiag(C, d, {"Y0": Y0, "eig": eig, "block_factor": mode}, verbose=False)
    (Yh, obj_h, data_h), (Yd, obj_d, data_d) = out["host"], out["device"]
    print("n %d d %d sigma %g (%s): host %.10f in %d iterations, device %.10f in %d (%d device calls), restatement %.10f; factor seconds %.2e / %.2e"
          % (n, d, sigma, eig, obj_h, data_h["iters"], obj_d, data_d["iters"], data_d["factor_device_calls"], ref,
             data_h["factor_seconds"], data_d["factor_seconds"]))
    assert abs(obj_h - ref) <= 1e-6 and abs(obj_d - ref) <= 1e-6
    assert data_d["dinf"] < 1e-8
    _check_device_solve(data_h, data_d, d, 0, Yd)
    assert data_d["Lambda"].shape == (n, d, d) and abs(np.sum(data_d["z"]) - obj_d) <= 1e-12 * abs(obj_d)
    assert abs(float(np.sum(C.multiply(data_d["X"]))) - obj_d) <= 1e-9 * abs(obj_d)


_POSE_REF = {}


def _pose_reference(n, d, degree, sigma):
    """The restatement's optimum: reference_solve at noise 0.3; its solve from p0 = d at noise 1.0, once per instance."""
    if sigma == 0.3:
        return BP.reference_solve(n, d, degree, 0.3)
    key = (n, d, degree, sigma)
    if key not in _POSE_REF:
        _POSE_REF[key] = BP.solve(BP.instance(n, d, degree, sigma)[0], d, BP.start_point(n, d, d, np.random.default_rng(0)))
    return _POSE_REF[key]


# noise 0.3: the reference_solve cases.  On them the restatement is optimal after ONE outer iteration also from p0 = d (10.9695109010
# and 76.1126274793): nothing is re-shaped unless the device's loop takes a second pass.  Noise 1.0 from p0 = d is where the
# staircase fires (the restatement widens once for n = 41 and twice for n = 67): iters >= 2 and the device calls are asserted there.
@pytest.mark.parametrize("n,d,degree,sigma", [(41, 2, 4, 0.3), (67, 3, 6, 0.3), (41, 2, 4, 1.0), (67, 3, 6, 1.0)])
@pytest.mark.parametrize("eig", ["host", "device"])
def test_pose_solves_host_against_device(lib, n, d, degree, sigma, eig):
    from manisdp_matlab_amd import solvers
    C = BP.instance(n, d, degree, sigma)[0]
    _, obj_r, data_r = _pose_reference(n, d, degree, sigma)
    assert data_r["status"] == 0
    out = {}
    for mode in ("host", "device"):
        out[mode] = solvers.ManiSDP_posegraph(C, d, {"p0": d, "eig": eig, "block_factor": mode}, verbose=False)
    (Yh, obj_h, data_h), (Yd, obj_d, data_d) = out["host"], out["device"]
    print("n %d d %d (%s): host %.10f in %d iterations, device %.10f in %d (%d device calls, %d reruns), restatement %.10f"
          % (n, d, eig, obj_h, data_h["iters"], obj_d, data_d["iters"], data_d["factor_device_calls"], data_d["reruns"], obj_r))
    assert abs(obj_h - obj_r) <= 1e-6 * abs(obj_r) and abs(obj_d - obj_r) <= 1e-6 * abs(obj_r)
    assert data_d["dinf"] < 1e-8 and data_d["gap"] < 1e-8
    _check_device_solve(data_h, data_d, d, 1, Yd, fires=sigma == 1.0)
    assert abs(float(np.sum(C.multiply(data_d["X"]))) - obj_d) <= 1e-9 * abs(obj_d)


# ------------------------------------------------------------------ rounding
def _check_rounding(lib, h, Y, d, efree, tag):
    W = F.top_eigenvectors(Y, d)
    Rr, tr, fr, nr = F.round_blocks(Y, d, efree, W)
    assert nr == 0
    A = F.blocks(Y, d, efree)
    Z = A[:, :d] @ W
    kappa = F.cond(F.block_gram(Z))
    h.set_point(Y)
    R, t, fl, nd = h.round_blocks(W)
    assert nd == 0 and fl == fr, tag
    ratio = float(np.max(np.max(np.abs(R - Rr), axis=(1, 2)) / (F.EPS * kappa)))
    print("%s: max |R - R_ref| / (eps cond) = %.2f, max cond %.1e, flipped %d" % (tag, ratio, kappa.max(), fl))
    assert ratio <= 64.0, tag
    assert np.max(np.abs(np.linalg.det(R) - 1.0)) <= 1e-12 and np.max(np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(d))) <= 1e-12
    if efree:
        assert np.max(np.abs(t - tr)) <= 1e-13 * np.max(np.abs(tr)), tag
    else:
        assert t is None
    # the mirrored frame: the same rotations with the last column negated
    W2 = W.copy()
    W2[:, -1] *= -1.0
    R2, t2, fl2, nd2 = h.round_blocks(W2)
    assert nd2 == 0 and fl2 == 1 - fl, tag
    # (W2 negates the last column of every Z_i, so every determinant and with them the majority change sign: the call that
    # reports flipped = 1 has negated the last column of the other call's Z_i W -- both round the same matrices)
    assert np.max(np.abs(R2 - R)) <= 1e-12, tag
    if efree:
        assert np.max(np.abs(t2 - t)) <= 1e-13 * np.max(np.abs(t)), tag
    return W, R


@pytest.mark.parametrize("kind,n,d", [("stiefel", 101, 2), ("stiefel", 67, 3), ("pose", 41, 2), ("pose", 67, 3)])
def test_round_blocks_against_restatement(lib, kind, n, d):
    from manisdp_matlab_amd import solvers
    B, ef = _ref(kind), _efree(kind)
    h, C = _handle(lib, kind, n, d, pcap=32)
    try:
        # a solved point (the noisy instance of the shape) and a random manifold point
        solve = solvers.ManiSDP_posegraph if ef else solvers.ManiSDP_onlyunitblockdiag
        Ys = solve(C, d, {}, verbose=False)[0]
        _check_rounding(lib, h, Ys, d, ef, "%s n %d d %d solved" % (kind, n, d))
        Y = np.array(B.point(n, d, 8))
        W, R = _check_rounding(lib, h, Y, d, ef, "%s n %d d %d random" % (kind, n, d))
        # W = None: the device's own top-d eigenvectors span the same subspace
        h.set_point(Y)
        Rn = h.round_blocks()[0]
        assert np.max(np.abs(np.linalg.det(Rn) - 1.0)) <= 1e-12
        # a minority reflection.  The determinants of Y_i W of a random point have either sign: first every block is given a
        # positive one (two rows of a block exchanged: still a point of the manifold, Y'Y and W unchanged), then rows 0 and 1
        # of block 0 are exchanged
        Yo = F.oriented(Y, d, ef, W)
        h.set_point(Yo)
        Ro, _, fo, ndo = h.round_blocks(W)
        assert fo == 0 and ndo == 0
        Ym = Yo.copy()
        Ym[[0, 1]] = Ym[[1, 0]]
        Rr, _, fr, _ = F.round_blocks(Ym, d, ef, W)
        h.set_point(Ym)
        Rm, _, fm, ndm = h.round_blocks(W)
        assert ndm == 0 and fm == fr == 0
        Z0 = F.blocks(Ym, d, ef)[:1, :d] @ W
        assert np.linalg.det(Z0[0]) < 0                    # block 0 alone is in the minority
        k0 = F.cond(F.block_gram(Z0))[0]
        assert abs(np.linalg.det(Rm[0]) - 1.0) <= 1e-12
        assert np.max(np.abs(Rm[0] - F.nearest_rotation_svd(Z0)[0])) <= 64 * F.EPS * k0
        assert np.max(np.abs(Rm[0] - Rr[0])) <= 64 * F.EPS * k0
        assert np.array_equal(Rm[1:], Ro[1:])
    finally:
        h.close()


def test_round_blocks_option_recovers_the_planted_poses(lib):
    from manisdp_matlab_amd import problems, solvers
    for mode in ("host", "device"):
        C, Rt, _ = BD.instance(67, 3, 6, 0.0)
        _, _, data = solvers.ManiSDP_onlyunitblockdiag(C, 3, {"round_blocks": True, "block_factor": mode}, verbose=False)
        assert data["status"] == 0 and data["round_fallback"] is False and "t" not in data
        assert problems.rotation_error(data["R"], Rt) <= 1e-6
        C, Rt, tt = BP.instance(41, 2, 4, 0.0)[:3]
        _, _, data = solvers.ManiSDP_posegraph(C, 2, {"round_blocks": True, "block_factor": mode}, verbose=False)
        assert data["status"] == 0 and data["round_fallback"] is False
        assert max(problems.pose_error(data["R"], data["t"], Rt, tt)) <= 1e-6
    # the default leaves data as it was
    _, _, data = solvers.ManiSDP_posegraph(C, 2, verbose=False)
    assert "R" not in data and "t" not in data and "round_fallback" not in data
