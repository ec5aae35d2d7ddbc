"""The pose-graph handle (msdp_create_posegraph_csc, Handle.posegraph, msdp_stiefel.hip) against the NumPy restatement of
tests/posegraph_ref.py: point operations over every dispatched <LPR, NCH> instance for d = 2 and 3, consistency with the
unit-block-diagonal handle when the free rows of C are zero, trustregions() counts, the escape's eigenpairs, whole solves
against the restatement (whose optima carry their own certificate), and the refused calls."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import posegraph_ref as B

pytestmark = pytest.mark.gpu

# (n, d, degree) -> noise of the instance the point operations run on (one of them noise-free)
SHAPES = {(41, 2, 4): 0.3, (67, 3, 6): 0.0, (343, 3, 6): 0.3}
# one width per dispatched <LPR, NCH> instance (ld = 2 .. 256), odd widths for the padding column; d and d + 1 are added per shape
WIDTHS = (4, 7, 12, 24, 33, 64, 100, 130, 256)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _widths(d):
    return sorted({d, d + 1} | {p for p in WIDTHS if p >= d})


# ------------------------------------------------------------------ point operations
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_point_operations_against_restatement(lib, shape):
    n, d, degree = shape
    C = B.instance(n, d, degree, SHAPES[shape])[0]
    h = lib.Handle.posegraph(C, d, pcap=256)
    try:
        for p in _widths(d):
            Y = B.point(n, d, p)
            M = B.StiefelEuclid(n, d, p)
            g = np.random.default_rng(500 + p)
            U = B.tangent_direction(Y, d, g)
            Z = g.standard_normal(Y.shape)                                   # an ambient direction for proj
            h.set_point(Y)
            assert h.tcg_path() == 0 and h.persist_form() == -1              # the generic per-iteration path
            f, G, H, z, L = h.cost(), h.rgrad(), h.hessvec(U), h.get_z(), h.get_blockmult()
            L_ref = B.blockmult(C, Y, d)
            f_ref = B.cost(C, Y, d)
            errs = dict(cost=abs(f - f_ref) / max(1.0, abs(f_ref)), Lam=_relerr(L, L_ref), z=_relerr(z, B.get_z(C, Y, d)),
                        grad=_relerr(G, B.rgrad(C, Y, d)), hess=_relerr(H, B.hessvec(C, Y, U, d)),
                        proj=_relerr(h.proj(Z), M.proj(Y, Z)))
            for bn in (0.1, 10.0):                                           # tangent directions of block norm 0.1 and 10
                Ub = B.tangent_direction(Y, d, g, blocknorm=bn)
                Zr = h.retr(Ub)
                errs["retr%g" % bn] = _relerr(Zr, M.retr(Y, Ub))
                Z3 = B.rot(Zr, d)
                errs["orth%g" % bn] = float(np.max(np.abs(Z3 @ np.swapaxes(Z3, 1, 2) - np.eye(d))))
                assert np.array_equal(B.free(Zr, d), B.free(Y + Ub, d))      # the free row: tau + eta, one addition
            print("n %d d %d p %d: " % (n, d, p) + " ".join("%s %.1e" % kv for kv in errs.items()))
            assert all(v < 1e-12 for v in errs.values()), (p, errs)
            assert L.shape == (n, d, d) and np.array_equal(L, np.swapaxes(L, 1, 2))
            assert np.all(z.reshape(n, d + 1)[:, d] == 0.0)                  # no multiplier on the free rows
            dual = float(np.sum(z))
            assert abs(dual - B.dual_value(C, Y, d)) <= 1e-12 * max(1.0, abs(dual))
            assert abs(dual - 2.0 * f) > 1e-3 * abs(f)                       # sum z is the dual value, NOT <C, X>, at a generic point
            assert np.array_equal(H, h.hessvec(U)) and np.array_equal(G, h.rgrad()) and f == h.cost()   # fixed summation orders
            assert np.array_equal(h.get_point(), Y)
            ms, by, fl = h.bench_hessvec(50)                                 # the measurement entry point accepts the kind
            assert ms > 0 and by > 0 and fl > 0
            if p == 12:
                assert h.bench_tcg_trip(16) > 0                              # ... and so does the generic chunked trip
    finally:
        h.close()


@pytest.mark.parametrize("n,d,degree", B.INSTANCES)
def test_zero_free_rows_equal_the_stiefel_kind(lib, n, d, degree):
    """A pose handle whose free rows and columns of C are zero: on the rotation rows the results of the onlyunitblockdiag handle
    of the rotation submatrix, and zero free rows of gradient and Hess-vec."""
    C = sp.csr_matrix(B.instance(n, d, degree, 0.3)[0])
    keep = np.ones(n * (d + 1), dtype=bool)
    keep[d::d + 1] = False
    Cr = sp.csr_matrix(C[keep][:, keep])                                     # the rotation submatrix, order n d
    Dk = sp.diags(keep.astype(np.float64))
    Cz = sp.csr_matrix(Dk @ C @ Dk)                                          # the pose matrix with zero free rows and columns
    Cz.eliminate_zeros()
    p = d + 4
    Y = B.point(n, d, p)
    U = B.tangent_direction(Y, d, np.random.default_rng(8))
    Yr = np.ascontiguousarray(Y[keep])
    Ur = np.ascontiguousarray(U[keep])
    h = lib.Handle.posegraph(Cz, d, pcap=p)
    hs = lib.Handle.onlyunitblockdiag(Cr, d, pcap=p)
    try:
        h.set_point(Y)
        hs.set_point(Yr)
        G, H = h.rgrad(), h.hessvec(U)
        e = dict(cost=abs(h.cost() - hs.cost()) / max(1.0, abs(hs.cost())), grad=_relerr(G[keep], hs.rgrad()),
                 hess=_relerr(H[keep], hs.hessvec(Ur)), Lam=_relerr(h.get_blockmult(), hs.get_blockmult()),
                 z=_relerr(h.get_z()[keep], hs.get_z()), proj=_relerr(h.proj(U + Y)[keep], hs.proj(Ur + Yr)),
                 retr=_relerr(h.retr(U)[keep], hs.retr(Ur)))
        print("n %d d %d: " % (n, d) + " ".join("%s %.1e" % kv for kv in e.items()))
        assert max(e.values()) < 1e-13
        assert np.all(G[~keep] == 0.0) and np.all(H[~keep] == 0.0)
    finally:
        h.close(); hs.close()


# ------------------------------------------------------------------ trustregions()
def test_rtr_counts_match_the_restatement(lib):
    c = B.COUNT_CASE
    C, Y0 = B.count_case()
    _, f_ref, info = B.trustregions(C, Y0, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
    h = lib.Handle.posegraph(C, c["d"], pcap=c["p"])
    try:
        h.set_point(Y0)
        assert h.tcg_path() == 0 and h.persist_form() == -1
        st = h.rtr(lib.default_opts(maxiter=c["maxiter"], maxinner=c["maxinner"], tolgradnorm=c["tolgradnorm"]))
        dev = (st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner)
        print("rtr: device", dev, st.cost, "restatement", B.counts(info), f_ref)
        assert dev == B.counts(info)
        assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
        assert abs(h.cost() - st.cost) <= 1e-11 * abs(st.cost)
        Y3 = B.rot(h.get_point(), c["d"])
        assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(c["d"]))) < 1e-13
    finally:
        h.close()


# ------------------------------------------------------------------ escape
@pytest.mark.parametrize("n,d,degree,stationary", [(41, 2, 4, False), (67, 3, 6, False), (41, 2, 4, True), (67, 3, 6, True)])
def test_escape_eigs_against_lapack(lib, n, d, degree, stationary):
    """S with the zero-padded multiplier: at a generic point, and at a critical point of the width-d problem with strong noise,
    which is no optimum of the SDP (S Y = 0 and S has negative eigenvalues)."""
    C = B.instance(n, d, degree, 1.5)[0]
    k = d
    h = lib.Handle.posegraph(C, d)
    try:
        if stationary:
            h.set_point(B.start_point(n, d, d, np.random.default_rng(3)))
            st = h.rtr(lib.default_opts(maxiter=400, maxinner=200, tolgradnorm=1e-9))
            assert st.gradnorm <= 1e-6 * max(1.0, abs(st.cost))
        else:
            h.set_point(B.point(n, d, d + 2))
        Y = h.get_point()
        L = h.get_blockmult()
        lam, V, lmax, its = h.escape_eigs(k, tol=1e-10, maxit=4000)
        assert h.escape_method() == 0                                         # the Lanczos path
    finally:
        h.close()
    S = (C - B.blockdiag(L)).toarray()
    dS = np.linalg.eigh(S)[0]
    scale = max(abs(dS[0]), abs(dS[-1]))
    if stationary:
        assert np.linalg.norm(S @ Y) <= 1e-6 * scale
    print("escape n %d d %d %s: lam" % (n, d, "stationary" if stationary else "generic"), lam, "lapack", dS[:k],
          "lmax err %.2e (scale %.3f, %d steps)" % (abs(lmax - dS[-1]), scale, its))
    assert V.shape == (n * (d + 1), k)
    assert abs(lmax - dS[-1]) < 1e-5 * scale
    assert lam[0] < 0 and abs(lam[0] - dS[0]) < 1e-8
    assert np.all(np.diff(lam[np.isfinite(lam)]) >= 0)
    used = set()
    for t in range(k):
        if np.isfinite(lam[t]) and lam[t] < -1e-9 * scale:
            near = [int(j) for j in np.argsort(np.abs(dS - lam[t]))[:4] if int(j) not in used]
            j = near[0]                                                      # no eigenvalue of S is reported more often than S has it
            assert abs(dS[j] - lam[t]) < 1e-8, t
            used.add(j)
            v = V[:, t]
            assert abs(np.linalg.norm(v) - 1.0) < 1e-8
            assert np.linalg.norm(S @ v - lam[t] * v) <= 1e-7 * scale, t
    assert len(used) == k                                                    # S has at least k negative eigenvalues at these points
    assert np.max(np.abs(V.T @ V - np.eye(k))) < 1e-6
    # the returned values lie at the bottom of the spectrum: the t-th between the t-th eigenvalue and the t-th distinct one (a
    # Krylov space holds one direction of an eigenspace; at a critical point of the d = 2 problem with rotation data every
    # eigenvalue of S is double)
    distinct = [dS[0]]
    for x in dS[1:]:
        if x - distinct[-1] > 1e-7 * scale:
            distinct.append(x)
    for t in range(k):
        if np.isfinite(lam[t]) and lam[t] < -1e-9 * scale:
            assert dS[t] - 1e-8 <= lam[t] <= distinct[t] + 1e-8, (t, lam, dS[:k], distinct[:k])


# ------------------------------------------------------------------ solves
def test_noise_free_solve(lib):
    from manisdp_matlab_amd import problems, solvers
    n, d = 41, 2
    C, R, t = B.instance(n, d, 4, 0.0)[:3]
    Y, obj, data = solvers.ManiSDP_posegraph(C, d, verbose=False)
    print("noise-free: obj %.3e, dual %.3e, rank %d, p %d, dinf %.1e, gap %.1e" % (obj, data["dual"], data["rank"], data["p"], data["dinf"], data["gap"]))
    assert data["status"] == 0 and data["dinf"] < 1e-8 and data["gap"] < 1e-8
    assert abs(obj) <= 1e-7
    assert data["rank"] == d
    assert max(problems.pose_error(*problems.round_poses(Y, d), R, t)) <= 1e-6


@pytest.mark.parametrize("n,d,degree", [(41, 2, 4), (67, 3, 6)])
def test_noisy_solves_equal_the_restatement(lib, n, d, degree):
    from manisdp_matlab_amd import solvers
    C = B.instance(n, d, degree, 0.3)[0]
    _, obj_r, data_r = B.reference_solve(n, d, degree, 0.3)
    assert data_r["status"] == 0 and max(data_r["dinf"], data_r["gap"]) < 1e-8
    Y, obj, data = solvers.ManiSDP_posegraph(C, d, verbose=False)
    print("n %d d %d: %.10f, restatement %.10f (%d iterations, p %d); device %d iterations, p %d, dinf %.1e, gap %.1e"
          % (n, d, obj, obj_r, data_r["iters"], data_r["p"], data["iters"], data["p"], data["dinf"], data["gap"]))
    assert data["status"] == 0 and data["dinf"] < 1e-8 and data["gap"] < 1e-8
    assert abs(obj - obj_r) <= 1e-6 * abs(obj_r)
    Y3 = B.rot(Y, d)
    assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(d))) < 1e-12     # (X_[ii])_{1..d,1..d} = I_d
    assert abs(float(np.sum(C.multiply(data["X"]))) - obj) <= 1e-9 * abs(obj)          # <C, X> = obj
    assert abs(np.sum(data["z"]) - data["dual"]) <= 1e-12 * abs(obj)


def test_larger_solve_with_the_device_escape(lib):
    from manisdp_matlab_amd import solvers
    n, d = 343, 3
    C = B.instance(n, d, 6, 0.5)[0]
    _, obj_r, data_r = B.reference_solve(n, d, 6, 0.5)
    assert data_r["status"] == 0
    Y, obj, data = solvers.ManiSDP_posegraph(C, d, verbose=False)            # N = 1372 > dense_eig_default: the device escape
    print("n %d d %d: %.10f, restatement %.10f; %d iterations, p %d, dinf %.1e, gap %.1e, %d cold checks" % (
        n, d, obj, obj_r, data["iters"], data["p"], data["dinf"], data["gap"], data.get("eig_verifications", 0)))
    assert data["status"] == 0 and data["dinf"] < 1e-8 and data["gap"] < 1e-8
    assert data["eig_verifications"] >= 1 and data["escape_method"] == 0     # certified by the independent cold check (Lanczos)
    assert abs(obj - obj_r) <= 1e-6 * abs(obj_r)


def test_ring_does_not_report_optimality_after_the_first_iteration(lib, capsys):
    from manisdp_matlab_amd import solvers
    n, d = 101, 2
    C = B.instance(n, d, 2, 0.2)[0]
    Y, obj, data = solvers.ManiSDP_posegraph(C, d, {"AL_maxiter": 2}, verbose=True)
    out = capsys.readouterr().out
    print(out)
    it1 = data["log"][0]
    assert it1[2] < 1e-8 and it1[3] > 1e-3                                   # S PSD after the first call, the gap wide open
    assert data["iters"] == 2                                                # ... and the loop went on
    assert "Optimality is reached!" not in out.split("Iter 2")[0]
    assert data["reruns"] >= 1 and data["log"][1][5] == it1[5]               # trustregions() again on the same factor, same width
    assert data["log"][1][1] < it1[1]                                        # and the cost fell


# ------------------------------------------------------------------ refusals
def test_refused_calls_name_the_kind(lib):
    n, d = 67, 3
    C = B.instance(n, d, 6, 0.3)[0]
    N = n * (d + 1)
    before = lib.pool_stats()[1]
    h = lib.Handle.posegraph(C, d)
    try:
        with pytest.raises(lib.MsdpError, match="pose-graph") as e:
            h.debug_shard(2, 0)                                              # (it is a call for handles without a point)
        assert e.value.code == lib.EUNSUPPORTED
        Y = B.point(n, d, 4)
        h.set_point(Y)
        for call in (lambda: h.comm_init_local(1, 0, 4245), lambda: h.comm_init(1, 0, bytes(128)),
                     lambda: h.comm_init_ipc(1, 0, "/msdp_pose_refused"), lambda: h.round_hyperplane(np.ones((64, 4))),
                     lambda: h.linesearch_accept(),                          # (its guard keeps `cur` and the state as they are)
                     lambda: h.factor_gram(), lambda: h.factor_rotate(np.eye(4)), lambda: h.factor_append(np.ones((N, 1)), 0.5),
                     lambda: h.linesearch_cost(Y, 0.5)):
            with pytest.raises(lib.MsdpError, match="pose-graph") as e:
                call()
            assert e.value.code == lib.EUNSUPPORTED
        assert np.isfinite(h.cost()) and np.array_equal(h.get_point(), Y)   # the handle still works
        with pytest.raises(lib.MsdpError, match="pose-graph") as e:
            h.set_point(np.zeros((N, 258)))
        assert e.value.code == lib.EUNSUPPORTED
    finally:
        h.close()
    # at the C ABI: N % (d + 1) != 0, d outside {2, 3}, pcap > 256
    Cc = sp.csc_matrix(C)
    Cc.sort_indices()
    jc, ir, val = Cc.indptr.astype(np.int64), Cc.indices.astype(np.int64), Cc.data.astype(np.float64)
    i64p, dp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    create = lib.load().msdp_create_posegraph_csc
    for dd, pcap, code in ((2, 32, lib.EINVAL), (4, 32, lib.EINVAL), (1, 32, lib.EINVAL), (0, 32, lib.EINVAL),
                           (3, 257, lib.EUNSUPPORTED)):
        out = ctypes.c_void_p()
        rc = create(N, dd, jc.ctypes.data_as(i64p), ir.ctypes.data_as(i64p), val.ctypes.data_as(dp), pcap, ctypes.byref(out))
        assert rc == code and not out.value, (dd, pcap)
        with pytest.raises(lib.MsdpError, match="pose-graph"):
            lib._check(rc)
    assert lib.pool_stats()[1] == before
