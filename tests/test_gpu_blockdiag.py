"""The unit-block-diagonal handle (msdp_create_onlyunitblockdiag_csc, Handle.onlyunitblockdiag, msdp_stiefel.hip) against the
NumPy restatement of tests/blockdiag_ref.py: point operations over every dispatched <LPR, NCH> instance for d = 2 and 3, the
block-CSR gather against the plain sparse handle, trustregions() counts, the escape's eigenpairs, whole solves against the
restatement and the CPU oracle on the affine formulation, and the refused calls."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import blockdiag_ref as B

pytestmark = pytest.mark.gpu

# (n, d) ragged against the lane groups per wave and the workgroup chunks; degrees 2 and 6, one instance with diagonal blocks
SHAPES = {(101, 2): dict(degree=6, diag=False), (67, 3): dict(degree=2, diag=False), (343, 3): dict(degree=6, diag=True)}
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
    n, d = shape
    C, _, _ = B.instance(n, d, SHAPES[shape]["degree"], 1.0, diag=SHAPES[shape]["diag"])
    h = lib.Handle.onlyunitblockdiag(C, d, pcap=256)
    try:
        for p in _widths(d):
            Y = B.point(n, d, p)
            M = B.StiefelStacked(n, d, p)
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
            for bn in (0.1, 10.0):                                           # tangent directions of block norm up to 10
                Ub = B.tangent_direction(Y, d, g, blocknorm=bn)
                Zr = h.retr(Ub)
                errs["retr%g" % bn] = _relerr(Zr, M.retr(Y, Ub))
                Z3 = B.to3(Zr, d)
                errs["orth%g" % bn] = float(np.max(np.abs(Z3 @ np.swapaxes(Z3, 1, 2) - np.eye(d))))
            print("n %d d %d p %d: " % (n, d, p) + " ".join("%s %.1e" % kv for kv in errs.items()))
            assert all(v < 1e-12 for v in errs.values()), (p, errs)
            assert L.shape == (n, d, d) and np.array_equal(L, np.swapaxes(L, 1, 2))
            assert abs(np.sum(z) - 2.0 * f) <= 1e-12 * max(1.0, abs(f))      # sum z = <C, X> = 2 cost
            assert np.array_equal(H, h.hessvec(U)) and np.array_equal(G, h.rgrad()) and f == h.cost()   # fixed summation orders
            assert np.array_equal(h.get_point(), Y)
            ms, by, fl = h.bench_hessvec(50)                                 # the measurement entry point accepts the kind
            assert ms > 0 and by > 0 and fl > 0
            if p == 12:
                assert h.bench_tcg_trip(16) > 0                              # ... and so does the generic chunked trip
    finally:
        h.close()


@pytest.mark.parametrize("n,d,q", [(101, 2, 3), (67, 3, 1), (343, 3, 11)])
def test_block_csr_against_plain_csr(lib, n, d, q):
    """C = A (x) I_d and a point whose block rows live in disjoint column sets (d independent unit-row factors): the block problem
    decouples into d copies of the plain sparse problem of A, row set by row set."""
    import lowrank_ref
    A = sp.csr_matrix(lowrank_ref.grid_cs(n))
    C = sp.kron(A, sp.identity(d), format="csr")
    g = np.random.default_rng(40 + q)
    Ys = g.standard_normal((d, n, q))
    Ys /= np.linalg.norm(Ys, axis=2, keepdims=True)
    Us = g.standard_normal((d, n, q))
    Us -= Ys * np.sum(Ys * Us, axis=2, keepdims=True)                         # tangent to each oblique factor
    Y = np.zeros((n, d, d * q))
    U = np.zeros((n, d, d * q))
    for a in range(d):
        Y[:, a, a * q:(a + 1) * q] = Ys[a]
        U[:, a, a * q:(a + 1) * q] = Us[a]
    Y, U = Y.reshape(n * d, d * q), U.reshape(n * d, d * q)
    h = lib.Handle.onlyunitblockdiag(C, d, pcap=d * q)
    hs = lib.Handle.onlyunitdiag(A, pcap=max(q, 2))
    try:
        h.set_point(Y)
        G, H, z = B.to3(h.rgrad(), d), B.to3(h.hessvec(U), d), h.get_z().reshape(n, d)
        for a in range(d):
            hs.set_point(np.ascontiguousarray(Ys[a]))
            Gs, Hs, zs = hs.rgrad(), hs.hessvec(np.ascontiguousarray(Us[a])), hs.get_z()
            e = (_relerr(G[:, a, a * q:(a + 1) * q], Gs), _relerr(H[:, a, a * q:(a + 1) * q], Hs), _relerr(z[:, a], zs))
            print("n %d d %d q %d row set %d: grad %.1e hess %.1e z %.1e" % ((n, d, q, a) + e))
            assert max(e) < 1e-12
            off = np.ones(d * q, dtype=bool)
            off[a * q:(a + 1) * q] = False
            assert np.max(np.abs(G[:, a, off])) < 1e-12 and np.max(np.abs(H[:, a, off])) < 1e-12
    finally:
        h.close(); hs.close()


# ------------------------------------------------------------------ trustregions()
def test_rtr_counts_match_the_restatement(lib):
    c = B.COUNT_CASE
    C, Y0 = B.count_case()
    _, f_ref, info = B.trustregions(C, Y0, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
    h = lib.Handle.onlyunitblockdiag(C, c["d"], pcap=c["p"])
    try:
        h.set_point(Y0)
        assert h.tcg_path() == 0 and h.persist_form() == -1
        st = h.rtr(lib.default_opts(maxiter=c["maxiter"], maxinner=c["maxinner"], tolgradnorm=c["tolgradnorm"]))
        dev = (st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner)
        print("rtr: device", dev, st.cost, "restatement", B.counts(info), f_ref)
        assert dev == B.counts(info)
        assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
        assert abs(h.cost() - st.cost) <= 1e-11 * abs(st.cost)
        Y3 = B.to3(h.get_point(), c["d"])
        assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(c["d"]))) < 1e-13      # twenty retractions later
    finally:
        h.close()


# ------------------------------------------------------------------ escape
@pytest.mark.parametrize("n,d,stationary", [(101, 2, False), (67, 3, False), (101, 2, True), (67, 3, True)])
def test_escape_eigs_against_lapack(lib, n, d, stationary):
    C, _, _ = B.instance(n, d, 6, 1.5 if d == 2 else 2.0)
    k = d
    h = lib.Handle.onlyunitblockdiag(C, d)
    try:
        h.set_point(B.point(n, d, d if stationary else d + 2))
        if stationary:
            # a critical point of the width-d problem that is no optimum of the SDP: S Y = 0 and S has negative eigenvalues;
            # the gradient is below the escape's threshold for deflating span(Y)
            st = h.rtr(lib.default_opts(maxiter=200, maxinner=100, tolgradnorm=1e-9))
            assert st.gradnorm <= 1e-6 * max(1.0, abs(st.cost))
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
    assert V.shape == (n * d, k)
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
    # ... and they are the bottom of the spectrum.  At a critical point of the d = 2 problem with rotation data S commutes with
    # the block-wise rotation by 90 degrees and every eigenvalue is double: a Krylov space holds one direction of an eigenspace,
    # so the t-th returned value lies between the t-th eigenvalue and the t-th DISTINCT one (both are descent directions of
    # the widening step); everywhere else the spectrum is simple and the k values are the k smallest.
    distinct = [dS[0]]
    for x in dS[1:]:
        if x - distinct[-1] > 1e-7 * scale:
            distinct.append(x)
    double = len(distinct) <= len(dS) // 2 + 1
    assert double == (stationary and d == 2)
    for t in range(k):
        assert dS[t] - 1e-8 <= lam[t] <= (distinct[t] if double else dS[t]) + 1e-8, (t, lam, dS[:k], distinct[:k])


# ------------------------------------------------------------------ solves
_REF = {}


def _reference(n, d, sigma):
    """The restatement's solve from p0 = d and the CPU oracle on the affine formulation, once per instance.  The oracle runs
    with 20 trust-region iterations of up to 50 inner steps per outer iteration: with its defaults (4 of 20) it stops on
    "slow progress" 2.6e-6 above the optimum on the d = 3 instance."""
    key = (n, d, sigma)
    if key not in _REF:
        from oracle import manisdp_ref as R
        C, Rt, edges = B.instance(n, d, 6, sigma)
        Y0 = B.random_point(n, d, d, np.random.default_rng(1))
        _, obj_r, data_r = B.solve(C, d, Y0)
        assert data_r["status"] == 0 and data_r["dinf"] < 1e-8
        At, b, c, K = B.affine_formulation(C, d)
        _, obj_a, data_a = R.ManiSDP_unitdiag(At, b, c, K, {"tol": 1e-9, "TR_maxiter": 20, "TR_maxinner": 50})
        assert data_a["status"] == 0
        _REF[key] = dict(C=C, Y0=Y0, obj_r=obj_r, data_r=data_r, obj_a=obj_a)
    return _REF[key]


def test_noise_free_solve(lib):
    from manisdp_matlab_amd import problems, solvers
    n, d = 67, 3
    C, Rt, edges = B.instance(n, d, 6, 0.0)
    Y, obj, data = solvers.ManiSDP_onlyunitblockdiag(C, d, verbose=False)
    print("noise-free: obj %.10f (-2|E|d = %d), rank %d, p %d, dinf %.1e" % (obj, -2 * len(edges) * d, data["rank"], data["p"], data["dinf"]))
    assert data["status"] == 0 and data["dinf"] < 1e-8
    assert abs(obj + 2 * len(edges) * d) <= 1e-6
    assert data["rank"] == d
    assert problems.rotation_error(problems.round_rotations(Y, d), Rt) <= 1e-6


@pytest.mark.parametrize("n,d,sigma", [(67, 3, 2.0), (101, 2, 1.5)])
@pytest.mark.parametrize("eig", ["host", "device"])
def test_noisy_solves_from_p0_equal_d(lib, n, d, sigma, eig):
    from manisdp_matlab_amd import solvers
    m = _reference(n, d, sigma)
    Y, obj, data = solvers.ManiSDP_onlyunitblockdiag(m["C"], d, {"Y0": m["Y0"], "eig": eig}, verbose=False)
    print("n %d d %d sigma %g (%s): %.10f, restatement %.10f (%d iterations, p %d), affine oracle %.10f; device %d iterations, p %d, dinf %.1e"
          % (n, d, sigma, eig, obj, m["obj_r"], m["data_r"]["iters"], m["data_r"]["p"], m["obj_a"], data["iters"], data["p"], data["dinf"]))
    assert data["status"] == 0 and data["dinf"] < 1e-8
    assert data["iters"] >= 2                                                # the staircase fires from p0 = d
    assert abs(obj - m["obj_r"]) <= 1e-6
    assert abs(obj - m["obj_a"]) <= 1e-6
    Y3 = B.to3(Y, d)
    assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(d))) < 1e-12     # X_[ii] = I_d
    assert abs(float(np.sum(m["C"].multiply(data["X"]))) - obj) <= 1e-9 * abs(obj)     # <C, X> = obj
    assert abs(np.sum(data["z"]) - obj) <= 1e-12 * abs(obj)


def test_larger_solve_with_the_device_escape(lib):
    from manisdp_matlab_amd import solvers
    n, d = 343, 3
    C, _, _ = B.instance(n, d, 6, 1.0)
    _, obj_r, data_r = B.solve(C, d, B.random_point(n, d, d + 2, np.random.default_rng(1)))
    assert data_r["status"] == 0
    Y, obj, data = solvers.ManiSDP_onlyunitblockdiag(C, d, {"eig": "device"}, verbose=False)
    print("n %d d %d: %.10f, restatement %.10f; %d iterations, p %d, dinf %.1e, %d cold checks" % (
        n, d, obj, obj_r, data["iters"], data["p"], data["dinf"], data.get("eig_verifications", 0)))
    assert data["status"] == 0 and data["dinf"] < 1e-8
    assert data["eig_verifications"] >= 1 and data["escape_method"] == 0     # certified by the independent cold check (Lanczos)
    assert abs(obj - obj_r) <= 1e-6 * abs(obj_r)


# ------------------------------------------------------------------ refusals
def test_refused_calls_name_the_kind(lib):
    n, d = 67, 3
    C, _, _ = B.instance(n, d, 2, 1.0)
    before = lib.pool_stats()[1]
    h = lib.Handle.onlyunitblockdiag(C, d)
    try:
        Y = B.point(n, d, 4)
        h.set_point(Y)
        for call in (lambda: h.comm_init_local(1, 0, 4245), lambda: h.round_hyperplane(np.ones((64, 4))), lambda: h.factor_gram(),
                     lambda: h.factor_rotate(np.eye(4)), lambda: h.factor_append(np.ones((n * d, 1)), 0.5),
                     lambda: h.linesearch_cost(Y, 0.5)):
            with pytest.raises(lib.MsdpError, match="unit-block-diagonal") as e:
                call()
            assert e.value.code == lib.EUNSUPPORTED
        assert np.isfinite(h.cost()) and np.array_equal(h.get_point(), Y)   # the handle still works
        with pytest.raises(lib.MsdpError, match="unit-block-diagonal") as e:
            h.set_point(np.zeros((n * d, 258)))
        assert e.value.code == lib.EUNSUPPORTED
    finally:
        h.close()
    hs = lib.Handle.onlyunitdiag(sp.csr_matrix(C))
    try:
        hs.set_point(B.point(n, d, 4))
        with pytest.raises(lib.MsdpError, match="unit-block-diagonal") as e:
            hs.get_blockmult()                                               # (its block order is 0: the library decides)
        assert e.value.code == lib.EUNSUPPORTED
    finally:
        hs.close()
    # at the C ABI: N % d != 0, d outside {2, 3}, pcap > 256
    Cc = sp.csc_matrix(C)
    Cc.sort_indices()
    jc, ir, val = Cc.indptr.astype(np.int64), Cc.indices.astype(np.int64), Cc.data.astype(np.float64)
    i64p, dp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    create = lib.load().msdp_create_onlyunitblockdiag_csc
    for dd, pcap, code in ((2, 32, lib.EINVAL), (4, 32, lib.EINVAL), (1, 32, lib.EINVAL), (3, 257, lib.EUNSUPPORTED)):
        out = ctypes.c_void_p()
        rc = create(n * d, dd, jc.ctypes.data_as(i64p), ir.ctypes.data_as(i64p), val.ctypes.data_as(dp), pcap, ctypes.byref(out))
        assert rc == code and not out.value, (dd, pcap)
        with pytest.raises(lib.MsdpError, match="unit-block-diagonal"):
            lib._check(rc)
    assert lib.pool_stats()[1] == before
