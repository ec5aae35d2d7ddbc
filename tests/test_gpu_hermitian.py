"""The Hermitian cost kind C = A + iB on the device (msdp_create_onlyunitdiag_csc_hermitian, Handle.onlyunitdiag_hermitian)
against the complex restatement of tests/hermitian_ref.py, the dense real handle of the order-2n embedding and the CPU oracle on
the real view: derivatives over every instance of the row kernels, the conjugation, bit identity with the plain sparse handle
at B = 0, one trustregions() call, the Lanczos escape against LAPACK, whole solves of phase-synchronisation instances and the
refusals.

Tolerances are those of tests/test_gpu_lowrank.py for the same quantities (1e-12 relative on operator outputs; counts equal
and the cost to 1e-11 for a trustregions() call; 1e-6 on a solve's optimum) and of tests/test_gpu_escape.py for the Lanczos
path."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import hermitian_ref as HR

pytestmark = pytest.mark.gpu
PCAP = max(HR.P_GRID)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _check_derivatives(lib, C, n, p, h, hd):
    """cost, gradient, Hess-vec and z of the Hermitian handle h at complex width p against the restatement and against the
    dense real handle hd of the embedding at the embedded point (twice the cost; the blocks of its outputs)."""
    Y, U = HR.table_point(n, p), HR.table_direction(n, p)
    h.set_point(Y)
    assert h.tcg_path() == 0 and h.persist_form() == -1
    f, G, H, z = h.cost(), h.rgrad(), h.hessvec(U), h.get_z()
    assert G.dtype == np.complex128 and G.shape == (n, p) and H.shape == (n, p) and z.dtype == np.float64 and z.shape == (n,)
    f_ref = HR.cost(C, Y)
    hd.set_point(HR.embed_point(Y))
    fd, Gd, Hd, zd = hd.cost(), hd.rgrad(), hd.hessvec(HR.embed_point(U)), hd.get_z()
    Gd = Gd[:n, :p] + 1j * Gd[n:, :p]
    Hd = Hd[:n, :p] + 1j * Hd[n:, :p]
    print("n %d p %d: cost %.2e / %.2e grad %.2e / %.2e hess %.2e / %.2e z %.2e / %.2e" % (
        n, p, abs(f - f_ref) / max(1.0, abs(f_ref)), abs(2 * f - fd) / max(1.0, abs(fd)), _relerr(G, HR.rgrad(C, Y)), _relerr(G, Gd),
        _relerr(H, HR.hessvec(C, Y, U)), _relerr(H, Hd), _relerr(z, HR.get_z(C, Y)), _relerr(z, zd[:n])))
    assert abs(f - f_ref) <= 1e-12 * max(1.0, abs(f_ref)), p
    assert _relerr(G, HR.rgrad(C, Y)) < 1e-12 and _relerr(H, HR.hessvec(C, Y, U)) < 1e-12, p
    assert _relerr(z, HR.get_z(C, Y)) < 1e-12, p
    assert abs(2.0 * f - fd) <= 1e-12 * max(1.0, abs(fd)), p
    assert _relerr(G, Gd) < 1e-12 and _relerr(H, Hd) < 1e-12, p
    assert _relerr(z, zd[:n]) < 1e-12 and _relerr(z, zd[n:]) < 1e-12, p
    assert np.array_equal(H, h.hessvec(U)) and np.array_equal(G, h.rgrad()) and f == h.cost()    # fixed summation orders, no atomics
    assert np.array_equal(h.get_point(), Y)
    assert h.tcg_path() == 0 and h.persist_form() == -1


# ------------------------------------------------------------------ derivatives
@pytest.mark.parametrize("storage", HR.STORAGES)
@pytest.mark.parametrize("n", HR.N_GRID)
def test_derivatives_against_restatement_and_embedded_dense_handle(lib, n, storage):
    C = HR.instance(storage, n)
    h, hd = lib.Handle.onlyunitdiag_hermitian(C, pcap=PCAP), lib.Handle.onlyunitdiag(HR.embed(C).toarray(), pcap=2 * PCAP)
    try:
        for p in HR.P_GRID:
            _check_derivatives(lib, C, n, p, h, hd)
    finally:
        h.close(); hd.close()


@pytest.mark.parametrize("storage", HR.STORAGES)
def test_derivatives_at_the_widest_instances(lib, storage):
    """Real widths 130 and 260: two and four column chunks per lane on 64 lanes per row."""
    n = 203
    C = HR.instance(storage, n)
    h, hd = lib.Handle.onlyunitdiag_hermitian(C, pcap=PCAP), lib.Handle.onlyunitdiag(HR.embed(C).toarray(), pcap=2 * PCAP)
    try:
        for p in HR.P_WIDE:
            _check_derivatives(lib, C, n, p, h, hd)
    finally:
        h.close(); hd.close()


def test_conjugate_matrix_is_another_problem(lib):
    """Row i of C is the conjugate of column i of the CSC input: reading the columns as rows would solve conj(C)."""
    n, p = 203, 5
    C = HR.instance("hub", n)
    Cc = sp.csr_matrix(C.conj())
    Y, U = HR.table_point(n, p), HR.table_direction(n, p)
    h, hc = lib.Handle.onlyunitdiag_hermitian(C), lib.Handle.onlyunitdiag_hermitian(Cc)
    try:
        h.set_point(Y); hc.set_point(Y)
        H, Hc = h.hessvec(U), hc.hessvec(U)
        G, Gc = h.rgrad(), hc.rgrad()
    finally:
        h.close(); hc.close()
    print("conj: hess differ %.2e, grad differ %.2e" % (_relerr(H, Hc), _relerr(G, Gc)))
    assert _relerr(H, Hc) > 1e-3
    assert _relerr(H, HR.hessvec(C, Y, U)) < 1e-12 and _relerr(Hc, HR.hessvec(Cc, Y, U)) < 1e-12
    assert _relerr(G, HR.rgrad(C, Y)) < 1e-12 and _relerr(Gc, HR.rgrad(Cc, Y)) < 1e-12


@pytest.mark.parametrize("storage", HR.STORAGES)
@pytest.mark.parametrize("n", HR.N_GRID)
def test_zero_imaginary_part_is_the_sparse_handle_bit_for_bit(lib, n, storage):
    """With B = 0 the complex gather adds exact zeros between the products of the real one, in the same order: the Hermitian
    handle at complex width p equals the plain sparse handle of A at real width 2p."""
    A = sp.csr_matrix(HR.instance(storage, n).real)
    widths = HR.P_GRID + (HR.P_WIDE if n == 203 else ())
    h, hs = lib.Handle.onlyunitdiag_hermitian(A.astype(np.complex128), pcap=PCAP), lib.Handle.onlyunitdiag(A, pcap=2 * PCAP)
    try:
        for p in widths:
            Y, U = HR.table_point(n, p), HR.table_direction(n, p)
            h.set_point(Y); hs.set_point(HR.real_view(Y))
            assert h.cost() == hs.cost(), p
            assert np.array_equal(HR.real_view(h.rgrad()), hs.rgrad()), p
            assert np.array_equal(HR.real_view(h.hessvec(U)), hs.hessvec(HR.real_view(U))), p
            assert np.array_equal(h.get_z(), hs.get_z()), p
    finally:
        h.close(); hs.close()


# ------------------------------------------------------------------ trustregions()
@pytest.mark.parametrize("n,p,storage", [(203, 3, "grid"), (1031, 9, "hub"), (1031, 17, "grid")])
def test_rtr_matches_the_oracle_on_the_real_view(lib, n, p, storage):
    from oracle import manisdp_ref as R, manopt_rtr
    C = HR.instance(storage, n)
    Y = HR.table_point(n, p)
    prob = R._OnlyUnitDiagProblem(HR.Op(C), n, 2 * p, q1="correct")
    _, f_ref, info = manopt_rtr.trustregions(prob, HR.real_view(Y).copy(), 3, 20, 1e-8)
    h = lib.Handle.onlyunitdiag_hermitian(C, pcap=p)
    try:
        h.set_point(Y)
        assert h.tcg_path() == 0 and h.persist_form() == -1                  # the generic per-iteration path
        st = h.rtr(lib.default_opts(maxiter=3, maxinner=20, tolgradnorm=1e-8))
        print("rtr: device", (st.iters, st.hessvecs, st.accepted, st.rejected, st.cost), "oracle",
              (info.iters, info.hessvecs, info.accepted, info.rejected, f_ref))
        assert (st.iters, st.hessvecs, st.accepted, st.rejected) == (info.iters, info.hessvecs, info.accepted, info.rejected)
        assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
        assert abs(h.cost() - st.cost) < 1e-10 * max(1.0, abs(st.cost))
        assert h.tcg_path() == 0 and h.persist_form() == -1
    finally:
        h.close()


# ------------------------------------------------------------------ escape
@pytest.mark.parametrize("n,p,storage", [(203, 4, "hub"), (1031, 6, "grid")])
def test_escape_eigs_against_lapack(lib, n, p, storage):
    C = HR.instance(storage, n)
    Y = HR.table_point(n, p)                                                 # not a stationary point: S*Y != 0
    k = 4
    h = lib.Handle.onlyunitdiag_hermitian(C)
    try:
        h.set_point(Y)
        z = h.get_z()
        lam, V, lmax, its = h.escape_eigs(k, tol=1e-9, maxit=600)
        assert h.escape_method() == 0                                        # Lanczos: the block eigen-solver stays real-sparse only
    finally:
        h.close()
    S = (C - sp.diags(z)).toarray()
    dS = np.linalg.eigh(S)[0]
    scale = max(abs(dS[0]), abs(dS[-1]))
    # the reference spectrum is separated where the test looks, so nothing below can pass by confusing two eigenvalues: the six
    # bottom eigenvalues lie at least 9e-3 apart in absolute terms (0.14 at n = 203; 0.0092 = 2.9e-3 * scale at n = 1031, scale
    # 3.13 -- six orders above the 1e-8 * scale a match is allowed), the top two at least 9e-3 * scale
    assert np.min(np.diff(dS[:6])) > 9e-3 and dS[-1] - dS[-2] > 9e-3 * scale
    print("escape: lam", lam, "lapack", dS[:k], "lmax err %.2e (scale %.3f, %d steps)" % (abs(lmax - dS[-1]), scale, its))
    assert V.dtype == np.complex128 and V.shape == (n, k)
    assert abs(lmax - dS[-1]) < 1e-5 * scale
    assert abs(lam[0] - dS[0]) < 1e-8 * scale
    assert np.all(np.diff(lam) >= 0)
    assert lam[0] < 0
    used = set()
    cols = []
    for t in range(k):
        if lam[t] < -1e-9 * scale:
            v = V[:, t]
            j = int(np.argmin(np.abs(dS - lam[t])))
            assert abs(dS[j] - lam[t]) < 1e-8 * scale, t
            assert j not in used, "eigenvalue %d of S reported twice (a v / iv pair)" % j
            used.add(j)
            assert np.linalg.norm(S @ v - lam[t] * v) < 1e-5 * scale, t
            cols.append(t)
    Vc = V[:, [t for t in range(k) if np.isfinite(lam[t])]]
    assert np.max(np.abs(Vc.conj().T @ Vc - np.eye(Vc.shape[1]))) < 1e-6
    assert len(cols) >= 2                                                    # both S have several negative eigenvalues at this point


# ------------------------------------------------------------------ solve
_SYNC = {}


def _sync_instance(n, sigma):
    key = (n, sigma)
    if key not in _SYNC:
        from manisdp_matlab_amd import problems
        from oracle import manisdp_ref as R
        C, z = problems.phase_synchronization(n, 8, sigma, np.random.default_rng(7))
        g = np.random.default_rng(1)
        Y0 = g.standard_normal((n, 2)) + 1j * g.standard_normal((n, 2))
        Y0 /= np.sqrt(np.sum(np.abs(Y0) ** 2, axis=1, keepdims=True))
        ref = {}
        for p0 in ((1, 2) if n == 203 else (2,)):
            Y0p = np.ascontiguousarray(Y0[:, :p0] / np.sqrt(np.sum(np.abs(Y0[:, :p0]) ** 2, axis=1, keepdims=True)))
            _, obj_r, data_r = HR.solve(C, Y0p)
            assert data_r["status"] == 0 and data_r["dinf"] < 1e-8
            ref[p0] = (Y0p, obj_r, data_r)
        # the CPU oracle on the embedding: order 2n, real Y0 of width 2, twice the optimum
        _, obj_e, data_e = R.ManiSDP_onlyunitdiag(HR.embed(C), {"Y0": HR.embed_point(ref[min(ref)][0][:, :1])}, q1="correct")
        assert data_e["status"] == 0 and data_e["dinf"] < 1e-8
        _SYNC[key] = dict(C=C, z=z, ref=ref, obj_embedded=obj_e)
    return _SYNC[key]


def _check_solve(m, p0, eig):
    from manisdp_matlab_amd import solvers
    C = m["C"]
    n = C.shape[0]
    Y0p, obj_r, data_r = m["ref"][p0]
    Y, obj, data = solvers.ManiSDP_onlyunitdiag(C, {"Y0": Y0p, "eig": eig}, verbose=False)
    print("phase sync n %d p0 %d (%s): %.10f, restatement %.10f (%d iterations, rank %d), embedded oracle / 2 %.10f; device %d iterations, p %d"
          % (n, p0, eig, obj, obj_r, data_r["iters"], data_r["rank"], 0.5 * m["obj_embedded"], data["iters"], data["p"]))
    assert data["status"] == 0
    assert abs(obj - obj_r) < 1e-6 * abs(obj_r)
    assert abs(obj - 0.5 * m["obj_embedded"]) < 1e-6 * abs(obj_r)
    assert data["dinf"] < 1e-8
    X = data["X"]
    assert Y.dtype == np.complex128 and X.shape == (n, n)
    assert np.max(np.abs(np.diag(X) - 1.0)) < 1e-12
    assert np.array_equal(X, X.conj().T) or np.max(np.abs(X - X.conj().T)) < 1e-15
    assert abs(np.real(np.sum(C.multiply(X.conj()))) - obj) < 1e-9 * abs(obj)         # <C, X> = obj
    if eig == "device":
        assert data["escape_method"] == 0
    return data


@pytest.mark.parametrize("eig", ["host", "device"])
@pytest.mark.parametrize("p0", [1, 2])
def test_phase_synchronization_solve(lib, p0, eig):
    _check_solve(_sync_instance(203, 3.0), p0, eig)


def test_phase_synchronization_solve_larger(lib):
    _check_solve(_sync_instance(1031, 4.0), 2, "device")


# ------------------------------------------------------------------ refusals
def test_refusals_name_the_kind(lib):
    n = 203
    C = HR.instance("grid", n)
    before = lib.pool_stats()[1]
    h = lib.Handle.onlyunitdiag_hermitian(C)
    try:
        # an odd real width through the raw call
        Yodd = np.ascontiguousarray(HR.real_view(HR.table_point(n, 2))[:, :3])
        rc = h._lib.msdp_set_point(h._h, 3, Yodd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        assert rc == lib.EINVAL
        with pytest.raises(lib.MsdpError, match="Hermitian") as e:
            lib._check(rc)
        assert e.value.code == lib.EINVAL
        with pytest.raises(lib.MsdpError, match="Hermitian") as e:
            h.comm_init_local(1, 0, 4244)
        assert e.value.code == lib.EUNSUPPORTED
        h.set_point(HR.table_point(n, 2))                                   # the handle still works
        assert np.isfinite(h.cost())
        with pytest.raises(lib.MsdpError, match="Hermitian") as e:
            h.round_hyperplane(np.ones((64, 2)))
        assert e.value.code == lib.EUNSUPPORTED
        with pytest.raises(lib.MsdpError, match="Hermitian") as e:
            h.factor_gram()
        assert e.value.code == lib.EUNSUPPORTED
        with pytest.raises(lib.MsdpError, match="Hermitian") as e:
            h.factor_rotate(np.eye(2))
        assert e.value.code == lib.EUNSUPPORTED
        with pytest.raises(lib.MsdpError, match="Hermitian") as e:
            h.factor_append(np.ones((n, 1)), 0.5)
        assert e.value.code == lib.EUNSUPPORTED
        assert np.array_equal(h.get_point(), HR.table_point(n, 2))
    finally:
        h.close()
    # a non-zero imaginary diagonal at the C ABI (the Python check is bypassed)
    Cc = sp.csc_matrix(C + sp.identity(n, dtype=np.complex128, format="csr"))
    Cc.sort_indices()
    val = Cc.data.copy()
    k = int(Cc.indptr[7] + np.nonzero(Cc.indices[Cc.indptr[7]:Cc.indptr[8]] == 7)[0][0])
    val[k] = 1.0 + 0.5j
    jc, ir = Cc.indptr.astype(np.int64), Cc.indices.astype(np.int64)
    out = ctypes.c_void_p()
    i64p, dp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    rc = lib.load().msdp_create_onlyunitdiag_csc_hermitian(n, jc.ctypes.data_as(i64p), ir.ctypes.data_as(i64p),
                                                           val.view(np.float64).ctypes.data_as(dp), 32, ctypes.byref(out))
    assert rc == lib.EINVAL and not out.value
    with pytest.raises(lib.MsdpError, match="Hermitian"):
        lib._check(rc)
    assert lib.pool_stats()[1] == before
    with pytest.raises(ValueError, match="Hermitian"):
        lib.Handle.onlyunitdiag_hermitian(sp.csr_matrix((val, Cc.indices, Cc.indptr), shape=(n, n)))
