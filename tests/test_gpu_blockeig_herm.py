"""GPU tests of the block eigen-solver of the saddle escape on a Hermitian cost matrix (option escape_method = 2 on a
Handle.onlyunitdiag_hermitian handle: k_be_step_herm, be_ritz_herm and k_be_extract_herm of msdp_blockeig.hip on a complex
panel of 16 / 32 / 64 columns) against LAPACK's eigh of the complex S = C - diag(z), through msdp_escape_eigs.

Tolerances are the real route's (tests/test_gpu_blockeig.py, whose _check_pairs is used as it is): values 2e-3 * scale and
residuals |S v - lambda v| 2e-2 * scale on a warm call (2 % of |theta| is what such a call is asked for), lambda_max 1e-6 * scale,
lambda_min of the cold check 1e-9 * scale with a lower bound within 1e-8 * scale, scale = max |lambda|.  The residual is taken
against the true complex S: a conjugated gather computes the spectrum of conj(S) -- the same values -- and fails there.
Orthonormality of the returned vectors: 1e-8, the bound tests/test_blockeig_herm_host.py puts on W^H G W = I of the stage that
produces them -- the closing stage of a call works on vectors that are already orthonormal to the conditioning of the filtered
block's Gram matrix, so its own G is the identity to that error and nothing amplifies the rounding of its Gram sums.  Instances: tests/hermitian_ref.py, fixed-width rows ("grid") and CSR rows of more than 64 entries ("hub") at
n = 257 (the smallest order past the route's lower limit of 256) and 1031."""
import numpy as np
import pytest
import scipy.sparse as sp

import hermitian_ref as HR
from test_gpu_blockeig import _check_pairs

pytestmark = pytest.mark.gpu

# (be_width in real columns, be_lpr): the nine instances be_step dispatches
STEP_INSTANCES = [(32, 16), (32, 8), (64, 32), (64, 16), (64, 8), (128, 64), (128, 32), (128, 16), (128, 8)]


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _reference(C, h):
    S = (C - sp.diags(h.get_z())).toarray()
    return S, np.linalg.eigvalsh(S)


def _cold(h):
    h.set_option("escape_deflate", 0); h.set_option("escape_warm", 0); h.set_option("escape_start_y", 0)


def _cold_check(h, w):
    """The independent check of the host loops: hashed noise only, nothing of Y, nothing carried over, k = 1."""
    _cold(h)
    lam1, V1, lmax1, _ = h.escape_eigs(1, tol=1e-9, maxit=60000)
    scale = max(abs(w[0]), abs(w[-1]))
    lb = h.escape_lower_bound()
    print("cold: lambda_min err %.2e * scale, lower bound %.3e below" % (abs(lam1[0] - w[0]) / scale, lam1[0] - lb))
    assert h.escape_method() == 1 and h.escape_info()[1]
    assert abs(lam1[0] - w[0]) <= 1e-9 * scale
    assert np.isfinite(lb) and lb <= lam1[0] and lam1[0] - lb <= 1e-8 * scale


def _warm_call(h, S, w, k):
    lam, V, lmax, deg = h.escape_eigs(k, tol=1e-9, maxit=60000)
    assert h.escape_method() == 1
    nvalid, conv, _ = h.escape_info()
    scale = max(abs(w[0]), abs(w[-1]))
    print("k = %d: %d steps, value err %.2e * scale, lmax err %.2e * scale" % (k, deg, abs(lam[0] - w[0]) / scale, abs(lmax - w[-1]) / scale))
    assert conv and nvalid == k
    assert h.escape_lower_bound() == -np.inf                   # a warm call never reports a bound
    assert V.dtype == np.complex128 and V.shape == (S.shape[0], k)
    assert np.max(np.abs(V.conj().T @ V - np.eye(k))) <= 1e-8
    _check_pairs(S, w, lam, V, lmax, k, 2e-3, 2e-2)
    return lam


# ------------------------------------------------------------------ 1. against LAPACK at a non-stationary point
@pytest.mark.parametrize("p", [3, 6])
@pytest.mark.parametrize("n", [257, 1031])
@pytest.mark.parametrize("storage", HR.STORAGES)
def test_block_escape_matches_lapack_at_a_table_point(lib, storage, n, p):
    C = HR.instance(storage, n)
    h = lib.Handle.onlyunitdiag_hermitian(C)
    try:
        h.set_option("escape_method", 2)
        h.set_point(HR.table_point(n, p))
        S, w = _reference(C, h)
        _warm_call(h, S, w, 4)
        _cold_check(h, w)
    finally:
        h.close()


# ------------------------------------------------------------------ 2. every instance of the filter step
@pytest.mark.parametrize("storage,n", [("grid", 1031), ("hub", 257)])
def test_every_step_instance_finds_lambda_min(lib, storage, n):
    """be_width 32 / 64 / 128 (16 / 32 / 64 complex columns) x every be_lpr be_step accepts for it, on fixed-width rows (the ELL
    form) and on CSR rows: a cold call each, lambda_min against LAPACK."""
    C = HR.instance(storage, n)
    h = lib.Handle.onlyunitdiag_hermitian(C)
    try:
        h.set_option("escape_method", 2)
        h.set_point(HR.table_point(n, 3))
        S, w = _reference(C, h)
        scale = max(abs(w[0]), abs(w[-1]))
        _cold(h)
        for width, lpr in STEP_INSTANCES:
            h.set_option("be_width", width); h.set_option("be_lpr", lpr)
            lam, V, lmax, deg = h.escape_eigs(1, tol=1e-9, maxit=60000)
            print("be_width %3d be_lpr %2d: %5d steps, err %.2e * scale" % (width, lpr, deg, abs(lam[0] - w[0]) / scale))
            assert h.escape_method() == 1 and h.escape_info()[1], (width, lpr)
            assert abs(lam[0] - w[0]) <= 1e-9 * scale, (width, lpr)
            # (the vector at the bound of a warm call: what tells this instance's gather from a conjugated one, whose vector is
            # conj(v) with the same lambda_min)
            assert np.linalg.norm(S @ V[:, 0] - lam[0] * V[:, 0]) <= 2e-2 * scale, (width, lpr)
    finally:
        h.close()


# ------------------------------------------------------------------ 3. at a saddle
def _saddle(lib, storage, n, method=2):
    """The handle at the point trustregions() reaches from table_point(n, 2) with the solver's defaults (40 iterations, 100
    inner, gradient norm 1e-8): a rank-2 stationary point, a saddle on the instances below."""
    C = HR.instance(storage, n)
    h = lib.Handle.onlyunitdiag_hermitian(C)
    h.set_option("escape_method", method)
    h.set_point(HR.table_point(n, 2))
    h.rtr(lib.default_opts(maxiter=40, maxinner=100, tolgradnorm=1e-8))
    return C, h


@pytest.mark.parametrize("storage,n", [("grid", 1031), ("hub", 257), ("hub", 1031)])
def test_block_escape_at_a_saddle(lib, storage, n):
    C, h = _saddle(lib, storage, n)
    try:
        S, w = _reference(C, h)
        scale = max(abs(w[0]), abs(w[-1]))
        nneg = int(np.sum(w < -1e-7 * scale))
        print("%s %d: %d eigenvalues below -1e-7 * scale, lambda_min %.3e" % (storage, n, nneg, w[0]))
        assert nneg >= 1, "precondition: the point is a saddle"
        _warm_call(h, S, w, 8)
        _warm_call(h, S, w, 8)                                  # warm: the first call's vectors in the start block
        _cold_check(h, w)
    finally:
        h.close()


# ------------------------------------------------------------------ 4. both paths agree
def test_block_and_lanczos_paths_agree(lib):
    out = []
    for method in (1, 2):
        C, h = _saddle(lib, "grid", 1031, method)
        try:
            h.set_option("escape_deflate", 0); h.set_option("escape_warm", 0)
            lam, V, lmax, _ = h.escape_eigs(1, tol=1e-10, maxit=60000)
            assert h.escape_method() == method - 1
            out.append((lam[0], lmax))
        finally:
            h.close()
    print("lanczos", out[0], "block", out[1])
    assert abs(out[0][0] - out[1][0]) <= 1e-8 * out[0][1]
    assert abs(out[0][1] - out[1][1]) <= 1e-6 * out[0][1]


# ------------------------------------------------------------------ 5. bookkeeping
def test_budget_exhausted_is_reported(lib):
    """64 filter steps at the saddle of ("hub", 1031), ten negative eigenvalues at the bottom of a spectrum of width 27: a tenth
    of what the regular call above spends for 2 % (at a table point the bottom eigenvalue stands alone -- -16.3 against -12.5
    -- and 64 steps do reach 1e-13)."""
    C, h = _saddle(lib, "hub", 1031)
    try:
        h.set_option("escape_deflate", 0); h.set_option("escape_warm", 0)
        h.escape_eigs(8, tol=1e-13, maxit=64)
        nvalid, conv, res = h.escape_info()
        assert h.escape_method() == 1 and not conv
        assert h.escape_lower_bound() == -np.inf
    finally:
        h.close()


def test_small_orders_and_the_default_stay_on_lanczos(lib):
    for n, method, want in ((203, 2, 0), (1031, 0, 0), (1031, 1, 0), (1031, 2, 1)):
        h = lib.Handle.onlyunitdiag_hermitian(HR.instance("grid", n))
        try:
            h.set_option("escape_method", method)
            h.set_point(HR.table_point(n, 3))
            lam, V, lmax, _ = h.escape_eigs(2, tol=1e-9, maxit=2000)
            assert h.escape_method() == want, (n, method)
            assert V.shape == (n, 2) and np.isfinite(lam[0])
        finally:
            h.close()


def test_too_many_pairs_are_refused_by_name(lib):
    h = lib.Handle.onlyunitdiag_hermitian(HR.instance("grid", 1031))
    try:
        h.set_option("escape_method", 2)
        h.set_point(HR.table_point(1031, 3))
        with pytest.raises(lib.MsdpError, match="56 eigenpairs per call for a Hermitian") as e:
            h.escape_eigs(57, tol=1e-9, maxit=2000)
        assert e.value.code == lib.EINVAL
        lam, V, _, _ = h.escape_eigs(2, tol=1e-9, maxit=60000)  # the handle still works
        assert h.escape_method() == 1 and h.escape_info()[1]
    finally:
        h.close()


def test_ritz_stages_of_a_complex_panel_run_on_the_host(lib):
    h = lib.Handle.onlyunitdiag_hermitian(HR.instance("hub", 257))
    try:
        h.set_option("escape_method", 2); h.set_option("escape_rr", 1)
        h.set_point(HR.table_point(257, 3))
        h.escape_eigs(4, tol=1e-9, maxit=60000)
        assert h.escape_method() == 1 and h.escape_info()[1]
        dev, host, fallback = h.ritz_stages()
        assert dev == 0 and fallback == 0 and host >= 2
    finally:
        h.close()


# ------------------------------------------------------------------ 6. whole solves
@pytest.mark.parametrize("factor", ["host", "device"])
@pytest.mark.parametrize("n,sigma", [(203, 3.0), (1031, 4.0)])
def test_phase_synchronization_solve_with_the_block_escape(lib, n, sigma, factor):
    """The two phase-synchronisation instances of tests/test_gpu_hermitian.py with options["escape_method"] = 2: n = 203 stays on
    Lanczos (below the limit), n = 1031 takes the block route; the optimum is the restatement's."""
    from manisdp_matlab_amd import solvers
    from test_gpu_hermitian import _sync_instance
    m = _sync_instance(n, sigma)
    Y0p, obj_r, data_r = m["ref"][2]
    Y, obj, data = solvers.ManiSDP_onlyunitdiag(m["C"], {"Y0": Y0p, "eig": "device", "escape_method": 2, "hermitian_factor": factor},
                                                verbose=False)
    print("phase sync n %d (%s factor): %.10f, restatement %.10f; %d iterations, p %d, escape method %d"
          % (n, factor, obj, obj_r, data["iters"], data["p"], data["escape_method"]))
    assert data["status"] == 0 and data["dinf"] < 1e-8
    assert abs(obj - obj_r) < 1e-6 * abs(obj_r)
    if n == 1031:
        assert abs(obj + 19611.84035) < 1e-6 * 19611.84035
    assert data["escape_method"] == (1 if n == 1031 else 0)
    assert Y.dtype == np.complex128
