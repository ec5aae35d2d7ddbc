"""GPU tests of the device Rayleigh-Ritz stage of the block eigen-solver (option escape_rr = 1; k_be_ritz in msdp_beritz.hip,
k_be_res_sum in msdp_blockeig.hip).

The kernel alone (msdp_debug_ritz_device) against scipy.linalg.eigh(H, G) under the bounds tests/test_blockeig_host.py sets for
the host stage on the same inputs; its three ways out (ok, hand the stage back to the host, breakdown); bit-reproducibility.
Then the stage inside the escape: against LAPACK on the dual slack of a toroidal grid under the bounds of
tests/test_gpu_blockeig.py, against the host stage on the same point, through a whole solve pinned by a README value, and on a
start block with dependent columns, which the kernel must hand back."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

from conftest import golden_path, within_print

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _sym(M):
    return 0.5 * (M + M.T)


def _check_ritz(lib, G, H, orthonormal=False):
    """The bounds of test_ritz_matches_generalised_eigh; (XW)'S(XW) of that test is W'HW here (H = X'SX)."""
    b = G.shape[0]
    th, W, rank, status = lib.ritz_device(G, H)
    assert status == 0 and rank == b
    wl = sla.eigh(_sym(H), _sym(G), eigvals_only=True)
    top = np.abs(wl).max()
    assert np.all(np.diff(th) >= 0)
    assert np.abs(th - wl).max() <= 1e-9 * top
    assert np.abs(W.T @ G @ W - np.eye(b)).max() <= 1e-8
    assert np.abs(W.T @ _sym(H) @ W - np.diag(th)).max() <= 1e-8 * top
    if orthonormal:
        assert np.abs(W.T @ W - np.eye(b)).max() <= 1e-8
    return th, W


def _generalised(b, cond):
    """The input of tests/test_blockeig_host.py::test_ritz_matches_generalised_eigh."""
    rng = np.random.default_rng(b)
    n = 4 * b
    S = rng.standard_normal((n, n)); S = S + S.T
    X = rng.standard_normal((n, b)) @ np.diag(np.logspace(0, np.log10(cond) / 2, b))
    return X, S, X.T @ X, X.T @ S @ X


@pytest.mark.parametrize("b,cond", [(32, 1e2), (64, 1e6)])
def test_kernel_matches_generalised_eigh(lib, b, cond):
    X, S, G, H = _generalised(b, cond)
    th, W = _check_ritz(lib, G, H)
    wl = sla.eigh(_sym(H), _sym(G), eigvals_only=True)
    Xr = X @ W                                                  # Ritz vectors: orthonormal, S-orthogonal
    assert np.abs(Xr.T @ S @ Xr - np.diag(th)).max() <= 1e-8 * np.abs(wl).max()


def test_kernel_on_the_warm_shape(lib):
    """What every stage after the first sees: the panel holds filtered Ritz vectors, G is the identity and H diagonal to rounding."""
    b = 64
    rng = np.random.default_rng(11)
    G = np.eye(b) + 1e-8 * _sym(rng.standard_normal((b, b)))
    H = np.diag(np.sort(rng.standard_normal(b))) + 1e-6 * _sym(rng.standard_normal((b, b)))
    _check_ritz(lib, G, H)


_FIVE = np.r_[-np.ones(5), np.linspace(0.5, 3.0, 27)]
_SPECTRA = {
    "five copies of -1": _FIVE,
    "eight values 1e-7 apart": np.r_[1.0 + 1e-7 * np.arange(8), np.linspace(2.0, 5.0, 24)],
    "all equal": 2.0 * np.ones(32),
    "all zero": np.zeros(32),
    "five copies, scaled 1e-6": 1e-6 * _FIVE,
    "five copies, scaled 1e6": 1e6 * _FIVE,
}


@pytest.mark.parametrize("name", sorted(_SPECTRA))
def test_kernel_on_multiple_and_degenerate_spectra(lib, name):
    b = 32
    lam = _SPECTRA[name]
    Q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((b, b)))
    H = Q.T @ np.diag(lam) @ Q
    th, _ = _check_ritz(lib, np.eye(b), H, orthonormal=True)   # (status 0 also for H = 0: an empty spectrum is no breakdown)
    assert np.abs(th - np.sort(lam)).max() <= 1e-9 * np.abs(lam).max()      # (H carries its spectrum to a few eps |lam|_max)


def _dependent():
    """The input of tests/test_blockeig_host.py::test_ritz_drops_dependent_columns."""
    rng = np.random.default_rng(7)
    b, n = 32, 200
    S = rng.standard_normal((n, n)); S = S + S.T
    X = rng.standard_normal((n, b))
    X[:, 20:24] = X[:, :4] @ rng.standard_normal((4, 4))          # four dependent columns
    return X.T @ X, X.T @ S @ X


def test_kernel_hands_dependent_columns_back(lib):
    G, H = _dependent()
    th, W, rank, status = lib.ritz_device(G, H)
    assert status == 1
    assert rank == 0 and not th.any() and not W.any()


@pytest.mark.parametrize("where", [(0, 0), (5, 17)])
def test_kernel_reports_a_breakdown(lib, where):
    """Non-finite data: status 2, and the kernel returns (every loop of it is bounded)."""
    _, _, G, H = _generalised(32, 1e2)
    G = G.copy()
    G[where] = np.nan
    G[where[::-1]] = np.nan
    th, W, rank, status = lib.ritz_device(G, H)
    assert status == 2
    th, W, rank, status = lib.ritz_device(np.zeros((32, 32)), H)    # max diag G = 0
    assert status == 2


def test_kernel_is_reproducible(lib):
    _, _, G, H = _generalised(64, 1e6)
    th1, W1, _, s1 = lib.ritz_device(G, H)
    th2, W2, _, s2 = lib.ritz_device(G, H)
    assert s1 == 0 and s2 == 0
    assert th1.tobytes() == th2.tobytes() and W1.tobytes() == W2.tobytes()


def test_unsupported_width_and_bad_option_value(lib):
    from manisdp_matlab_amd import problems
    with pytest.raises(lib.MsdpError, match=r"error -6: debug_ritz_device: block widths 32 and 64"):
        lib.ritz_device(np.eye(16), np.eye(16))
    h = lib.Handle.onlyunitdiag(problems.toroidal_grid_maxcut(8, 8, seed=1))
    with pytest.raises(lib.MsdpError, match=r"error -1: escape_rr: 0 host, 1 device"):
        h.set_option("escape_rr", 2)
    assert h.ritz_stages() == (0, 0, 0)
    h.close()


# ---------------------------------------------------------------------------------------------------- the stage inside the escape
def _check_pairs(S, w, lam, V, lmax, k, tol_val, tol_res):
    """tests/test_gpu_blockeig.py::_check_pairs and its bounds."""
    scale = max(abs(w[0]), abs(w[-1]))
    assert abs(lmax - w[-1]) <= 1e-6 * scale
    assert abs(lam[0] - w[0]) <= tol_val * scale
    for t in range(k):
        if lam[t] < -1e-9 * scale or t == 0:
            v = V[:, t]
            assert abs(np.linalg.norm(v) - 1.0) < 1e-8
            assert np.min(np.abs(w - lam[t])) <= 10 * tol_val * scale
            assert np.linalg.norm(S @ v - lam[t] * v) <= tol_res * scale
    # the returned values are the BOTTOM of the spectrum, in order
    assert np.all(np.diff(lam[np.isfinite(lam)]) >= -1e-12 * scale)
    nneg = int(np.sum(w < -1e-7 * scale))
    assert int(np.sum(lam < -1e-7 * scale)) == min(nneg, k)


def _reference(C, h):
    S = C - sp.diags(h.get_z())
    return S, np.linalg.eigvalsh(S.toarray())


@pytest.mark.parametrize("p", [6, 60])
def test_device_stage_through_the_escape_matches_lapack(lib, p):
    """The flow of test_block_escape_matches_lapack_on_a_grid with escape_rr = 1: a random point, a near-stationary one, the
    cold-started check.  p = 6 runs on a 64-wide panel (every stage on the device or handed back, none on the host by choice).
    With p = 60 the two regular calls take the 128-wide panel, where the option must change nothing: every stage of theirs on the
    host.  The cold check holds no column of Y, so it runs on a 64-wide panel whatever p is, on the device again: the stages are
    counted in front of it and behind it."""
    from manisdp_matlab_amd import problems
    C = problems.toroidal_grid_maxcut(60, 100, seed=9)
    n = C.shape[0]
    rng = np.random.default_rng(p)
    Y = rng.standard_normal((n, p)); Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    h = lib.Handle.onlyunitdiag(C, pcap=64)
    h.set_option("escape_rr", 1)
    h.set_point(Y)
    S, w = _reference(C, h)
    lam, V, lmax, _ = h.escape_eigs(8, tol=1e-9, maxit=60000)
    assert h.escape_method() == 1
    nvalid, conv, _ = h.escape_info()
    assert conv and nvalid == 8
    _check_pairs(S, w, lam, V, lmax, 8, 2e-3, 2e-2)
    h.rtr(lib.default_opts(maxiter=60, maxinner=200, tolgradnorm=1e-9))
    S, w = _reference(C, h)
    lam, V, lmax, _ = h.escape_eigs(8, tol=1e-9, maxit=60000)
    assert h.escape_method() == 1 and h.escape_info()[1]
    _check_pairs(S, w, lam, V, lmax, 8, 2e-3, 2e-2)
    device, host, fallback = h.ritz_stages()
    if p == 6:
        assert device > 0 and host == 0
    else:
        assert device == 0 and host > 0 and fallback == 0
    h.set_option("escape_deflate", 0); h.set_option("escape_warm", 0); h.set_option("escape_start_y", 0)
    lam1, V1, _, _ = h.escape_eigs(1, tol=1e-9, maxit=60000)
    assert h.escape_method() == 1 and h.escape_info()[1]
    scale = max(abs(w[0]), abs(w[-1]))
    assert abs(lam1[0] - w[0]) <= 1e-9 * scale
    assert np.linalg.norm(S @ V1[:, 0] - lam1[0] * V1[:, 0]) <= 1e-5 * scale
    lb = h.escape_lower_bound()
    assert np.isfinite(lb) and lb <= lam1[0] and lam1[0] - lb <= 1e-8 * scale
    device1, host1, _ = h.ritz_stages()
    assert device1 > device and host1 == host                  # hashed noise on 64 columns: nothing to hand back
    h.close()


def _near_stationary(lib, C, Y, escape_rr):
    h = lib.Handle.onlyunitdiag(C)
    h.set_option("escape_rr", escape_rr)
    h.set_point(Y)
    h.rtr(lib.default_opts(maxiter=40, maxinner=100, tolgradnorm=1e-8))
    h.set_option("escape_deflate", 0); h.set_option("escape_warm", 0)
    return h


def test_host_and_device_stages_agree(lib):
    """The cold check of test_block_and_lanczos_paths_agree under both settings of escape_rr: same lambda_min."""
    from manisdp_matlab_amd import problems
    C = problems.toroidal_grid_maxcut(50, 80, seed=2)
    n, p = C.shape[0], 12
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((n, p)); Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    out = []
    for escape_rr in (0, 1):
        h = _near_stationary(lib, C, Y, escape_rr)
        lam, _, lmax, _ = h.escape_eigs(1, tol=1e-10, maxit=60000)
        assert h.escape_method() == 1 and h.escape_info()[1]
        device, host, fallback = h.ritz_stages()
        assert (device > 0 and host == 0) if escape_rr else (device == 0 and host > 0 and fallback == 0)
        out.append((lam[0], lmax))
        h.close()
    assert abs(out[0][0] - out[1][0]) <= 1e-8 * out[0][1]


def test_dependent_start_block_falls_back_and_converges(lib):
    """A factor whose last four columns repeat its first four, put into the start block of a cold call (escape_start_y = 1): the
    Gram matrix of the first stage is singular, the kernel hands the stage back, the host stage drops the dependent directions and
    refills them with noise, and the call converges as it does with the host stage throughout."""
    from manisdp_matlab_amd import problems
    C = problems.toroidal_grid_maxcut(50, 80, seed=2)
    n, p = C.shape[0], 12
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((n, p))
    Y[:, 8:] = Y[:, :4]
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    out = []
    for escape_rr in (0, 1):
        h = lib.Handle.onlyunitdiag(C)
        h.set_option("escape_rr", escape_rr)
        h.set_point(Y)
        h.set_option("escape_deflate", 0); h.set_option("escape_warm", 0); h.set_option("escape_start_y", 1)
        lam, _, lmax, _ = h.escape_eigs(1, tol=1e-10, maxit=60000)
        assert h.escape_method() == 1 and h.escape_info()[1]
        device, host, fallback = h.ritz_stages()
        if escape_rr:
            assert fallback >= 1 and device > 0 and host == 0
        out.append((lam[0], lmax))
        h.close()
    assert abs(out[0][0] - out[1][0]) <= 1e-8 * out[0][1]


def test_pinned_optimum_with_the_device_stage():
    """Gset G32 against the value the reference's README prints, block eigen-solver forced (n = 2000), device stage on."""
    import json
    from manisdp_matlab_amd import problems, solvers
    printed = json.load(open(golden_path("known_answers_printed.json")))
    C = problems.maxcut_cost_matrix(golden_path("G32.txt.gz"))
    Y, obj, data = solvers.ManiSDP_onlyunitdiag(C, {"eig": "device", "escape_method": 2, "escape_rr": "device"}, verbose=False)
    assert data["status"] == 0 and data["dinf"] < 1e-8
    assert within_print(-obj, printed["maxG32"])
    assert data["escape_rr_stages"][0] > 0
