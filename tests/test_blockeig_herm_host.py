"""Host-side Rayleigh-Ritz stage of the block eigen-solver's complex panel (be_ritz_herm in
manisdp-matlab_amd/csrc/msdp_blockeig.hip, through msdp_debug_ritz_herm) against LAPACK's generalised Hermitian solver.
CPU only: the entry point runs no device code.

Tolerances are those of tests/test_blockeig_host.py for the same quantities of the real stage: theta to 1e-9 of the largest
|theta|, W^H G W = I to 1e-8, W^H H W = diag(theta) to 1e-8 of the largest |theta| (1e-9 on both where the eigen-basis route
drops dependent columns)."""
import numpy as np
import pytest
import scipy.linalg as sla

from manisdp_matlab_amd import _lib

BC = [16, 32, 64]


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _pencil(rng, lam):
    """(G, H) with G = B^H B, H = B^H diag(lam) B for a random complex B: the eigenvalues of H c = theta G c are lam."""
    bc = len(lam)
    B = _crandn(rng, bc, bc) / np.sqrt(2 * bc) + np.eye(bc)
    return B.conj().T @ B, B.conj().T @ (np.asarray(lam)[:, None] * B)


def _check(G, H, theta, W, r, tol_val=1e-9, tol_orth=1e-8):
    bc = G.shape[0]
    Gh, Hh = 0.5 * (G + G.conj().T), 0.5 * (H + H.conj().T)
    assert np.all(np.diff(theta[:r]) >= 0)
    assert np.all(np.isinf(theta[r:])) and np.all(W[:, r:] == 0.0)
    Wr = W[:, :r]
    scale = np.abs(theta[:r]).max()
    assert np.abs(Wr.conj().T @ Gh @ Wr - np.eye(r)).max() <= tol_orth
    assert np.abs(Wr.conj().T @ Hh @ Wr - np.diag(theta[:r])).max() <= tol_orth * scale
    if r == bc:
        wl = sla.eigh(Hh, Gh, eigvals_only=True)
        assert np.abs(theta - wl).max() <= tol_val * np.abs(wl).max()


@pytest.mark.parametrize("bc,cond", [(16, 1e2), (32, 1e6), (64, 1e3)])
def test_ritz_herm_matches_generalised_eigh(bc, cond):
    rng = np.random.default_rng(bc)
    n = 4 * bc
    S = _crandn(rng, n, n); S = S + S.conj().T
    X = _crandn(rng, n, bc) @ np.diag(np.logspace(0, np.log10(cond) / 2, bc))
    G, H = X.conj().T @ X, X.conj().T @ S @ X
    theta, W, r = _lib.ritz_herm(G, H)
    assert r == bc
    _check(G, H, theta, W, r)
    Xr = X @ W                                            # Ritz vectors: orthonormal, S-orthogonal in the complex inner product
    assert np.abs(Xr.conj().T @ Xr - np.eye(bc)).max() <= 1e-8
    assert np.abs(Xr.conj().T @ S @ Xr - np.diag(theta)).max() <= 1e-8 * np.abs(theta).max()


@pytest.mark.parametrize("bc", BC)
def test_ritz_herm_double_and_triple_eigenvalue(bc):
    """Every complex direction once: a double and a triple eigenvalue come back with their multiplicity and an orthonormal
    basis (on the real view each would appear twice as often)."""
    rng = np.random.default_rng(100 + bc)
    lam = np.sort(rng.uniform(-1.0, 1.0, bc))
    lam[1] = lam[2] = -1.25
    lam[5] = lam[6] = lam[7] = 0.375
    lam = np.sort(lam)
    G, H = _pencil(rng, lam)
    theta, W, r = _lib.ritz_herm(G, H)
    assert r == bc
    _check(G, H, theta, W, r)
    assert np.abs(theta - lam).max() <= 1e-9 * np.abs(lam).max()
    assert int(np.sum(np.abs(theta + 1.25) < 1e-9)) == 2 and int(np.sum(np.abs(theta - 0.375) < 1e-9)) == 3


@pytest.mark.parametrize("bc", BC)
def test_ritz_herm_cluster_at_the_bottom(bc):
    """Twelve eigenvalues within 1e-8 of the bottom of a spectrum of width 2: the bottom of S at a near-stationary point."""
    rng = np.random.default_rng(200 + bc)
    lam = np.sort(np.r_[-1.0 + 1e-8 * rng.uniform(0.0, 1.0, 12), rng.uniform(-0.9, 1.0, bc - 13), 1.0])
    G, H = _pencil(rng, lam)
    theta, W, r = _lib.ritz_herm(G, H)
    assert r == bc
    _check(G, H, theta, W, r)
    assert np.abs(theta - lam).max() <= 1e-9 * np.abs(lam).max()
    assert int(np.sum(theta < -1.0 + 1e-7)) == 12


@pytest.mark.parametrize("bc", BC)
def test_ritz_herm_drops_dependent_columns(bc):
    """G of rank bc - 5: the Cholesky route gives way to the eigen-basis of G, the dropped directions come back as +inf / zero
    columns, and the kept ones are the Ritz pairs of the spanned subspace."""
    rng = np.random.default_rng(300 + bc)
    n = 6 * bc
    S = _crandn(rng, n, n); S = S + S.conj().T
    X = _crandn(rng, n, bc)
    X[:, bc - 5:] = X[:, :5] @ _crandn(rng, 5, 5)        # five dependent columns
    G, H = X.conj().T @ X, X.conj().T @ S @ X
    theta, W, r = _lib.ritz_herm(G, H)
    assert r == bc - 5
    _check(G, H, theta, W, r, tol_orth=1e-9)
    Q, _ = np.linalg.qr(X[:, :bc - 5])
    wl = np.linalg.eigvalsh(Q.conj().T @ S @ Q)
    assert np.abs(theta[:r] - wl).max() <= 1e-9 * np.abs(wl).max()
    Xr = X @ W[:, :r]
    assert np.abs(Xr.conj().T @ Xr - np.eye(r)).max() <= 1e-9
