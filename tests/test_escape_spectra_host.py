"""CPU tests of tests/escape_spectra_ref.py, the constructed-spectrum matrices for the saddle escape: the prescribed spectrum IS
the spectrum of what build() returns (LAPACK as a second opinion, to 1e-12 * scale: four digits below the 1e-8 * scale the escape
tests ask of lambda_min), the returned columns are its eigenvectors, and sparse_copies() has the multiplicities it claims."""
import numpy as np
import pytest

import escape_spectra_ref as R

N = 200


@pytest.mark.parametrize("name", R.CATALOGUE)
def test_build_reproduces_the_prescribed_spectrum(name):
    lam = R.spectrum(name, N)
    assert lam.shape == (N,) and np.all(np.diff(lam) >= 0)
    S, w, U = R.build(N, lam, seed=11)
    scale = np.abs(lam).max()
    assert np.array_equal(w, lam)
    assert np.array_equal(S, S.T)                                           # exactly symmetric
    assert np.abs(np.linalg.eigvalsh(S) - lam).max() <= 1e-12 * scale
    assert np.abs(S @ U - U * lam).max() <= 1e-12 * scale                   # S (H e_i) = lam_i H e_i
    assert np.linalg.norm(S @ U - U * lam, axis=0).max() <= 1e-12 * scale
    assert np.abs(U.T @ U - np.eye(N)).max() <= 1e-14


def test_catalogue_entries_hold_what_their_names_say():
    sp = lambda name: R.spectrum(name, N)
    assert sp("posdef")[0] == 1.0 and sp("posdef")[-1] == 2.0
    assert sp("negdef")[0] == -2.0 and sp("negdef")[-1] == -1.0
    assert np.sum(sp("mult5") == -1.0) == 5 and sp("mult5")[5] == 1.0
    assert np.sum(sp("mult12") == -1.0) == 12 and sp("mult12")[12] == 1.0
    assert np.allclose(np.diff(sp("cluster")[:8]), 1e-7, rtol=1e-6, atol=0) and sp("cluster")[8] == 0.5
    assert np.all(np.diff(sp("cluster_tight")[:8]) > 0) and sp("cluster_tight")[7] - sp("cluster_tight")[0] < 1e-10
    assert sorted(set(sp("three_distinct"))) == [-1.0, 0.0, 3.0] and np.sum(sp("three_distinct") == -1.0) == N // 3
    assert np.all(sp("scalar") == 2.0) and np.all(sp("zero") == 0.0)
    assert np.sum(sp("kernel_psd") == 0.0) == 10 and sp("kernel_psd")[10] == 1e-3 and sp("kernel_psd")[0] == 0.0
    kh = sp("kernel_hidden")
    assert kh[0] == -1e-6 and np.sum(kh == 0.0) == 10 and np.sum(kh < 0) == 1 and abs(kh[-1] - 1.0) < 1e-15
    assert sp("shift_pos")[0] == 100.0 and abs(sp("shift_pos")[-1] - 100.1) < 1e-13
    assert abs(sp("shift_neg")[0] + 100.1) < 1e-13 and sp("shift_neg")[-1] == -100.0
    assert np.allclose(sp("graded")[:10], -(10.0 ** -np.arange(10)), rtol=1e-15, atol=0)
    assert np.array_equal(sp("tiny"), 1e-6 * sp("mult5")) and np.array_equal(sp("huge"), 1e6 * sp("mult5"))


@pytest.mark.parametrize("name", R.CATALOGUE)
def test_smallest_orders(name):
    n = R.MIN_ORDER[name]
    lam = R.spectrum(name, n)
    S, w, U = R.build(n, lam, seed=3, ncols=4)
    assert U.shape == (n, min(4, n))
    assert np.abs(np.linalg.eigvalsh(S) - lam).max() <= 1e-12 * np.abs(lam).max()
    with pytest.raises(ValueError):
        R.spectrum(name, n - 1)


@pytest.mark.parametrize("base", ["cycle", "torus"])
@pytest.mark.parametrize("t", [8, 12])
def test_sparse_copies_have_the_multiplicities_they_claim(base, t):
    C, w = R.sparse_copies(t, base, seed=5)
    n = C.shape[0]
    assert 40 <= n // t <= 60 and n == t * (n // t)
    Cd = C.toarray()
    assert np.array_equal(Cd, Cd.T)
    for sign in (1.0, -1.0):
        S = sign * (Cd - np.diag(Cd.sum(axis=1)))          # Y = all rows e_1: z = (C*1), S = C - diag(z)
        ws = np.sort(sign * w)
        scale = np.abs(ws).max()
        assert np.abs(np.linalg.eigvalsh(S) - ws).max() <= 1e-12 * scale
        assert np.abs(S @ np.ones(n)).max() <= 1e-14 * scale
        # every distinct eigenvalue of one copy (separated by more than 1e-6 * scale) appears exactly t times; the kernel too
        wb = ws[::t]
        assert np.all(np.diff(wb) > 1e-6 * scale)
        for x in wb:
            assert int(np.sum(np.abs(ws - x) <= 1e-12 * scale)) == t
        assert int(np.sum(np.abs(ws) <= 1e-12 * scale)) == t
