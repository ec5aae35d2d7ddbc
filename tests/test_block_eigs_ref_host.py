"""Host-only checks of the references and generators behind tests/test_gpu_block_eigs.py (block_eigs_ref.py): LAPACK against mpmath
at 40 digits on every matrix family, so that the GPU comparison measures msdp_block_eigs and not its reference; and the properties
the generators promise (planted negative counts, a bottom set that stops short of the whole block in families 1 to 4)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_eigs_ref as R  # noqa: E402

MP_ORDERS = {1: (33, 65, 129), 2: (33, 65), 3: (33, 65), 4: (33, 65), 6: (33, 65)}


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_lapack_stays_within_a_tenth_of_the_eigenvalue_tolerance(fam):
    """numpy.linalg.eigvalsh against mpmath.eigsy at 40 digits (closed forms and exact diagonals where a block has them): the error
    of LAPACK is at most one tenth of 1e-13 * n * scale on every case of the family that carries a 40-digit reference -- the dense
    families at orders 33 and 65 (family 1 also at 129), every structured block."""
    cases = [c for c in R.family_cases(fam, mp_orders=MP_ORDERS.get(fam, ())) if c.mp or c.closed is not None]
    assert cases
    if fam != 5:
        assert {c.n for c in cases} == set(MP_ORDERS[fam])
    worst = 0.0
    for c in cases:
        ratio = R.lapack_error_ratio(c)
        worst = max(worst, ratio)
        assert ratio <= 0.1, f"{c.name}: LAPACK uses {ratio:.3g} of the eigenvalue tolerance"
    print(f"\nfamily {fam}: {len(cases)} cases, LAPACK error at most {worst:.2e} of the tolerance")


@pytest.mark.parametrize("fam", [1, 2, 3, 4])
def test_generators_keep_the_subspace_check_meaningful(fam):
    """Families 1 to 4: for k = 8 and 9 the bottom set J (the k smallest eigenvalues and whatever lies within 1e-4 * scale above
    them) ends below the block's order with a gap of at least 1e-4 * scale, and family 2 has the planted number of negative
    eigenvalues."""
    for c in R.family_cases(fam):
        assert np.array_equal(c.S, c.S.T)
        wr = np.linalg.eigvalsh(c.S)
        scale = R.scale_of(wr)
        for k in (8, 9):
            j = R.bottom_set(wr, min(k, c.n), scale)
            assert j < c.n, c.name
            assert wr[j] - wr[j - 1] > R.CLUSTER_GAP * scale
        if c.nneg >= 0:
            assert int(np.sum(wr < 0)) == c.nneg, c.name
        if c.nzero:
            assert np.abs(wr[:c.nzero]).max() <= 1e-14 and wr[c.nzero] >= 0.5 - 1e-12, c.name


def test_check_block_rejects_wrong_results():
    """The assertions themselves: an exact eigen-decomposition passes; a shifted eigenvalue, a vector rotated out of the bottom
    eigenspace, a lost orthogonality and a wrong sign on a tiny eigenvalue each fail."""
    c = [c for c in R.family_cases(2, orders=[33]) if c.nneg == 3][0]
    w, Q = np.linalg.eigh(c.S)
    k = 8
    V = Q[:, :k].copy()
    assert R.check_block(c.S, w, V, k, nneg=3, vacuous_ok=False) is False
    with pytest.raises(AssertionError, match="eigenvalue error"):
        R.check_block(c.S, w + 1e-10, V, k)
    bad = w.copy(); bad[:3] = 1e-12
    with pytest.raises(AssertionError, match="eigenvalue error|negative eigenvalues"):
        R.check_block(c.S, bad, V, k, nneg=3)
    t = 1e-5
    Vb = V.copy(); Vb[:, 0] = np.cos(t) * Q[:, 0] + np.sin(t) * Q[:, 20]
    with pytest.raises(AssertionError, match="residual|outside"):
        R.check_block(c.S, w, Vb, k)
    Vb = V.copy(); Vb[:, 1] = (Q[:, 1] + 1e-9 * Q[:, 0]) / np.sqrt(1 + 1e-18)
    with pytest.raises(AssertionError, match="V'V"):
        R.check_block(c.S, w, Vb, k)
    # any orthonormal basis of a multiple eigenvalue passes: individual vectors inside it are not determined
    G, _ = np.linalg.qr(np.random.default_rng(0).standard_normal((3, 3)))
    Vb = V.copy(); Vb[:, :3] = Q[:, :3] @ G
    assert R.check_block(c.S, w, Vb, k, nneg=3, vacuous_ok=False) is False
