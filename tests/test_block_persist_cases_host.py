"""CPU condition on the inputs of tests/test_gpu_block_persist.py (tests/block_persist_cases.py): on every case the counts of
the NumPy restatement's trustregions() do not change when the start is perturbed by 1e-14 relative in five random directions,
so that the summation order of a device path cannot change them; and the cases reach both families of inner stops."""
import numpy as np
import pytest

import block_persist_cases as K


def _stable(kind, n, d, p, maxiter):
    _, f0, i0 = K.restatement(kind, n, d, p, maxiter)
    C, Y0 = K.matrix(kind, n, d), K.start(kind, n, d, p)
    g = np.random.default_rng(99)
    for _ in range(5):
        _, f1, i1 = K.ref(kind).trustregions(C, K.perturbed(kind, Y0, d, g), d, maxiter, K.MAXINNER, K.TOLGRADNORM)
        assert K.counts(i1) == K.counts(i0) and i1.numinner == i0.numinner, (kind, n, d, p, K.counts(i0), K.counts(i1))
        assert abs(f1 - f0) <= 1e-11 * abs(f0)
    return i0


@pytest.mark.parametrize("kind", ["stiefel", "pose"])
@pytest.mark.parametrize("n,d", K.SHAPES)
def test_sweep_cases_are_stable_under_perturbations_of_the_start(kind, n, d):
    for p in K.widths(d):
        i0 = _stable(kind, n, d, p, K.MAXITER)
        assert i0.iters == K.MAXITER and i0.hessvecs >= K.MAXITER


@pytest.mark.parametrize("case", K.LONG_CASES)
def test_long_cases_are_stable_under_perturbations_of_the_start(case):
    i0 = _stable(*case)
    assert i0.hessvecs >= 30


def test_cases_end_on_both_families_of_inner_stops():
    """A case that ends on the trust-region boundary or negative curvature (stop 1 or 2) and one that ends on the kappa / theta
    test (stop 3 or 4), for either kind."""
    for kind in ("stiefel", "pose"):
        last = {K.restatement(k, n, d, p)[2].stop_inner[-1] for (k, n, d, p) in K.cases() if k == kind}
        last |= {K.restatement(*c)[2].stop_inner[-1] for c in K.LONG_CASES if c[0] == kind}
        assert last & {1, 2} and last & {3, 4}, (kind, last)
