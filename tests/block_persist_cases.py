"""The cases of the block kinds' persistent tCG tests (option "block_persist", msdp_blockpersist.hip): shared by
tests/test_block_persist_cases_host.py, which shows on the CPU that the restatement's counts on every case do not move under
1e-14 perturbations of the start, and tests/test_gpu_block_persist.py, which holds both device paths to them.

A case is (kind, n, d, p): kind "stiefel" = the unit-block-diagonal problem (tests/blockdiag_ref.py), "pose" = the pose-graph
problem (tests/posegraph_ref.py); the start is point(n, d, p, seed) of the kind with the seed of SEEDS (0 unless the case with
seed 0 sat on the edge of a decision), the budget one trustregions() call of MAXITER iterations of up to MAXINNER inner steps."""
import numpy as np

import blockdiag_ref as BD
import posegraph_ref as PG

SHAPES = ((67, 3), (101, 2), (343, 3))
MAXITER, MAXINNER, TOLGRADNORM = 3, 20, 1e-9
# degree and noise per shape: those of the kinds' own device tests
STIEFEL_INSTANCE = {(67, 3): dict(degree=2, sigma=1.0, diag=False), (101, 2): dict(degree=6, sigma=1.0, diag=False),
                    (343, 3): dict(degree=6, sigma=1.0, diag=True)}
POSE_INSTANCE = {(67, 3): dict(degree=6, sigma=0.3), (101, 2): dict(degree=6, sigma=0.3), (343, 3): dict(degree=6, sigma=0.3)}
# (kind, n, d, p) -> seed of the start, where seed 0 is not stable under the perturbations
SEEDS = {}


# Beyond the sweep: budgets that reach the inner loop's convergence test (the sweep's three iterations from a random point all
# end on the trust-region boundary or on negative curvature after one to six inner steps): (kind, n, d, p, maxiter).  The first
# three and the fourth end on stop 3, the last runs 166 inner steps over 16 iterations, two of them rejected.
LONG_CASES = (("stiefel", 101, 2, 9, 8), ("stiefel", 343, 3, 32, 8), ("stiefel", 343, 3, 17, 11), ("pose", 101, 2, 9, 13),
              ("pose", 343, 3, 17, 16))


def widths(d):
    """Every lanes-per-block instance (ld = 2, 4, 6 .. 8, 10 .. 16, 18 .. 32) and both sides of each boundary."""
    return sorted({d, 5, 8, 9, 16, 17, 32})


def cases():
    return [(kind, n, d, p) for kind in ("stiefel", "pose") for (n, d) in SHAPES for p in widths(d)]


def ref(kind):
    return BD if kind == "stiefel" else PG


def matrix(kind, n, d):
    if kind == "stiefel":
        o = STIEFEL_INSTANCE[(n, d)]
        return BD.instance(n, d, o["degree"], o["sigma"], diag=o["diag"])[0]
    o = POSE_INSTANCE[(n, d)]
    return PG.instance(n, d, o["degree"], o["sigma"])[0]


def start(kind, n, d, p):
    return ref(kind).point(n, d, p, SEEDS.get((kind, n, d, p), 0))


_REF = {}


def restatement(kind, n, d, p, maxiter=MAXITER):
    """(Y, f, info) of the restatement's trustregions() on the case, computed once."""
    key = (kind, n, d, p, maxiter)
    if key not in _REF:
        _REF[key] = ref(kind).trustregions(matrix(kind, n, d), start(kind, n, d, p), d, maxiter, MAXINNER, TOLGRADNORM)
    return _REF[key]


def counts(info):
    return (info.iters, info.hessvecs, info.accepted, info.rejected, info.stop_inner[-1] if info.stop_inner else 0)


def perturbed(kind, Y0, d, rng):
    return ref(kind).polar_blocks(Y0 * (1.0 + 1e-14 * rng.standard_normal(Y0.shape)), d)
