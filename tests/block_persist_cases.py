"""The cases of the block kinds' persistent tCG tests (option "block_persist", msdp_blockpersist.hip): shared by
tests/test_block_persist_cases_host.py, which shows on the CPU that the restatement's counts on every case do not move under
1e-14 perturbations of the start, and tests/test_gpu_block_persist.py and tests/test_gpu_block_persist_instances.py, which hold
both device paths to them.

A case is (kind, n, d, p): kind "stiefel" = the unit-block-diagonal problem (tests/blockdiag_ref.py), "pose" = the pose-graph
problem (tests/posegraph_ref.py); the start is point(n, d, p, seed) of the kind with the seed of SEEDS (0 unless the case with
seed 0 sat on the edge of a decision), the budget one trustregions() call of MAXITER iterations of up to MAXINNER inner steps.

The second half of the file restates the plan arithmetic of msdp_blockpersist_plan.h (plan, instance_of) and lists, with the
grid caps they run under, every case of the two device test files (gpu_runs): the ledger of the instances of
k_tcg_persist_blk<D, EF, LPR, R> that the suite reaches."""
import numpy as np
import scipy.sparse as sp

import blockdiag_ref as BD
import posegraph_ref as PG

SHAPES = ((67, 3), (101, 2), (343, 3))
MAXITER, MAXINNER, TOLGRADNORM = 3, 20, 1e-9
# degree and noise per shape: those of the kinds' own device tests; every other shape takes the DEFAULT_ ones
STIEFEL_INSTANCE = {(67, 3): dict(degree=2, sigma=1.0, diag=False), (101, 2): dict(degree=6, sigma=1.0, diag=False),
                    (343, 3): dict(degree=6, sigma=1.0, diag=True)}
POSE_INSTANCE = {(67, 3): dict(degree=6, sigma=0.3), (101, 2): dict(degree=6, sigma=0.3), (343, 3): dict(degree=6, sigma=0.3)}
DEFAULT_STIEFEL = dict(degree=6, sigma=1.0, diag=True)
DEFAULT_POSE = dict(degree=6, sigma=0.3)
# (kind, n, d, p) -> seed of the start, where seed 0 is not stable under the perturbations
# (pose, 2053, 2, 4): fourteen iterations from seed 0 move the cost by 3e-11 relative under the perturbations, from seed 1 by 1e-12
SEEDS = {("pose", 2053, 2, 4): 1}
KINDS = ("stiefel", "pose")


# Beyond the sweep: budgets that reach the inner loop's convergence test (the sweep's three iterations from a random point all
# end on the trust-region boundary or on negative curvature after one to six inner steps): (kind, n, d, p, maxiter).  The first
# three and the fourth end on stop 3, the last runs 166 inner steps over 16 iterations, two of them rejected.
LONG_CASES = (("stiefel", 101, 2, 9, 8), ("stiefel", 343, 3, 32, 8), ("stiefel", 343, 3, 17, 11), ("pose", 101, 2, 9, 13),
              ("pose", 343, 3, 17, 16))

# ------------------------------------------------------------------ two row slots
# (n, d) -> widths: with the grid capped at 8 every one of them takes two row slots (8 RSTEP < n <= 16 RSTEP), at the planned grid
# one.  Per lanes-per-block count: a second slot that holds one block or none (n = 16 RSTEP / 2 + 3 and the like), a half-full
# and a full one (n = 1024 at lpr 8: every lane group owns two blocks); both block orders.
TWO_SLOT_SHAPES = {(4099, 2): (2,), (6150, 2): (2,),                                    # lpr 1
                   (2053, 2): (4,), (2053, 3): (3,), (3080, 3): (4,),                   # lpr 2
                   (1031, 2): (8,), (1031, 3): (5,), (1540, 3): (8,),                   # lpr 4
                   (521, 2): (9,), (521, 3): (9,), (821, 3): (16,), (1024, 2): (16,),   # lpr 8
                   (389, 2): (17, 32)}                                                  # lpr 16 with D = 2
# long budgets on two slots: (kind, n, d, p, maxiter, grid cap); the last two run two slots on SIXTEEN workgroups
# (16 RSTEP < n <= 32 RSTEP), where the chunk order of msdp_chunk_rows is no longer the identity
# ((1031, 2, 8) takes a tenth iteration: nine are 29 Hess-vecs, one short of what a long case has to run; pose (521, 3, 17) stops
# after eleven: fourteen move its cost by 9e-11 relative under the perturbations of the host test, eleven by 1e-13)
LONG_TWO_SLOT_CASES = (("stiefel", 521, 2, 9, 9, 8), ("stiefel", 821, 3, 16, 9, 8), ("stiefel", 1031, 2, 8, 10, 8),
                       ("stiefel", 521, 3, 9, 9, 8), ("stiefel", 2053, 2, 4, 13, 8),
                       ("pose", 521, 2, 9, 14, 8), ("pose", 1031, 3, 5, 14, 8), ("pose", 2053, 3, 3, 14, 8),
                       ("pose", 4099, 2, 2, 14, 8), ("pose", 821, 3, 16, 14, 8), ("pose", 2053, 2, 4, 14, 8),
                       ("pose", 521, 3, 9, 14, 8),
                       ("pose", 521, 3, 17, 11, 16), ("stiefel", 1031, 2, 9, 9, 16))

# ------------------------------------------------------------------ the step itself
# one case per (kind, lpr, R), two at lpr 2: (n, d, p), run at the planned grid (one slot) and with the cap 8 (two slots), from
# start() and from the restatement's point after STEP_WARM iterations (test_block_persist_cases_host.py: that tCG runs five trips
# or more).  (2053, 2, 4) is here because the sweep's three iterations on it are tCGs of ONE trip for the Stiefel kind: without
# it the second half of a trip of <2, 0, 2, *> -- the new direction and its tangent step -- would run under no test.
STEP_SHAPES = ((4099, 2, 2), (2053, 3, 3), (2053, 2, 4), (1031, 3, 5), (521, 3, 9), (389, 2, 17))
# (the Stiefel kind at p = d runs its first iterations to the boundary in a trip or two: its warm starts lie deeper)
STEP_WARM = {("stiefel", 4099, 2, 2): 30, ("stiefel", 2053, 3, 3): 30, ("stiefel", 1031, 3, 5): 16, ("stiefel", 521, 3, 9): 8,
             ("stiefel", 389, 2, 17): 5, ("stiefel", 2053, 2, 4): 12, ("pose", 2053, 2, 4): 8,
             ("pose", 4099, 2, 2): 16, ("pose", 2053, 3, 3): 12, ("pose", 1031, 3, 5): 8,
             ("pose", 521, 3, 9): 8, ("pose", 389, 2, 17): 5}

# ------------------------------------------------------------------ trust-region options
OPTION_SHAPES = ((101, 2, 9), (343, 3, 17))
OPTION_MAXITER = {"stiefel": 8, "pose": 13}
# kappa, theta, mininner: stop 4 behind mininner; the pow branch; stop 3 at the length mininner; theta > 1
OPTION_SETS = (dict(kappa=1e6, theta=1.0, mininner=3), dict(kappa=0.1, theta=0.5, mininner=1),
               dict(kappa=0.5, theta=0.25, mininner=5), dict(kappa=1e-3, theta=2.0, mininner=1))

# ------------------------------------------------------------------ edges
# a solve the budget finishes: (kind, n, d, p, maxiter, tolgradnorm)
FINISHED_CASES = (("stiefel", 101, 2, 9, 40, 1e-2), ("pose", 101, 2, 9, 60, 1e-1))
# fewer blocks than the eight workgroups of the smallest grid, and one more
FEW_BLOCKS = (1, 5, 9)
# a cap that leaves no plan (n > 16 RSTEP at cap 8): (n, d, p)
CAP_TOO_SMALL = (521, 3, 17)
# whole blocks removed: (n, d, p) at the planned grid (one slot) and with the cap 8 (two)
MASKED_SHAPES = ((521, 2, 9), (521, 3, 9), (1031, 3, 5))


def widths(d):
    """Every lanes-per-block instance (ld = 2, 4, 6 .. 8, 10 .. 16, 18 .. 32) and both sides of each boundary."""
    return sorted({d, 5, 8, 9, 16, 17, 32})


def cases():
    return [(kind, n, d, p) for kind in KINDS for (n, d) in SHAPES for p in widths(d)]


def two_slot_cases():
    return [(kind, n, d, p) for kind in KINDS for (n, d), ps in TWO_SLOT_SHAPES.items() for p in ps]


def ref(kind):
    return BD if kind == "stiefel" else PG


def blk(kind, d):
    """Rows of a block: d, and the free row of the pose kind."""
    return d + (kind == "pose")


def small_instance(kind, n, d):
    """FEW_BLOCKS: the generators with the degree cut to what n blocks admit."""
    deg = min(6, n - 1)
    if kind == "stiefel":
        return BD.instance(n, d, deg, 1.0, diag=True)[0]
    return PG.instance(n, d, deg, 0.3)[0]


def matrix(kind, n, d):
    if n < 12:
        return small_instance(kind, n, d)
    if kind == "stiefel":
        o = STIEFEL_INSTANCE.get((n, d), DEFAULT_STIEFEL)
        return BD.instance(n, d, o["degree"], o["sigma"], diag=o["diag"])[0]
    o = POSE_INSTANCE.get((n, d), DEFAULT_POSE)
    return PG.instance(n, d, o["degree"], o["sigma"])[0]


def block_mask(n, seed=5):
    """MASKED_SHAPES: which blocks stay (about three quarters of them)."""
    return np.random.default_rng(seed).random(n) >= 0.25


def masked_matrix(kind, n, d):
    """matrix() with the rows and columns of the removed blocks zeroed, Dk C Dk: a principal submatrix padded with zeros, so it
    is bounded below where C is.  Removed blocks have an empty block row, their neighbours lose entries down to one or none."""
    key = ("masked", kind, n, d)
    if key not in _REF:
        keep = np.repeat(block_mask(n), blk(kind, d)).astype(np.float64)
        Dk = sp.diags(keep)
        Cz = sp.csr_matrix(Dk @ sp.csr_matrix(matrix(kind, n, d)) @ Dk)
        Cz.eliminate_zeros()
        Cz.sort_indices()
        _REF[key] = Cz
    return _REF[key]


def block_row_lengths(C, B):
    """Entries per block row of the block CSR form of C with blocks of B rows (what msdp_stiefel_setup builds)."""
    Cc = sp.coo_matrix(C)
    nb = C.shape[0] // B
    pat = sp.csr_matrix((np.ones(Cc.nnz), (Cc.row // B, Cc.col // B)), shape=(nb, nb))
    pat.sum_duplicates()
    return np.diff(pat.indptr)


def start(kind, n, d, p):
    return ref(kind).point(n, d, p, SEEDS.get((kind, n, d, p), 0))


_REF = {}


def problem(kind, C, n, d, p):
    return ref(kind).Problem(C, n, d, p)


def trustregions(kind, C, Y0, d, maxiter, tol=TOLGRADNORM, **opts):
    """manopt_rtr.trustregions on the kind's Problem with the file's inner cap; opts: kappa, theta, mininner."""
    from oracle import manopt_rtr
    n = Y0.shape[0] // blk(kind, d)
    return manopt_rtr.trustregions(problem(kind, C, n, d, Y0.shape[1]), np.array(Y0, dtype=np.float64), maxiter, MAXINNER, tol, **opts)


def restatement(kind, n, d, p, maxiter=MAXITER, tol=TOLGRADNORM, masked=False, **opts):
    """(Y, f, info) of the restatement's trustregions() on the case, computed once."""
    key = (kind, n, d, p, maxiter, tol, masked, tuple(sorted(opts.items())))
    if key not in _REF:
        C = masked_matrix(kind, n, d) if masked else matrix(kind, n, d)
        _REF[key] = trustregions(kind, C, start(kind, n, d, p), d, maxiter, tol, **opts)
    return _REF[key]


def warm_start(kind, n, d, p):
    """The restatement's point after STEP_WARM iterations from start(): from there the first tCG runs to its convergence test,
    not to the trust-region boundary after a trip or two."""
    return np.ascontiguousarray(restatement(kind, n, d, p, STEP_WARM[(kind, n, d, p)])[0])


def first_step(kind, n, d, p, warm, Y=None):
    """(eta, Heta, trips, stop) of the first tCG of a trustregions() call at start() or warm_start() (or at Y): the gradient
    and the radius Delta0 = typicaldist / 8 as trustregions() takes them (trustregions.m:363-372, :405-409)."""
    from oracle import manopt_rtr
    key = ("step", kind, n, d, p, warm)
    if Y is not None or key not in _REF:
        x = np.array((warm_start if warm else start)(kind, n, d, p) if Y is None else Y, dtype=np.float64)
        prob = problem(kind, matrix(kind, n, d), n, d, p)
        prob.cost(x)
        out = manopt_rtr.tCG(prob, x, prob.grad(x), prob.M.typicaldist() / 8.0, MAXINNER)
        if Y is not None:
            return out
        _REF[key] = out
    return _REF[key]


def counts(info):
    return (info.iters, info.hessvecs, info.accepted, info.rejected, info.stop_inner[-1] if info.stop_inner else 0)


def perturbed(kind, Y0, d, rng):
    return ref(kind).polar_blocks(Y0 * (1.0 + 1e-14 * rng.standard_normal(Y0.shape)), d)


# ------------------------------------------------------------------ the plan, restated (msdp_blockpersist_plan.h)
THREADS, WAVES, MAXLPR, MAXR, MAXGRID, LDS_MAX, LDS_STATIC = 512, 8, 16, 2, 256, 160 * 1024, 256
CUS = 256                                      # compute units of the device the ledger is written for


def ld_of(p):
    """The row stride of the factor: p rounded up to even (a lane holds two columns)."""
    return p + (p & 1)


def lpr_of(p):
    """Lanes per block: the smallest power of two with 2 lpr >= ld."""
    lpr = 1
    while 2 * lpr < ld_of(p):
        lpr *= 2
    return lpr


def rstep_of(lpr):
    """Blocks per row slot of a workgroup of 8 waves."""
    return WAVES * 64 // lpr


def lds_of(B, efree, lpr, R):
    """Dynamic LDS bytes of a workgroup: a double2 per thread for the D rows of Y and the B rows of the gradient, and the D x D
    multiplier block of every owned block, per row slot."""
    D = B - efree
    return R * ((D + B) * THREADS * 16 + rstep_of(lpr) * D * D * 8)


def plan(nb, B, efree, p, cus=CUS, grid_cap=0, wide=0):
    """dict(lpr, grid, slots, rstep, lds) of msdp_blockpersist_plan, or None where it has none."""
    D = B - efree
    if nb < 1 or not 2 <= B <= 4 or efree not in (0, 1) or not 2 <= D <= 3 or p < 1 or p > 2 * MAXLPR:
        return None
    gmax = min(cus, MAXGRID)
    if 0 < grid_cap < gmax:
        gmax = max(grid_cap, 8)
    gmax = gmax // 8 * 8
    if gmax < 8 or gmax > cus:
        return None
    lpr = lpr_of(p)
    rstep = rstep_of(lpr)
    for R in range(1, MAXR + 1):
        lds = lds_of(B, efree, lpr, R)
        if lds + LDS_STATIC > LDS_MAX:
            break
        cap = R * rstep                          # blocks of a workgroup
        if cap * gmax < nb:
            continue
        G = max(((nb + cap - 1) // cap + 7) // 8 * 8, 8)      # the fewest workgroups that need R slots
        return dict(lpr=lpr, grid=gmax if wide else G, slots=R, rstep=rstep, lds=lds)
    return None


def plan_of(kind, n, d, p, grid_cap=0, cus=CUS, wide=0):
    return plan(n, blk(kind, d), int(kind == "pose"), p, cus, grid_cap, wide)


def instance_of(kind, n, d, p, grid_cap, cus=CUS):
    """(D, EF, lpr, R) of the kernel k_tcg_persist_blk<D, EF, LPR, R> that runs the case, or None where no plan exists."""
    pl = plan_of(kind, n, d, p, grid_cap, cus)
    return (d, int(kind == "pose"), pl["lpr"], pl["slots"]) if pl else None


def gather_depth(B, R):
    """Entries of a block row in flight together (bp_batch of msdp_blockpersist.hip)."""
    return 4 if R == 1 else {2: 4, 3: 2, 4: 1}[B]


INSTANTIATED = frozenset((D, EF, lpr, R) for D in (2, 3) for EF in (0, 1) for lpr in (1, 2, 4, 8, 16) for R in (1, 2))
# D = 3 needs p >= 3, hence ld >= 4 and lpr >= 2: blk_kernel_de instantiates these four, no handle selects them
UNREACHABLE = frozenset((3, EF, 1, R) for EF in (0, 1) for R in (1, 2))


def gpu_runs():
    """Every (kind, n, d, p, grid cap) that the device tests run on the persistent path with a plan (the ledger)."""
    runs = set()
    for (kind, n, d, p) in cases() + two_slot_cases():
        runs |= {(kind, n, d, p, 0), (kind, n, d, p, 8)}
    for (kind, n, d, p, _) in LONG_CASES:
        runs |= {(kind, n, d, p, 0), (kind, n, d, p, 8)}
    for (kind, n, d, p, _, grid) in LONG_TWO_SLOT_CASES:
        runs.add((kind, n, d, p, grid))
    for kind in KINDS:
        for (n, d, p) in STEP_SHAPES + OPTION_SHAPES + MASKED_SHAPES:
            runs |= {(kind, n, d, p, 0), (kind, n, d, p, 8)}
        for n in FEW_BLOCKS:
            for d in (2, 3):
                runs |= {(kind, n, d, d, 0), (kind, n, d, 32, 0)}
        n, d, p = CAP_TOO_SMALL
        runs.add((kind, n, d, p, 0))
    for (kind, n, d, p, _, _) in FINISHED_CASES:
        runs.add((kind, n, d, p, 0))
    return sorted(runs)
