"""Per-iteration record of the decisions of Manopt's trust-region solver, and the case table of tests/test_gpu_tr_decisions.py.

oracle.manopt_rtr.trustregions / tCG (tCG.m:160-289, trustregions.m:441-729) restated in plain NumPy with the same arithmetic, for
any problem object the oracle accepts (M, cost, grad, hess, on_accept / on_reject; an optional `precon(x, r)` takes the
preconditioned branch of tCG.m as tests/posegraph_precon_ref.py states it).  Besides the oracle's result, `trustregions` returns
one record per TR iteration: numinner, stop_inner, accepted, the radius action (`quarter`, `double`, `double_capped` where
2 Delta > Delta_bar, `keep`), Delta / cost / gradnorm after the iteration, and the iteration's MARGIN: the smallest relative distance
from equality of every comparison the iteration took, each scaled by the quantities compared:

    d_Hd against 0                      |d_Hd| / (|mdelta| |H mdelta|)                                        tCG.m:183
    e_Pe_new against Delta^2            |e_Pe_new - Delta^2| / Delta^2                                        tCG.m:183
    new_model against model_value       |difference| / the larger magnitude                                   tCG.m:228
    norm_r against its threshold        |norm_r - t| / t, on the trips with j >= mininner                     tCG.m:249
    kappa against norm_r0^theta         |difference| / the larger of the two                                  tCG.m:249-255
    rho against 0.25, 0.75, rho_prime   |rho - t| |rhoden| / max(1, |fx|)                                     trustregions.m:653-688
    rhoden against 0                    |rhoden| / max(1, |fx|)                                               trustregions.m:614
    norm_grad against tolgradnorm       |norm_grad - tol| / tol, the test in front of the iteration           stoppingcriterion.m:51

An iteration is DECIDED when its margin is at least DECIDED = 1e-9: three orders above the 1e-12 relative tolerance the suite holds
every operator to, the headroom for what accumulates over a tCG of a few dozen trips.  It is a condition on the choice of cases, not
a tolerance on the device: a case is compared with the device up to its first undecided iteration and no further
(`decided_prefix`).  tests/test_tr_decisions_ref_host.py holds this file to the oracle and the case table to its coverage.

The case table: ROUTES names every route through the decision code in the device sources with the handle options that
reach it and what the path queries must report; `case(name)` builds the problems, at the smallest shapes each route accepts;
OPTION_SETS are the option sets every case runs under for MAXITER trust-region iterations."""
import functools
import math
import os

import numpy as np

from oracle.manopt_rtr import EPS, RTRInfo

DECIDED = 1e-9
MAXITER = 12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------ the restatement
def _rel(a, b):
    s = max(abs(a), abs(b))
    return abs(a - b) / s if s > 0 and math.isfinite(s) else 0.0


def tCG(problem, x, grad, Delta, maxinner, kappa=0.1, theta=1.0, mininner=1):
    """oracle.manopt_rtr.tCG (posegraph_precon_ref.tCG where the problem has a preconditioner), returning
    (eta, Heta, inner_it, stop_tCG, margin)."""
    M = problem.M
    inner = lambda a, b: M.inner(x, a, b)
    precon = getattr(problem, "precon", None)
    margins = []
    eta = M.zerovec(x)
    Heta = M.zerovec(x)
    r = grad
    e_Pe = 0.0
    r_r = inner(r, r)
    norm_r = math.sqrt(r_r)
    norm_r0 = norm_r
    z = precon(x, r) if precon else r
    z_r = inner(z, r)
    d_Pd = z_r
    mdelta = z
    e_Pd = 0.0
    model_value = 0.0
    stop_tCG = 5
    margins.append(_rel(kappa, norm_r0 ** theta))
    j = 0
    for j in range(1, maxinner + 1):
        Hmdelta = problem.hess(x, mdelta)
        d_Hd = inner(mdelta, Hmdelta)
        margins.append(abs(d_Hd) / max(M.norm(x, mdelta) * M.norm(x, Hmdelta), 1e-300))
        alpha = z_r / d_Hd if d_Hd != 0.0 else math.copysign(math.inf, z_r) if z_r != 0 else math.nan
        e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd
        if d_Hd > 0:
            margins.append(abs(e_Pe_new - Delta ** 2) / Delta ** 2)
        if d_Hd <= 0 or e_Pe_new >= Delta ** 2:
            tau = (-e_Pd + math.sqrt(e_Pd * e_Pd + d_Pd * (Delta ** 2 - e_Pe))) / d_Pd
            eta = eta - tau * mdelta
            Heta = Heta - tau * Hmdelta
            stop_tCG = 1 if d_Hd <= 0 else 2
            break
        e_Pe = e_Pe_new
        new_eta = eta - alpha * mdelta
        new_Heta = Heta - alpha * Hmdelta
        new_model_value = inner(new_eta, grad) + 0.5 * inner(new_eta, new_Heta)
        margins.append(_rel(new_model_value, model_value))
        if new_model_value >= model_value:
            stop_tCG = 6
            break
        eta = new_eta
        Heta = new_Heta
        model_value = new_model_value
        r = r - alpha * Hmdelta
        r_r = inner(r, r)
        norm_r = math.sqrt(r_r)
        bound = norm_r0 * min(norm_r0 ** theta, kappa)
        if j >= mininner:
            margins.append(abs(norm_r - bound) / bound if bound > 0 else 0.0)
        if j >= mininner and norm_r <= bound:
            stop_tCG = 3 if kappa < norm_r0 ** theta else 4
            break
        z = precon(x, r) if precon else r
        zold_rold = z_r
        z_r = inner(z, r)
        beta = z_r / zold_rold
        mdelta = z + beta * mdelta
        mdelta = M.tangent(x, mdelta)
        e_Pd = beta * (e_Pd + alpha * d_Pd)
        d_Pd = z_r + beta * beta * d_Pd
    margin = min(margins)
    return eta, Heta, j, stop_tCG, (margin if math.isfinite(margin) else 0.0)


class Run:
    """What `trustregions` returns: the oracle's (x, fx, info), the records, why the loop ended (`tolgradnorm` or `maxiter`) and the
    margin of the gradient test that ended it (None for `maxiter`)."""

    def __init__(self, x, fx, info, records, ended, end_margin):
        self.x, self.fx, self.info, self.records, self.ended, self.end_margin = x, fx, info, records, ended, end_margin

    def totals(self, k=None):
        """(iters, hessvecs, accepted, rejected, last_stop_inner) after the first k records (all of them by default)."""
        rec = self.records if k is None else self.records[:k]
        acc = sum(1 for r in rec if r["accepted"])
        return (len(rec), sum(r["numinner"] for r in rec), acc, len(rec) - acc, rec[-1]["stop_inner"] if rec else 0)

    def decided_prefix(self):
        """Number of leading records with a margin of at least DECIDED."""
        k = 0
        while k < len(self.records) and self.records[k]["margin"] >= DECIDED:
            k += 1
        return k

    def end_decided(self):
        """The loop ended on tolgradnorm before MAXITER, every iteration before that and the test that ended it decided."""
        return (self.ended == "tolgradnorm" and self.decided_prefix() == len(self.records)
                and self.end_margin is not None and self.end_margin >= DECIDED)

    def outcomes(self, k=None):
        """(stop codes, (accepted, action) pairs) of the first k records (the decided prefix by default)."""
        rec = self.records[:self.decided_prefix() if k is None else k]
        return {r["stop_inner"] for r in rec}, {("accept" if r["accepted"] else "reject", r["action"]) for r in rec}

    def sequence(self, k=None):
        """The decisions of the first k records (the decided prefix by default), for comparing two option sets."""
        rec = self.records[:self.decided_prefix() if k is None else k]
        return [(r["numinner"], r["stop_inner"], r["accepted"], r["action"]) for r in rec]


def trustregions(problem, x, maxiter, maxinner, tolgradnorm, kappa=0.1, theta=1.0, rho_prime=0.1, rho_regularization=1e3,
                 mininner=1, Delta_bar=None, Delta0=None):
    """oracle.manopt_rtr.trustregions with records: returns a Run."""
    M = problem.M
    if Delta_bar is None:
        Delta_bar = M.typicaldist()
    if Delta0 is None:
        Delta0 = Delta_bar / 8.0
    info = RTRInfo()
    fx = problem.cost(x)
    info.cost_evals += 1
    fgradx = problem.grad(x)
    norm_grad = M.norm(x, fgradx)
    Delta = Delta0
    records = []
    k = 0
    while True:
        grad_margin = abs(norm_grad - tolgradnorm) / tolgradnorm if tolgradnorm > 0 else 1.0
        if norm_grad < tolgradnorm:
            ended, end_margin = "tolgradnorm", grad_margin
            break
        if k >= maxiter:
            ended, end_margin = "maxiter", None
            break
        eta, Heta, numit, stop_inner, margin = tCG(problem, x, fgradx, Delta, maxinner, kappa=kappa, theta=theta, mininner=mininner)
        margins = [grad_margin, margin]
        info.hessvecs += numit
        info.numinner.append(numit)
        info.stop_inner.append(stop_inner)
        x_prop = M.retr(x, eta)
        fx_prop = problem.cost(x_prop)
        info.cost_evals += 1
        rhonum = fx - fx_prop
        vecrho = fgradx + 0.5 * Heta
        rhoden = -M.inner(x, eta, vecrho)
        rho_reg = max(1.0, abs(fx)) * EPS * rho_regularization
        rhonum = rhonum + rho_reg
        rhoden = rhoden + rho_reg
        scale = max(1.0, abs(fx))
        margins.append(abs(rhoden) / scale)
        model_decreased = rhoden >= 0
        rho = rhonum / rhoden if rhoden != 0 else (math.nan if rhonum == 0 else math.copysign(math.inf, rhonum))
        if math.isnan(rho):
            margins.append(0.0)
        cmp_rho = lambda t: abs(rho - t) * abs(rhoden) / scale
        action = "keep"
        margins.append(cmp_rho(0.25))
        if rho < 0.25 or (not model_decreased) or math.isnan(rho):
            Delta = Delta / 4.0
            action = "quarter"
        else:
            margins.append(cmp_rho(0.75))
            if rho > 0.75 and stop_inner in (1, 2):
                action = "double_capped" if 2.0 * Delta > Delta_bar else "double"
                Delta = min(2.0 * Delta, Delta_bar)
        if model_decreased:
            margins.append(cmp_rho(rho_prime))
        accepted = bool(model_decreased and rho > rho_prime)
        if accepted:
            x = x_prop
            fx = fx_prop
            if hasattr(problem, "on_accept"):
                problem.on_accept()
            fgradx = problem.grad(x)
            norm_grad = M.norm(x, fgradx)
            info.accepted += 1
        else:
            if hasattr(problem, "on_reject"):
                problem.on_reject()
            info.rejected += 1
        k += 1
        m = min(margins)
        records.append(dict(numinner=numit, stop_inner=stop_inner, accepted=accepted, action=action, Delta=Delta, cost=fx,
                            gradnorm=norm_grad, rho=rho, margin=m if math.isfinite(m) else 0.0))
    info.gradnorm = norm_grad
    info.cost = fx
    info.iters = k
    info.Delta = Delta
    return Run(x, fx, info, records, ended, end_margin)


# ------------------------------------------------------------------ the cases
def _unit_rows(n, p, seed):
    Y = np.random.default_rng(seed).standard_normal((n, p))
    return Y / np.linalg.norm(Y, axis=1, keepdims=True)


def _sdpa(name):
    from manisdp_matlab_amd import problems
    At, b, c, K = problems.from_sdpa(os.path.join(GOLDEN, name + ".dat-s.gz"))
    return At, np.asarray(b, float), np.asarray(c.todense()).ravel(), K["s"]


def _bqp(d):
    from manisdp_matlab_amd import problems
    Q = np.loadtxt(os.path.join(GOLDEN, f"bqp_Q_{d}_1.txt.gz"), delimiter=",")
    e = np.loadtxt(os.path.join(GOLDEN, f"bqp_e_{d}_1.txt.gz"), delimiter=",")
    At, b, c, K = problems.bqpmom(d, Q, e)
    c = np.asarray(c.todense()).ravel()
    return At, np.asarray(b, float), c / np.abs(c).max(), K["s"]


class Case:
    """A problem of the table: `problem()` a fresh oracle problem object, `Y0` the start (read-only), `handle(lib)` the device handle
    before any route option is set, `maxinner` the inner cap of the option sets that do not set their own."""

    def __init__(self, kind, data, Y0, maxinner=30, **par):
        self.kind, self.data, self.Y0, self.maxinner, self.par = kind, data, Y0, maxinner, par
        self.Y0.setflags(write=False)

    def problem(self):
        from oracle import manisdp_ref as R
        n, p = self.Y0.shape
        if self.kind in ("sparse", "dense"):
            return R._OnlyUnitDiagProblem(self.data, n, p, q1="correct")
        if self.kind in ("unitdiag", "unittrace", "generic"):
            At, b, c = self.data
            cls = {"unitdiag": R._UnitDiagProblem, "unittrace": R._UnitTraceProblem, "generic": R._GenericProblem}[self.kind]
            prob = cls(At, b, c, n, p)
            prob.y, prob.sigma = self.par["y"], self.par["sigma"]
            return prob
        d = self.par["d"]
        if self.kind == "blockdiag":
            import blockdiag_ref
            return blockdiag_ref.Problem(self.data, n // d, d, p)
        if self.kind == "posegraph":
            import posegraph_ref
            return posegraph_ref.Problem(self.data, n // (d + 1), d, p)
        import posegraph_precon_ref
        return posegraph_precon_ref.Problem(self.data, n // (d + 1), d, p, posegraph_precon_ref.minv_blocks(self.data, d))

    def handle(self, lib):
        p = self.Y0.shape[1]
        if self.kind in ("sparse", "dense"):
            return lib.Handle.onlyunitdiag(self.data, pcap=p)
        if self.kind in ("unitdiag", "unittrace", "generic"):
            At, b, c = self.data
            kind = {"unitdiag": lib.KIND_UNITDIAG, "unittrace": lib.KIND_UNITTRACE, "generic": lib.KIND_GENERIC}[self.kind]
            h = lib.Handle.affine(kind, At, b, c, self.Y0.shape[0], pcap=p)
            h.set_multipliers(self.par["y"], self.par["sigma"])
            return h
        if self.kind == "blockdiag":
            return lib.Handle.onlyunitblockdiag(self.data, self.par["d"], pcap=p)
        return lib.Handle.posegraph(self.data, self.par["d"], pcap=p)           # (the route sets "precon")


@functools.lru_cache(maxsize=None)
def case(name):
    from manisdp_matlab_amd import problems
    kind, _, arg = name.partition(":")
    if kind == "torus":                                    # torus:7x11:4 -- toroidal_grid_maxcut(7, 11, seed=3) at p = 4
        shape, p = arg.split(":")
        a, b = (int(v) for v in shape.split("x"))
        C = problems.toroidal_grid_maxcut(a, b, seed=3)
        return Case("sparse", C, _unit_rows(C.shape[0], int(p), 11))
    if kind == "G1":                                       # G1:12 -- rows of about 48 entries: the CSR-row instances
        C = problems.maxcut_cost_matrix(os.path.join(GOLDEN, "G1.txt.gz"))
        return Case("sparse", C, _unit_rows(C.shape[0], int(arg), 11))
    if kind == "dense":                                    # dense:33:5 -- a dense symmetric matrix of order 33
        n, p = (int(v) for v in arg.split(":"))
        A = np.random.default_rng(33).standard_normal((n, n))
        return Case("dense", np.ascontiguousarray(A + A.T), _unit_rows(n, p, 11))
    if kind == "bqp":                                      # bqp:10:4 -- the unit-diagonal affine kind
        d, p = (int(v) for v in arg.split(":"))
        At, b, c, n = _bqp(d)
        y = np.random.default_rng(5).standard_normal(b.size) * 0.1
        return Case("unitdiag", (At, b, c), _unit_rows(n, p, 3), y=y, sigma=0.37)
    if kind == "theta":                                    # theta:1:3 -- theta1 on the sphere
        k, p = (int(v) for v in arg.split(":"))
        At, b, c, n = _sdpa(f"theta{k}")
        Y = np.random.default_rng(3).standard_normal((n, p))
        y = np.random.default_rng(5).standard_normal(b.size)
        return Case("unittrace", (At, b, c), Y / np.linalg.norm(Y), y=y, sigma=1000.0)
    if kind == "generic":                                  # generic:mcp100:5 -- the Euclidean manifold
        nm, p = arg.split(":")
        At, b, c, n = _sdpa(nm)
        Y = 0.5 * np.random.default_rng(3).standard_normal((n, int(p)))
        return Case("generic", (At, b, c), Y, y=np.zeros(b.size), sigma=10.0)
    if arg.count(":") == 4:                                # posepc:67:3:6:5:w20 -- from the cold case's point after 20 iterations
        cold, _, w = name.rpartition(":w")
        c = case(cold)
        return Case(c.kind, c.data, np.array(trustregions(c.problem(), np.array(c.Y0), int(w), **options(cold, "default")).x), **c.par)
    n, d, degree, p = (int(v) for v in arg.split(":"))     # stiefel:67:3:6:5, pose:41:2:4:4, posepc:...
    if kind == "stiefel":
        import blockdiag_ref
        return Case("blockdiag", blockdiag_ref.instance(n, d, degree, 1.0)[0], blockdiag_ref.point(n, d, p).copy(), d=d)
    import posegraph_ref
    return Case("posegraph" if kind == "pose" else "posegraph_precon", posegraph_ref.instance(n, d, degree, 0.3)[0],
                posegraph_ref.point(n, d, p).copy(), d=d)


OPTION_SETS = ("default", "delta0_bar", "delta_small", "theta2", "kappa_small", "mininner5", "maxinner3", "rho_prime", "rho_reg",
               "tolgrad", "mininner5_theta2", "rho_prime_delta0_bar")
# What the set of an option is compared with to show that the option is under test: the set without it.  Under the default kappa and
# theta only the sphere and Euclidean cases have a tCG that converges in under five trips within MAXITER iterations, so mininner = 5
# alone changes nothing elsewhere: the eleventh set adds it to theta = 2, kappa = 0.5, whose tCGs stop after one to three trips.
# The preconditioned cases accept no step with rho below 0.25 from the default start radius but do from Delta0 = Delta_bar: the
# twelfth set is rho_prime = 0.24 from there.
OPTION_BASE = {"theta2": "default", "kappa_small": "default", "mininner5": "default", "rho_prime": "default", "rho_reg": "default",
               "mininner5_theta2": "theta2", "rho_prime_delta0_bar": "delta0_bar"}
OPTIONS_UNDER_TEST = {"mininner": ("mininner5", "mininner5_theta2"), "kappa": ("kappa_small",), "theta": ("theta2",),
                      "rho_prime": ("rho_prime", "rho_prime_delta0_bar"), "rho_regularization": ("rho_reg",)}
TOLGRAD_OFF = 1e-12                # no case comes near it in MAXITER iterations


def _mid_run_tolerance(run):
    """A gradient tolerance the default run meets in mid-run: the geometric mean of the gradient norms on both sides of the first
    accepted step, from the fourth iteration on, that takes the norm below everything before it; None where there is none."""
    g = [r["gradnorm"] for r in run.records]
    for k in range(3, len(g) - 1):
        if g[k] < min(g[:k]) and g[k] > 0:
            return math.sqrt(g[k] * min(g[:k]))
    return None


def options(name, opt):
    """The keyword arguments (of `trustregions` here, of the oracle's, and the fields of the device's options) of an option set."""
    c = case(name)
    typical = c.problem().M.typicaldist()
    o = dict(maxinner=c.maxinner, tolgradnorm=TOLGRAD_OFF)
    if opt == "delta0_bar":
        o.update(Delta0=typical)
    elif opt == "delta_small":
        o.update(Delta_bar=typical / 16.0, Delta0=typical / 16.0)
    elif opt == "theta2":
        o.update(theta=2.0, kappa=0.5)
    elif opt == "kappa_small":
        o.update(kappa=1e-3)
    elif opt == "mininner5":
        o.update(mininner=5)
    elif opt == "mininner5_theta2":
        o.update(mininner=5, theta=2.0, kappa=0.5)
    elif opt == "maxinner3":
        o.update(maxinner=3)
    elif opt == "rho_prime":
        o.update(rho_prime=0.24)
    elif opt == "rho_prime_delta0_bar":
        o.update(rho_prime=0.24, Delta0=typical)
    elif opt == "rho_reg":
        o.update(rho_regularization=1e14)
    elif opt == "tolgrad":
        tol = _mid_run_tolerance(reference(name, "default"))
        if tol is not None:
            o.update(tolgradnorm=tol)
    elif opt != "default":
        raise KeyError(opt)
    return o


@functools.lru_cache(maxsize=None)
def reference(name, opt):
    """The Run of a case under an option set, computed once and never written to."""
    c = case(name)
    return trustregions(c.problem(), np.array(c.Y0), MAXITER, **options(name, opt))


# ------------------------------------------------------------------ what the reference itself can carry
# The device is held to the reference's cost to 1e-11 and to its gradient norm to 1e-8 relative.  A tCG of a few dozen trips on an
# ill-conditioned Hessian amplifies rounding: on some cases the reference's OWN cost after such an iteration moves by 1e-9 to 1e-5
# when its start is perturbed by 1e-14 relative, two orders above machine epsilon (the Euclidean case under kappa = 1e-3, the
# pose-graph cases at their inner cap).  No implementation can be held to the bounds there, so a case is compared with the device
# up to `prefix(name, opt)`: its decided prefix, cut in front of the first iteration at which, under three such perturbations, a
# decision changes or the cost or the gradient norm moves by more than a tenth of the device's bound.  It never reaches further
# than the decided prefix, and the coverage the host test asserts is that of this prefix.
PERTURBATION, STABLE_COST, STABLE_GRADNORM = 1e-14, 1e-12, 1e-9


@functools.lru_cache(maxsize=None)
def prefix(name, opt):
    base = reference(name, opt)
    c = case(name)
    K = base.decided_prefix()
    g = np.random.default_rng(1)
    for _ in range(3):
        Y = np.array(c.Y0) * (1.0 + PERTURBATION * g.standard_normal(c.Y0.shape))
        run = trustregions(c.problem(), Y, MAXITER, **options(name, opt))
        k = 0
        while k < min(K, len(run.records)):
            a, b = run.records[k], base.records[k]
            if ((a["numinner"], a["stop_inner"], a["accepted"], a["action"], a["Delta"]) != (b["numinner"], b["stop_inner"], b["accepted"], b["action"], b["Delta"])
                    or abs(a["cost"] - b["cost"]) > STABLE_COST * max(1.0, abs(b["cost"]))
                    or abs(a["gradnorm"] - b["gradnorm"]) > STABLE_GRADNORM * max(1.0, b["gradnorm"])):
                break
            k += 1
        K = k
    return K


def ends_in_mid_run(name, opt):
    """The reference stops on tolgradnorm at an iteration 0 < k < MAXITER, every iteration before it compared and the test that
    stops it decided."""
    run = reference(name, opt)
    return run.end_decided() and 0 < len(run.records) < MAXITER and prefix(name, opt) == len(run.records)


# ------------------------------------------------------------------ the routes
# Every route through the decision code (row), the handle options that reach it (set in this order before the point), what tcg_path(),
# persist_form() and trip_form() must report after every call, whether the chunked trips run with "graph" 1 and 0, and its cases.
_TORUS = ("torus:7x11:4", "torus:7x11:8", "torus:5x10:5", "torus:33x37:17")
_BLOCK = ("stiefel:67:3:6:5", "stiefel:101:2:4:4", "pose:41:2:4:4", "pose:67:3:6:5")
ROUTES = {
    # k_tcg_upd1 / k_tcg_upd2_obl + k_rtr_decide (msdp_kernels.hip)
    "three_launch/sparse": dict(row="three_launch", opts=(("persist", 0), ("trip1", 0), ("trip2", 0)), path=0, trip=3, graphs=(1, 0),
                                cases=_TORUS + ("G1:12",)),
    "three_launch/dense": dict(row="three_launch", opts=(), path=0, trip=3, graphs=(1, 0), cases=("dense:33:5",)),
    "three_launch/unitdiag": dict(row="three_launch", opts=(), path=0, trip=3, graphs=(1, 0), cases=("bqp:10:4",)),
    # msdp_trip2.hip
    "two_launch": dict(row="two_launch", opts=(("persist", 0), ("trip1", 0), ("trip2", 2)), path=0, trip=2, graphs=(1, 0),
                       cases=_TORUS + ("G1:12",)),
    # msdp_trip1.hip
    "linear": dict(row="linear", opts=(("persist", 0),), path=0, trip=1, graphs=(1, 0), cases=_TORUS + ("G1:12",)),
    # msdp_persist.hip: the two-reduction trip and its fused TR loop
    "persist_two/fused": dict(row="persist_two_fused", opts=(("persist_pipe", 0), ("fused_rtr", 1)), path=1, form=0, trip=0,
                              cases=_TORUS + ("G1:12",)),
    # the same tCG + k_tr_tail_obl (msdp_trtail.hip)
    "persist_two/tail": dict(row="persist_two_tail", opts=(("persist_pipe", 0), ("fused_rtr", 0)), path=1, form=0, trip=0,
                             cases=_TORUS + ("G1:12",)),
    # msdp_pipe.h: the one-reduction trip, its fused TR loop and the per-iteration launches
    "pipe/fused": dict(row="pipe", opts=(("persist_pipe", 1), ("fused_rtr", 1)), path=1, form=2, trip=0, cases=_TORUS + ("G1:12",)),
    "pipe/tail": dict(row="pipe", opts=(("persist_pipe", 1), ("fused_rtr", 0)), path=1, form=2, trip=0, cases=_TORUS + ("G1:12",)),
    # k_sph_upd2a (msdp_sphere.hip)
    "sphere": dict(row="sphere", opts=(), path=0, trip=3, graphs=(1, 0),
                   cases=("theta:1:3", "theta:1:6", "generic:mcp100:5")),
    # msdp_tcg_upd2_scalars (msdp_device.h)
    "block": dict(row="block", opts=(), path=0, trip=3, graphs=(1, 0), cases=_BLOCK),
    # msdp_tcg_upd2_scalars<true>, the preconditioned form (k_pose_pc_upd2, msdp_pose_precon.hip)
    "pose_precon": dict(row="pose_precon", opts=(("precon", 1),), path=0, trip=3, graphs=(1, 0),
                        cases=("posepc:41:2:4:4", "posepc:67:3:6:5", "posepc:67:3:6:5:w12", "posepc:67:3:6:5:w20")),
    # k_tcg_persist_blk (msdp_blockpersist.hip)
    "block_persist": dict(row="block_persist", opts=(("block_persist", 1),), path=1, form=0, trip=0, block_persist=True, cases=_BLOCK),
}
ROWS = tuple(dict.fromkeys(r["row"] for r in ROUTES.values()))
ALL_CASES = tuple(dict.fromkeys(c for r in ROUTES.values() for c in r["cases"]))

STOPS_REQUIRED = {1, 2, 3, 4, 5}
OUTCOMES_REQUIRED = {("accept", "double"), ("accept", "double_capped"), ("accept", "keep"), ("accept", "quarter"),
                     ("reject", "quarter")}


def row_cases(row):
    return tuple(dict.fromkeys(c for r in ROUTES.values() if r["row"] == row for c in r["cases"]))
