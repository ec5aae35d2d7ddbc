"""Host-side mirrors of the reference's three primal entry points.

Same names, option names, defaults, printed protocol and ``data`` fields as
``src/primal/ManiSDP_onlyunitdiag.m``, ``ManiSDP_unitdiag.m`` and
``ManiSDP_unittrace.m``.  The augmented-Lagrangian loop and the bookkeeping
(multiplier / sigma updates, KKT residues, rank cut, escape set-up) stay on the
host exactly as in the reference; every ``trustregions(problem, Y, opts)`` call
(``ManiSDP_onlyunitdiag.m:43``, ``ManiSDP_unitdiag.m:57``, ``ManiSDP_unittrace.m:57``)
is replaced by ``msdp_rtr`` on the HIP library, with the factor resident in HBM.

Factors are NumPy ``(n, p)`` arrays (for the oblique kinds the bytes of MATLAB's
``p x n`` column-major ``Y``).  Returned ``X`` is the factor ``Y`` (``X = Y Y'``);
``data['X']`` holds the dense matrix only when ``n <= options['dense_X_max']``.
"""
from __future__ import annotations

import math
import time

import numpy as np
import scipy.sparse as sp

from . import _lib


# Several replicated host loops in ONE process (the in-process ranks of tests/test_gpu_local_ranks.py: N threads, one BLAS
# pool) must not race for BLAS threads: how many each call gets would decide the summation order of the p x p Gram / thin-SVD
# arithmetic, and replicated loops must produce the same bits.  The harness sets this to 1; one process per GPU never needs it.
FORCED_HOST_THREADS = None


def _host_threads():
    """Context manager capping the BLAS/LAPACK threads of the host-side AL bookkeeping (thin SVD, residues) at the
    CPUs this process may actually use.  On a 256-core box inside a 16-CPU cgroup quota the default (256 threads on
    20000 x 40 matrices) burns the quota and gets the thread that feeds the GPU throttled."""
    import contextlib
    import os
    try:
        from threadpoolctl import threadpool_limits
    except Exception:                                      # pragma: no cover
        return contextlib.nullcontext()
    try:
        ncpu = len(os.sched_getaffinity(0))
    except Exception:                                      # pragma: no cover
        ncpu = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            ncpu = min(ncpu, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    if FORCED_HOST_THREADS:
        return threadpool_limits(limits=int(FORCED_HOST_THREADS))
    return threadpool_limits(limits=max(1, min(ncpu, 16)))

__all__ = ["ManiSDP_onlyunitdiag", "ManiSDP_unitdiag", "ManiSDP_unittrace", "ManiSDP", "ManiSDP_multiblock",
           "ManiDSDP_unitdiag", "round_unitdiag", "ManiSDP_onlyunitblockdiag", "onlyunitblockdiag_defaults", "ManiSDP_posegraph", "posegraph_defaults", "DEFAULTS",
           "DATA_FIELDS"]

# Option defaults of the reference's entry points: ManiSDP_onlyunitdiag.m:8-17,
# ManiSDP_unitdiag.m:10-26, ManiSDP_unittrace.m:10-25, ManiSDP.m:9-25.
DEFAULTS = {
    "onlyunitdiag": dict(p0=2, AL_maxiter=20, tol=1e-8, theta=1e-1, delta=8, alpha=0.5, tolgradnorm=1e-8,
                         TR_maxinner=100, TR_maxiter=40, line_search=0),
    "unitdiag": dict(p0=2, AL_maxiter=300, gama=2, sigma0=1e-3, sigma_min=1e-2, sigma_max=1e7, tol=1e-8,
                     theta=1e-3, delta=8, alpha=0.1, tolgradnorm=1e-8, TR_maxinner=20, TR_maxiter=4,
                     tau1=1, tau2=1, line_search=0),
    "unittrace": dict(p0=1, AL_maxiter=1000, gama=2, sigma0=1e1, sigma_min=1e2, sigma_max=1e7, tol=1e-8,
                      theta=1e-2, delta=8, alpha=0.05, tolgradnorm=1e-8, TR_maxinner=40, TR_maxiter=3,
                      tau1=1e-5, tau2=1e-4, line_search=1),
    "generic": dict(p0=1, AL_maxiter=1000, gama=2, sigma0=1e-2, sigma_min=1e-1, sigma_max=1e7, tol=1e-8,
                    theta=1e-2, delta=8, alpha=0.1, tolgradnorm=1e-8, TR_maxinner=20, TR_maxiter=4,
                    tau1=1e-2, tau2=1e-1, line_search=1, solver=0),
}
# Fields of the reference's `data` output (ManiSDP_onlyunitdiag.m:86-95, ManiSDP_unitdiag.m:114-127,
# ManiSDP_unittrace.m:119-131); the Python mirrors add counters (hessvecs, rtr_seconds, ...) next to them.
DATA_FIELDS = {
    "onlyunitdiag": ("X", "S", "z", "dinf", "gradnorm", "time", "status"),
    "unitdiag": ("X", "y", "S", "z", "gap", "pinf", "dinf", "gradnorm", "time", "fac_size", "status"),
    "unittrace": ("X", "y", "S", "z", "gap", "pinf", "dinf", "gradnorm", "time", "status"),
    "generic": ("X", "y", "S", "gap", "pinf", "dinf", "gradnorm", "time", "status"),
}


def _join_comm(h, comm):
    """options['comm']: (nranks, rank, rccl_unique_id) -- one process per GPU -- or ("local", nranks, rank, group) -- the
    in-process stand-in of msdp_comm_init_local: N handles of one process on one GPU, one host thread each."""
    if comm[0] == "local":
        h.comm_init_local(int(comm[1]), int(comm[2]), int(comm[3]))
    else:
        h.comm_init(int(comm[0]), int(comm[1]), comm[2])


def _say(verbose, msg):
    if verbose:
        print(msg, flush=True)


def _rtr_opts(o):
    return _lib.default_opts(maxiter=int(o["TR_maxiter"]), maxinner=int(o["TR_maxinner"]),
                             tolgradnorm=float(o["tolgradnorm"]))


_RANK_CUT_SVD = False


def _thin_svd_rank(Y, theta, gram=None):
    """svd(Y) and r = sum(e >= theta*e(1)) (ManiSDP_onlyunitdiag.m:52-54) through the
    p x p Gram matrix: never forms the n x n V of the reference.  ``gram``: the Gram matrix
    as the device computed it (msdp_factor_gram), Y is not needed then."""
    if _RANK_CUT_SVD and gram is None:
        _, e, Qt = np.linalg.svd(Y, full_matrices=False)
        return Qt.T, e, int(np.sum(e >= theta * e[0]))
    G = gram if gram is not None else Y.T @ Y
    w, Q = np.linalg.eigh(G)
    order = np.argsort(w)[::-1]
    w = np.maximum(w[order], 0.0)
    Q = Q[:, order]
    e = np.sqrt(w)
    r = int(np.sum(e >= theta * e[0]))
    return Q, e, r


def _rank_cut(Y, Q, e, r):
    """Y = V(:,1:r)'.*e(1:r): with Y = V diag(e) Q', V(:,k) e_k = Y Q(:,k)."""
    return Y @ Q[:, :r]


def _extreme_eigs_host(S, k, dense_max):
    """lambda_min side (k smallest eigenpairs) and lambda_max of S on the host.
    n <= dense_max: LAPACK like the reference's eig(full(S)) (ManiSDP_onlyunitdiag.m:50)."""
    n = S.shape[0]
    if n <= dense_max:
        Sd = S.toarray() if sp.issparse(S) else np.asarray(S)
        dS, vS = np.linalg.eigh(Sd)
        return dS, vS, int(np.sum(dS < 0))
    raise RuntimeError("host eigensolver limit exceeded; use the device escape (options['eig'] = 'device')")


def _device_escape(h, run, o, data, default_tol, default_maxit):
    """One device escape call (``run(tol, maxit)`` -> lam, V, lam_max, steps) with the convergence contract of
    ``msdp_escape_info``: a Lanczos run that hit ``maxit`` only bounds lambda_min from above, so it is repeated
    once with four times the step budget; ``certified`` tells the AL loop whether dinf may end the solve.
    ``options["escape_stats"] = True`` (every solver with a device escape shares this helper and _verify_lambda_min; off by
    default, so ``data`` keeps its fields; the timing tools set it) counts in ``data["eig_calls"]`` / ``data["eig_steps"]`` the
    calls made here and the steps they report, and in ``data["eig_verify_steps"]`` those of the cold checks."""
    tol = float(o.get("eig_tol", default_tol))
    maxit = int(o.get("eig_maxit", default_maxit))
    lam, vS, lam_max, steps = run(tol, maxit)
    nvalid, conv, res = h.escape_info()
    if not conv:
        data["eig_retries"] = data.get("eig_retries", 0) + 1
        lam, vS, lam_max, more = run(tol, 4 * maxit)
        steps += more
        nvalid, conv, res = h.escape_info()
    if o.get("escape_stats"):                             # on request (timing tools): escape calls and the steps they report -- Lanczos
        data["eig_calls"] = data.get("eig_calls", 0) + 1    # steps, or filter steps and products of the block eigen-solver with its
        data["eig_steps"] = data.get("eig_steps", 0) + int(steps)   # lambda_max run; the cold checks under "eig_verify_steps"
    if not conv:
        data["eig_unconverged"] = data.get("eig_unconverged", 0) + 1
    return lam, vS, lam_max, nvalid, conv


def _verify_lambda_min(h, run1, o, data, default_tol, default_maxit, dense_n=0):
    """The independent check behind "Optimality is reached!".  The regular escape call deflates span(Y) and starts
    from what the previous call found: fast, but its lambda_min is only as good as S*Y is small and it can stay above
    the true one.  Before dinf may end the solve -- and once at the end of a solve that did not converge, so that the
    reported dinf is the true one -- lambda_min and lambda_max are recomputed without those shortcuts:
      * affine kinds with a dense S of moderate order (dense_n <= options.verify_dense_max, default 4000): the
        reference's own eig(S) (ManiSDP_unitdiag.m:68) on the host, on the S the device holds;
      * sparse C (block eigen-solver, msdp_blockeig.hip): the subspace iteration once more from a block of hashed noise --
        no column of Y, nothing carried over from earlier calls, four times tighter tolerance;
      * otherwise plain Lanczos runs on S itself: no deflation, nothing carried over from earlier calls; the start
        vector is a hashed random combination of the columns of Y plus 5 % hashed noise (span(Y), the near-kernel of S
        at a near-stationary point, is where a lambda_min the deflated estimate missed would live).
    Returns (lambda_min, its eigenvector as an n x 1 array, lambda_max, converged).  With ``options["escape_stats"]`` the steps
    of these runs are added to ``data["eig_verify_steps"]`` (see _device_escape)."""
    t1 = time.time()
    data["eig_verifications"] = data.get("eig_verifications", 0) + 1
    if 0 < dense_n <= int(o.get("verify_dense_max", 4000)):
        S = h.get_dual_slack()
        w, V = np.linalg.eigh(0.5 * (S + S.T))
        data["eig_seconds"] += time.time() - t1
        return float(w[0]), V[:, :1], float(w[-1]), True
    h.set_option("escape_deflate", 0)
    h.set_option("escape_warm", 0)
    # block eigen-solver (sparse C): hashed noise only, no column of Y -- the cold run costs ~2400 filter steps on G81 and is
    # independent of everything the regular calls used; Lanczos path: span(Y) + 5 % noise (33 000 -> 22 000 steps on G81)
    h.set_option("escape_start_y", int(o.get("verify_start_in_span_y", 0 if h.escape_method() == 1 else 1)))
    try:
        lam, vS, lam_max, steps = run1(float(o.get("eig_tol", default_tol)), int(o.get("eig_maxit", default_maxit)))
        _, conv, _ = h.escape_info()
        if not conv:                                      # once more with four times the step budget
            lam, vS, lam_max, more = run1(float(o.get("eig_tol", default_tol)), 4 * int(o.get("eig_maxit", default_maxit)))
            steps += more
            _, conv, _ = h.escape_info()
        if o.get("escape_stats"):
            data["eig_verify_steps"] = data.get("eig_verify_steps", 0) + int(steps)
    finally:
        h.set_option("escape_deflate", 1)
        h.set_option("escape_warm", 1)
        h.set_option("escape_start_y", 0)
    data["eig_seconds"] += time.time() - t1
    return float(lam[0]), vS[:, :1], float(lam_max), conv


def _escape_rr_option(o):
    """options["escape_rr"]: where the dense algebra of the block eigen-solver's Rayleigh-Ritz stages runs -- "host" (default) or
    "device" (msdp_set_option "escape_rr" = 1: panels of 32 / 64 columns; wider panels and stages the kernel hands back stay on
    the host).  Returns the value of the device option."""
    rr = o.get("escape_rr", "host")
    if rr not in ("host", "device"):
        raise ValueError(f"options['escape_rr'] must be 'host' or 'device', not {rr!r}")
    return 1 if rr == "device" else 0


def _round_order(order, where):
    """The visiting order of a rounding's local search: "index" (rows 0 .. n-1, the default) or "color" (rows by colour class,
    set_option("round_order", 1)); anything else is a ValueError."""
    if not isinstance(order, str) or order not in ("index", "color"):
        raise ValueError(f"{where} must be 'index' or 'color', not {order!r}")
    return order


def _round_option(o):
    """options["round"] = {"trials", "sweeps", "seed", "order"}: round the solution to +1/-1 vectors on the device after the solve
    (msdp_round_hyperplane; not in the reference, so no DEFAULTS entry).  Returns None when the option is absent, else
    (trials, sweeps, seed, order) -- trials a multiple of 64 up to _lib.ROUND_MAX_TRIALS, sweeps >= 0 (0: no local search),
    order "index" (default) or "color"."""
    r = o.get("round")
    if r is None:
        return None
    if not isinstance(r, dict):
        raise ValueError(f"options['round'] must be a dict with 'trials', 'sweeps' and 'seed', not {r!r}")
    unknown = sorted(set(r) - {"trials", "sweeps", "seed", "order"})
    if unknown:
        raise ValueError(f"options['round'] has unknown fields {unknown} (known: 'trials', 'sweeps', 'seed', 'order')")
    trials, sweeps, seed = r.get("trials", 256), r.get("sweeps", 50), r.get("seed", 0)
    for name, v in (("trials", trials), ("sweeps", sweeps), ("seed", seed)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"options['round'][{name!r}] must be an integer, not {v!r}")
    if trials <= 0 or trials % 64 or trials > _lib.ROUND_MAX_TRIALS:
        raise ValueError(f"options['round']['trials'] must be a multiple of 64 in 64..{_lib.ROUND_MAX_TRIALS}, not {trials}")
    if sweeps < 0 or seed < 0:
        raise ValueError(f"options['round']['sweeps'] and ['seed'] must be >= 0, not {sweeps} and {seed}")
    if o.get("comm") is not None:
        raise ValueError("options['round'] needs a single-rank solve (no options['comm'])")
    return int(trials), int(sweeps), int(seed), _round_order(r.get("order", "index"), "options['round']['order']")


def round_unitdiag(C, Y, trials=256, sweeps=50, rng=None, R=None, order="index"):
    """Round the factor Y (n x p, unit rows) of a unit-diagonal SDP with cost C to a +1/-1 vector on the device: `trials`
    hyperplane roundings x = sign(Y r) with Gaussian r (drawn from `rng` unless R, trials x p, is given), each improved by up
    to `sweeps` sweeps of 1-opt local search; the best of them is returned.  Returns (x, value, info): x int8 of length n,
    value = x' C x, info the dict of Handle.round_hyperplane (all values, sweeps and flips per word of 64 trials).  C: sparse,
    dense, or a problems.SparsePlusLowRank.  order: "index" -- a sweep visits the rows 0 .. n-1 -- or "color": by colour class,
    one launch per colour over the whole device (sparse C only; the library refuses the other two)."""
    order = _round_order(order, "round_unitdiag: order")
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if R is None:
        R = (rng or np.random.default_rng(0)).standard_normal((int(trials), Y.shape[1]))
    from .problems import SparsePlusLowRank
    if isinstance(C, SparsePlusLowRank):
        h = _lib.Handle.onlyunitdiag_lowrank(C.Cs, C.V, C.s, pcap=max(32, Y.shape[1]))
    else:
        h = _lib.Handle.onlyunitdiag(C.tocsr() if sp.issparse(C) else np.asarray(C, dtype=np.float64), pcap=max(32, Y.shape[1]))
    try:
        h.set_point(Y)
        if order == "color":
            h.set_option("round_order", 1)
        res = h.round_hyperplane(R, sweeps=sweeps)
    finally:
        h.close()
    return res["x"], float(res["values"][res["best"]]), res


def _round_phases_option(o):
    """options["round_phases"] = {"M", "trials", "sweeps", "seed", "order"} of a complex Hermitian C: round the solution to phases
    on the device after the solve (msdp_round_phases; not in the reference, so no DEFAULTS entry).  Returns None when the option
    is absent, else (M, trials, sweeps, seed, order) -- M = 0 (the unit circle) or 2 .. _lib.ROUND_PHASES_MAX_M (the M-th roots of
    unity), trials a multiple of 64 up to _lib.ROUND_PHASES_MAX_TRIALS, sweeps >= 0 (0: no local search), order "index" (default)
    or "color"."""
    r = o.get("round_phases")
    if r is None:
        return None
    if not isinstance(r, dict):
        raise ValueError(f"options['round_phases'] must be a dict with 'M', 'trials', 'sweeps' and 'seed', not {r!r}")
    unknown = sorted(set(r) - {"M", "trials", "sweeps", "seed", "order"})
    if unknown:
        raise ValueError(f"options['round_phases'] has unknown fields {unknown} (known: 'M', 'trials', 'sweeps', 'seed', 'order')")
    M, trials, sweeps, seed = r.get("M", 0), r.get("trials", 256), r.get("sweeps", 20), r.get("seed", 0)
    for name, v in (("M", M), ("trials", trials), ("sweeps", sweeps), ("seed", seed)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"options['round_phases'][{name!r}] must be an integer, not {v!r}")
    if M != 0 and not 2 <= M <= _lib.ROUND_PHASES_MAX_M:
        raise ValueError(f"options['round_phases']['M'] must be 0 or in 2..{_lib.ROUND_PHASES_MAX_M}, not {M}")
    if trials <= 0 or trials % 64 or trials > _lib.ROUND_PHASES_MAX_TRIALS:
        raise ValueError(f"options['round_phases']['trials'] must be a multiple of 64 in 64..{_lib.ROUND_PHASES_MAX_TRIALS}, not {trials}")
    if sweeps < 0 or seed < 0:
        raise ValueError(f"options['round_phases']['sweeps'] and ['seed'] must be >= 0, not {sweeps} and {seed}")
    return int(M), int(trials), int(sweeps), int(seed), _round_order(r.get("order", "index"), "options['round_phases']['order']")


def _hermitian_factor_option(o):
    """options["hermitian_factor"] of a complex Hermitian C: "host" (default) or "device" (the rank decision, the cut and the
    widening through msdp_hfactor_gram / _rotate / _append); anything else is a ValueError."""
    mode = o.get("hermitian_factor", "host")
    if mode not in ("host", "device"):
        raise ValueError(f"options['hermitian_factor'] must be 'host' or 'device', not {mode!r}")
    return mode


def _draw_phase_R(rng, trials, p):
    """The Gaussian rows of a phase rounding: the real draw first."""
    Rr = rng.standard_normal((int(trials), int(p)))
    return Rr + 1j * rng.standard_normal((int(trials), int(p)))


def round_phases(C, Y, M=0, trials=256, sweeps=20, rng=None, R=None, order="index"):
    """Round the factor Y (n x p complex, rows of unit norm) of a complex unit-diagonal SDP with Hermitian cost C to phases on
    the device: `trials` roundings of Y r with complex Gaussian r (drawn from `rng`, the real parts first, unless R, trials x p
    complex, is given) to the unit circle (M = 0) or the M-th roots of unity, each improved by up to `sweeps` Gauss-Seidel
    sweeps of coordinate minimisation; the best of them is returned.  Returns (z, value, info): z complex of length n,
    value = z^H C z, info the dict of Handle.round_phases.  order: "index" -- a sweep visits the rows 0 .. n-1 -- or "color": by
    colour class, one launch per colour over the whole device."""
    order = _round_order(order, "round_phases: order")
    Y = np.ascontiguousarray(Y, dtype=np.complex128)
    if R is None:
        R = _draw_phase_R(rng or np.random.default_rng(0), trials, Y.shape[1])
    h = _lib.Handle.onlyunitdiag_hermitian(C, pcap=max(32, Y.shape[1]))
    try:
        h.set_point(Y)
        if order == "color":
            h.set_option("round_order", 1)
        res = h.round_phases(R, M=M, sweeps=sweeps)
    finally:
        h.close()
    return res["z"], float(res["values"][res["best"]]), res


# =============================================================== onlyunitdiag
def ManiSDP_onlyunitdiag(C, options=None, verbose=True, rng=None):
    with _host_threads():
        return _onlyunitdiag_impl(C, options, verbose, rng)


def _set_device_options(h, o):
    """options['device_options']: run-time switches of the handle (msdp_set_option), for A/B runs and tests."""
    for name, value in (o.get("device_options") or {}).items():
        h.set_option(name, int(value))


def _rows_complex(Y):               # complex oblique factor: rows of unit norm
    return Y / np.sqrt(np.sum(np.abs(Y) ** 2, axis=1, keepdims=True))


def _onlyunitdiag_impl(C, options=None, verbose=True, rng=None):
    """``[X, obj, data] = ManiSDP_onlyunitdiag(C, options)`` (reference
    src/primal/ManiSDP_onlyunitdiag.m:6).  Extra, optional option fields that the
    reference does not have: ``Y0`` (start point instead of ``randn``), ``eig``
    (``'host'`` dense LAPACK | ``'device'`` few-eigenvector escape; default by size),
    ``dense_X_max``."""
    o = dict(options or {})
    for k, v in DEFAULTS["onlyunitdiag"].items():
        o.setdefault(k, v)
    if getattr(C, "dtype", None) is not None and np.dtype(C.dtype).kind == "c":
        return _onlyunitdiag_hermitian_impl(C, o, verbose, rng)     # complex C: the Hermitian problem (real C: untouched below)
    if _round_phases_option(o) is not None or _hermitian_factor_option(o) != "host":   # (malformed values: refused by the calls)
        raise ValueError("options['round_phases'] and options['hermitian_factor'] belong to a complex Hermitian C "
                         "(a real C takes options['round'] and options['device_factor'])")
    escape_rr = _escape_rr_option(o)                       # (a bad value is refused before anything is built)
    rounding = _round_option(o)
    dense_default = int(o.get("dense_eig_default", 600))   # the host eig(S) is the default up to this order (round 6: G1, n = 800, 0.124 s with it,
                                                           # 0.047 s with the device escape + its independent check; the affine kinds switch at 400 / 600)
    dense_X_max = int(o.get("dense_X_max", 4000))
    rng = rng or np.random.default_rng(0)

    _say(verbose, "ManiSDP is starting...")
    n = C.shape[0]
    _say(verbose, f"SDP size: n = {n}, m = {n}")
    from .problems import SparsePlusLowRank, SyntheticDenseC
    comm = o.get("comm")
    pcap = max(32, int(o["p0"]) + 2 * int(o["delta"]))
    if isinstance(C, SparsePlusLowRank):
        # C = Cs + V diag(s) V' stays in its parts on the device; the dense matrix exists only for the host eigen-solver of
        # small problems.  Row-sharded low-rank terms are not implemented: the library refuses every communicator.
        if comm is not None:
            raise ValueError("a problems.SparsePlusLowRank cost needs a single-rank solve (no options['comm'])")
        if not 1 <= C.q <= _lib.LOWRANK_MAX:
            raise ValueError(f"the low-rank term has q = {C.q} columns; the device kernels hold 1 .. {_lib.LOWRANK_MAX}")
        eig_mode = o.get("eig", "host" if n <= dense_default else "device")
        Csp = C.toarray() if eig_mode in ("host", "host_sparse") else None
        h = _lib.Handle.onlyunitdiag_lowrank(C.Cs, C.V, C.s, pcap=pcap)
    elif isinstance(C, SyntheticDenseC):
        # BASELINE config 5: every rank generates its rows of the dense C on the device; the matrix never exists on the host
        # (only the host eigen-solver of small test problems asks for it)
        eig_mode = o.get("eig", "host" if (n <= dense_default and comm is None) else "device")
        Csp = C.toarray() if eig_mode == "host" else None
        nr, rk = (1, 0) if comm is None else ((int(comm[1]), int(comm[2])) if comm[0] == "local" else (int(comm[0]), int(comm[1])))
        h = _lib.Handle.dense_synthetic(n, C.seed, nranks=nr, rank=rk, pcap=pcap)
    else:
        Csp = C.tocsr() if sp.issparse(C) else np.asarray(C, dtype=np.float64)
        eig_mode = o.get("eig", "host" if n <= dense_default else "device")
        h = _lib.Handle.onlyunitdiag(Csp, pcap=pcap)
    if comm is not None:
        eig_mode = "device"

    def setup():
        # options['comm'] = (nranks, rank, unique_id): rows of the factor and of C sharded over the ranks (msdp_comm_init); the
        # host loop then runs replicated -- same start point (pass Y0 or seed rng identically), same data, same decisions on
        # every rank; the escape runs replicated on a full copy of the sparse C (device eigen-solver only)
        if comm is not None:
            if not (sp.issparse(Csp) or isinstance(C, SyntheticDenseC)):
                raise ValueError("row-sharded solves need a sparse C or a problems.SyntheticDenseC")
            _join_comm(h, comm)
            if o.get("halo_exchange"):                     # only the rows this rank's rows of C reference travel before S*U
                h.set_option("halo_exchange", 1)
        if "escape_method" in o:                           # 0 auto, 1 Lanczos, 2 block eigen-solver also below its size threshold
            h.set_option("escape_method", int(o["escape_method"]))
        if escape_rr:
            h.set_option("escape_rr", escape_rr)
        _set_device_options(h, o)

    def finish(run):
        if eig_mode == "device":
            run.data["escape_rr_stages"] = h.ritz_stages()     # Rayleigh-Ritz stages: (device, host, host after fallback)
        if rounding is not None and run.obj is not None:       # options["round"]: +1/-1 vectors from the evaluated point
            trials, sweeps, seed, order = rounding
            h.set_point(run.Y)
            if order == "color":                               # (refused by the library for a dense or a low-rank C)
                h.set_option("round_order", 1)
            res = h.round_hyperplane(np.random.default_rng(seed).standard_normal((trials, run.Y.shape[1])), sweeps=sweeps)
            run.data["round"] = {"x": res["x"], "value": float(res["values"][res["best"]]), "values": res["values"],
                                 "best": res["best"], "info": res["info"]}

    Y = o.get("Y0", None)
    if Y is None:                                          # trustregions.m:390-392 -> M.rand()
        Y = rng.standard_normal((n, int(o["p0"])))
        Y /= np.sqrt(np.sum(Y * Y, axis=1, keepdims=True))
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    # Rank decision, rank cut and widening of the factor on the device (msdp_factor_gram / _rotate / _append): the factor
    # stays resident between the trustregions() calls and comes to the host once, when the solve ends.  Default with the
    # device escape (large n); the line-search variant keeps the host form (its direction U is a host array anyway).
    device_factor = bool(o.get("device_factor", eig_mode == "device" and o["line_search"] != 1))
    get_z = h.get_z_all if comm is not None else h.get_z    # :46-47  z = sum((Y*C).*Y)
    kind = _Manifold(
        evaluate=lambda blocks: _obj_sum_z(get_z()),       # :48
        host_S=lambda z, Lam: (Csp - sp.diags(z)) if sp.issparse(Csp) else (Csp - np.diag(z)),   # :49
        fetch=h.get_point_all if comm is not None else h.get_point, normalise=_rows,
        device=(h.factor_gram, h.factor_rotate, lambda V, alpha: h.factor_append(V, alpha, normalize=True)) if device_factor else None,
        setup=setup, finish=finish, verify_at_end=True, reshape_last=True, line_search=o["line_search"] == 1 and not device_factor)
    run = _manifold_loop(h, o, kind, Y, int(o["p0"]), eig_mode, verbose)
    Y, z, S, data = run.Y, run.z, run.S, run.data
    if S is None and Csp is not None and sp.issparse(Csp) and z is not None:
        S = Csp - sp.diags(z)                              # :49 (kept sparse; the reference returns full(S))
    if S is None and isinstance(C, SparsePlusLowRank) and z is not None and n <= dense_X_max:
        S = C.toarray() - np.diag(z)                       # the implicit C is formed only below dense_X_max (None above)
    data.update({"Y": Y, "S": S, "z": z, "dinf": run.dinf, "gradnorm": run.gradnorm,
                 "time": time.time() - run.t0, "p": Y.shape[1],
                 "X": (Y @ Y.T if n <= dense_X_max else None)})   # :45,86
    return Y, run.obj, data


def _onlyunitdiag_hermitian_impl(C, o, verbose, rng):
    """ManiSDP_onlyunitdiag for a complex Hermitian C:  min <C, X>  s.t. X Hermitian PSD, X_ii = 1  (phase synchronisation,
    unimodular quadratic programmes; manopt's elliptope_SDP_complex).  The algorithm, the defaults and the option names are
    those of ManiSDP_onlyunitdiag.m; the algebra is complex: the factor Y is n x p complex with rows of unit modulus sum,
    z = Re sum((C Y) .* conj(Y), 2), the rank decision comes from Y^H Y, the cut is Y Q(:, 1:r), widening is [Y, alpha v] with
    the rows renormalised, X = Y Y^H.  ``o``: the options with the defaults filled in.  Every refusal comes before the first
    library call.  Extra option fields: ``hermitian_factor`` ("host" | "device": the rank decision, the cut and the widening through
    msdp_hfactor_gram / _rotate / _append, the factor resident between the trustregions() calls) and ``round_phases`` = {"M",
    "trials", "sweeps", "seed"} (msdp_round_phases on the evaluated point: ``data["round"]`` = z, value, values, best, info, and k
    for M >= 2) and ``escape_method`` (device escape: 0 / 1 = Lanczos on the real view, the default; 2 = the block eigen-solver
    on a complex panel where n >= 256; ``data["escape_method"]`` reports what the last escape call ran).  ``data["factor_seconds"]``: what the factor costs between the trustregions() calls -- its transfers (after the
    first upload), the rank decision, the cut and the widening."""
    Csp = _lib.hermitian_csc(sp.csc_matrix(C) if not sp.issparse(C) else C).tocsr()   # ValueError unless C == C^H exactly
    for name, what in (("round", "+1/-1 rounding belongs to the real problem"), ("comm", "a single-rank solve is needed")):
        if o.get(name) is not None:
            raise ValueError(f"options[{name!r}] is not available for a complex Hermitian C: {what}")
    if o["line_search"] == 1:
        raise ValueError("options['line_search'] = 1 is not available for a complex Hermitian C")
    if o.get("device_factor"):
        raise ValueError("options['device_factor'] is not available for a complex Hermitian C: its device re-shaping is options['hermitian_factor'] = 'device'")
    rounding = _round_phases_option(o)
    device_factor = _hermitian_factor_option(o) == "device"
    dense_X_max = int(o.get("dense_X_max", 4000))
    rng = rng or np.random.default_rng(0)
    n = Csp.shape[0]
    eig_mode = o.get("eig", "host" if n <= int(o.get("dense_eig_default", 600)) else "device")
    if eig_mode not in ("host", "device"):
        raise ValueError(f"options['eig'] must be 'host' or 'device' for a complex Hermitian C, not {eig_mode!r}")
    _say(verbose, "ManiSDP is starting...")
    _say(verbose, f"SDP size: n = {n}, m = {n} (complex Hermitian)")
    p = int(o["p0"])
    Y = o.get("Y0", None)
    if Y is None:
        Y = rng.standard_normal((n, p)) + 1j * rng.standard_normal((n, p))
        Y /= np.sqrt(np.sum(np.abs(Y) ** 2, axis=1, keepdims=True))
    Y = np.ascontiguousarray(Y, dtype=np.complex128)
    p = Y.shape[1]
    h = _lib.Handle.onlyunitdiag_hermitian(Csp, pcap=max(32, p + 2 * int(o["delta"])))

    def setup():
        if "escape_method" in o:                           # 0 auto and 1: Lanczos on the real view; 2: block eigen-solver on a complex panel (n >= 256)
            h.set_option("escape_method", int(o["escape_method"]))
        _set_device_options(h, o)

    def finish(run):
        if rounding is not None and run.obj is not None:       # options["round_phases"]: phases from the evaluated point
            M, trials, sweeps, seed, order = rounding
            h.set_point(run.Y)
            if order == "color":
                h.set_option("round_order", 1)
            res = h.round_phases(_draw_phase_R(np.random.default_rng(seed), trials, run.Y.shape[1]), M=M, sweeps=sweeps)
            run.data["round"] = {"z": res["z"], "value": float(res["values"][res["best"]]), "values": res["values"],
                                 "best": res["best"], "info": res["info"]}
            if M:
                run.data["round"]["k"] = res["k"]

    kind = _Manifold(
        evaluate=lambda blocks: _obj_sum_z(h.get_z()),     # :46-48  z = Re sum((C Y) .* conj(Y), 2)
        host_S=lambda z, Lam: Csp - sp.diags(z),           # (eigh of the complex S)
        fetch=h.get_point, normalise=_rows_complex, host_gram=lambda Y: Y.conj().T @ Y,   # :52-54 from Y^H Y
        device=(h.hfactor_gram, h.hfactor_rotate, h.hfactor_append) if device_factor else None,
        setup=setup, finish=finish, reshape_last=True)
    run = _manifold_loop(h, o, kind, Y, p, eig_mode, verbose)
    Y, z, data = run.Y, run.z, run.data
    data.update({"Y": Y, "S": (Csp - sp.diags(z)) if z is not None else None, "z": z, "dinf": run.dinf, "gradnorm": run.gradnorm,
                 "factor_seconds": run.factor_seconds,
                 "time": time.time() - run.t0, "p": Y.shape[1], "X": (Y @ Y.conj().T if n <= dense_X_max else None)})
    return Y, run.obj, data


# =============================================================== onlyunitblockdiag
def onlyunitblockdiag_defaults(d):
    """The option defaults of ManiSDP_onlyunitblockdiag for block order d: those of ManiSDP_onlyunitdiag except p0 = d + 2 and
    delta = d (see its docstring)."""
    return dict(DEFAULTS["onlyunitdiag"], p0=int(d) + 2, delta=int(d))


def _polar_blocks(Y, d):
    """Every block of d rows replaced by its polar factor u v' (the nearest block with orthonormal rows)."""
    u, _, vt = np.linalg.svd(Y.reshape(Y.shape[0] // d, d, Y.shape[1]), full_matrices=False)
    return np.ascontiguousarray((u @ vt).reshape(Y.shape))


def _block_factor_option(o, what):
    """options["block_factor"] of the two block kinds: "host" (default) or "device"; anything else is a ValueError."""
    mode = o.get("block_factor", "host")
    if mode not in ("host", "device"):
        raise ValueError(f"options['block_factor'] must be 'host' or 'device' for the {what} problem, not {mode!r}")
    return mode


def _block_escape_method_option(o, what):
    """options["escape_method"] of the two block kinds: None (not given) or 0 / 1 / 2; anything else is a ValueError."""
    if "escape_method" not in o:
        return None
    m = o["escape_method"]
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) not in (0, 1, 2):
        raise ValueError(f"options['escape_method'] must be 0, 1 or 2 for the {what} problem, not {m!r}")
    return int(m)


def _round_blocks_option(h, d, Y_eval, data):
    """options["round_blocks"]: data["R"] (and data["t"] of a pose-graph handle) from Handle.round_blocks at the evaluated
    point, which both settings of block_factor leave resident when their loop ends; the host functions of problems.py where
    the device reports degenerate blocks (data["round_fallback"] = True)."""
    from . import problems
    R, t, _, ndeg = h.round_blocks()
    data["round_fallback"] = ndeg > 0
    if ndeg > 0:
        if h.efree:
            R, t = problems.round_poses(Y_eval, d)
        else:
            R = problems.round_rotations(Y_eval, d)
    data["R"] = R
    if h.efree:
        data["t"] = t


def ManiSDP_onlyunitblockdiag(C, d, options=None, verbose=True, rng=None):
    """``min <C, X>  s.t. X PSD of order N = n d, X_[ii] = I_d`` for d = 2 or 3 (synchronisation over O(d) / SO(d): rotation
    averaging, pose graphs; problems.rotation_synchronization), on the stacked Stiefel manifold of the factor: blocks of d
    consecutive rows of Y (N x p) are orthonormal, manopt's stiefelstackedfactory(n, d, p).  No multipliers and no penalty: the
    constraint is the manifold, as X_ii = 1 is for ManiSDP_onlyunitdiag, whose loop, option names and printed protocol this
    follows.  Returns (Y, obj, data); ``data["Lambda"]`` holds the multiplier blocks (n, d, d), S = C - blockdiag(Lambda).

    Defaults: those of ManiSDP_onlyunitdiag except ``p0 = d + 2`` and ``delta = d`` -- both are choices (a start above the
    rank-d solution of the noise-free problem; one escape direction per row of a block), neither is measured.  The random
    start takes the Q factors of randn(p, d).  lambda_min / lambda_max of S come from the host for N <= dense_eig_default and
    from the device escape, with the independent cold check before "Optimality is reached!", above that (options["eig"]).
    The rank decision is that of the reference (Y'Y); the factor is cut to r columns only when d <= r <= p - 1, widened by
    [Y, alpha V(:, 1:nne)], and after either step every block is re-orthonormalised on the host by its polar factor.
    ``options["block_persist"] = True`` runs the tCG of every trust-region iteration as one persistent launch where the handle
    is eligible (p <= 32; msdp_set_option "block_persist"), the generic trips elsewhere; default False.
    ``options["block_factor"] = "device"`` keeps the factor on the device between the trustregions() calls: the rank decision
    from Handle.blockfactor_gram, the cut, the widening and the re-orthonormalisation by blockfactor_rotate / _append, one
    set_point per solve; an iteration whose call reports degenerate blocks or exceeds the handle's capacity takes the host
    steps (``data["factor_host_fallbacks"]``; ``data["factor_device_calls"]`` counts the device calls).  Default ``"host"``.
    ``data["factor_seconds"]`` is the wall time of the re-shapes on either path: rank decision, cut, widening, polar factors
    and the transfers only that path needs (host: get_point and the next set_point; device: the Gram matrix).
    ``options["round_blocks"] = True`` fills ``data["R"]`` (n, d, d) from Handle.round_blocks at the evaluated point before the
    handle closes (problems.round_rotations where the device reports degenerate blocks: ``data["round_fallback"]``).
    ``options["escape_method"]`` selects the device escape (``eig = "device"``), the independent cold check included: 0 (default)
    and 1 = single-vector Lanczos runs over the one-thread-per-block product; 2 = the Chebyshev-filtered block eigen-solver on
    block storage where N = n d >= 256 and the factor is at most 112 columns wide (Lanczos otherwise), which returns whole eigenspaces where an eigenvalue of S is
    multiple (d = 2: every one is double).  ``data["escape_method"]`` reports what the last escape call ran (1 = block); any
    other value raises ValueError before a handle is created.
    ``line_search = 1``, ``device_factor``, ``round``, ``comm`` and ``precon`` raise ValueError before the library is loaded."""
    with _host_threads():
        return _onlyunitblockdiag_impl(C, d, options, verbose, rng)


def _block_kind(h, o, d, device, evaluate, host_S, polar, setup, rerun=False):
    """The _Manifold of the two block kinds: what differs between them is how a point is evaluated, the host S, which rows the
    polar factors re-orthonormalise, the options of the set-up, and the pose-graph kind's rerun."""
    def finish(run):
        if run.obj is None:
            return
        if device:                                         # the multiplier blocks once, at the evaluated point
            run.Lam = h.get_blockmult()
        if o.get("round_blocks"):
            _round_blocks_option(h, d, run.Y, run.data)

    return _Manifold(evaluate=evaluate, host_S=host_S, fetch=h.get_point, normalise=lambda Y: polar(Y, d),
                     device=(h.blockfactor_gram, h.blockfactor_rotate, h.blockfactor_append) if device else None,
                     setup=setup, finish=finish, min_rank=d, polar_cut=True, max_width=256, rerun=rerun)


def _block_kind_data(run, S, N, dense_X_max):
    """The data fields the two block kinds share."""
    Y = run.Y
    return {"Y": Y, "S": S, "z": run.z, "Lambda": run.Lam, "dinf": run.dinf, "gradnorm": run.gradnorm, "rank": run.r,
            "factor_device_calls": run.device_calls, "factor_host_fallbacks": run.host_fallbacks, "factor_seconds": run.factor_seconds,
            "time": time.time() - run.t0, "p": Y.shape[1], "X": (Y @ Y.T if N <= dense_X_max else None)}


def _onlyunitblockdiag_impl(C, d, options, verbose, rng):
    d = int(d)
    if d not in (2, 3):
        raise ValueError(f"the block order d must be 2 or 3, not {d}")
    o = dict(options or {})
    for k, v in onlyunitblockdiag_defaults(d).items():
        o.setdefault(k, v)
    for name, what in (("round", "+1/-1 rounding belongs to the unit-diagonal problem (problems.round_rotations rounds rotations)"),
                       ("comm", "a single-rank solve is needed")):
        if o.get(name) is not None:
            raise ValueError(f"options[{name!r}] is not available for the unit-block-diagonal problem: {what}")
    if o["line_search"] == 1:
        raise ValueError("options['line_search'] = 1 is not available for the unit-block-diagonal problem")
    if o.get("precon") is not None:
        raise ValueError("options['precon'] is not available for the unit-block-diagonal problem: the diagonal blocks of its cost "
                         "matrix are zero (block-Jacobi preconditioning is ManiSDP_posegraph's)")
    if o.get("device_factor"):
        raise ValueError("options['device_factor'] is not available for the unit-block-diagonal problem: the rank cut stays on the host")
    device = _block_factor_option(o, "unit-block-diagonal") == "device"
    escape_method = _block_escape_method_option(o, "unit-block-diagonal")
    if C.shape[0] != C.shape[1] or C.shape[0] % d:
        raise ValueError(f"the cost matrix must be square of an order that is a multiple of d = {d}, not {C.shape}")
    dense_X_max = int(o.get("dense_X_max", 4000))
    N = C.shape[0]
    nb = N // d
    eig_mode = o.get("eig", "host" if N <= int(o.get("dense_eig_default", 600)) else "device")
    if eig_mode not in ("host", "device"):
        raise ValueError(f"options['eig'] must be 'host' or 'device' for the unit-block-diagonal problem, not {eig_mode!r}")
    p = int(o["p0"])
    Y = o.get("Y0", None)
    if Y is None and p < d:
        raise ValueError(f"options['p0'] = {p} is below the block order d = {d}")
    Csp = sp.csr_matrix(C, dtype=np.float64)
    rng = rng or np.random.default_rng(0)
    _say(verbose, "ManiSDP is starting...")
    _say(verbose, f"SDP size: n = {N}, m = {nb * d * (d + 1) // 2} ({nb} blocks of order {d})")
    if Y is None:
        Y = np.empty((nb, d, p))
        for i in range(nb):                                # stiefelstackedfactory.m:142-150
            Y[i] = np.linalg.qr(rng.standard_normal((p, d)))[0].T
        Y = Y.reshape(N, p)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    p = Y.shape[1]
    h = _lib.Handle.onlyunitblockdiag(Csp, d, pcap=min(256, max(32, p + 2 * int(o["delta"]))))

    def setup():
        if o.get("block_persist"):                         # the tCG of a TR iteration in one persistent launch where it applies
            h.set_option("block_persist", 1)
        if escape_method is not None:                      # 0 auto and 1: Lanczos; 2: block eigen-solver on block storage (N >= 256)
            h.set_option("escape_method", escape_method)
        _set_device_options(h, o)

    def evaluate(blocks):
        if not blocks:
            return _obj_sum_z(h.get_z())                   # the diagonals alone; the blocks once, at the end
        Lam = h.get_blockmult()                            # Lambda_i = sym((C Y)_i Y_i')
        z = np.ascontiguousarray(np.diagonal(Lam, axis1=1, axis2=2)).ravel()
        return z, Lam, float(np.sum(z)), None

    host_S = lambda z, Lam: Csp - sp.block_diag(list(Lam), format="csr")
    run = _manifold_loop(h, o, _block_kind(h, o, d, device, evaluate, host_S, _polar_blocks, setup), Y, p, eig_mode, verbose)
    run.data.update(_block_kind_data(run, host_S(None, run.Lam) if run.Lam is not None else None, N, dense_X_max))
    return run.Y, run.obj, run.data


# =============================================================== posegraph
def posegraph_defaults(d):
    """The option defaults of ManiSDP_posegraph for dimension d: those of ManiSDP_onlyunitblockdiag (p0 = d + 2, delta = d)."""
    return onlyunitblockdiag_defaults(d)


def _polar_rotation_rows(Y, d):
    """The d rotation rows of every block of d + 1 rows replaced by their polar factor; the free rows as they are."""
    A = np.array(Y.reshape(Y.shape[0] // (d + 1), d + 1, Y.shape[1]))
    u, _, vt = np.linalg.svd(A[:, :d, :], full_matrices=False)
    A[:, :d, :] = u @ vt
    return np.ascontiguousarray(A.reshape(Y.shape))


def _pad_blocks(Lam):
    """blockdiag(Lambda_i (+) 0): the d x d multiplier blocks as a sparse matrix of order n (d + 1)."""
    nb, d, _ = Lam.shape
    P = np.zeros((nb, d + 1, d + 1))
    P[:, :d, :d] = Lam
    return sp.block_diag(list(P), format="csr")


def ManiSDP_posegraph(C, d, options=None, verbose=True, rng=None):
    """``min <C, X>  s.t. X PSD of order N = n (d + 1), (X_[ii])_{1..d,1..d} = I_d`` for d = 2 or 3: the SDP of pose-graph
    optimisation (synchronisation over SE(d), the non-marginalised form of SE-Sync / Cartan-Sync; problems.pose_graph).  Block
    i of the factor Y (N x p) is d orthonormal rows (the rotation) followed by one free row (the position): the product of
    manopt's stiefelstackedfactory(n, d, p) and euclideanfactory(n, p).  C symmetric and bounded below on the free rows (a
    pose-graph C is PSD).  The loop, option names and printed protocol follow ManiSDP_onlyunitblockdiag, except:

    * the start has the Q factors of randn(p, d) in the rotation rows and zeros in the free rows; ``p0 = d + 2``, ``delta = d``
      (choices, not measured);
    * ``obj = 2 cost = <C, Y Y'>`` from the device, not the dual value ``sum tr Lambda``: the two differ by ``sum <g_i, tau_i>``
      away from a critical point.  ``gap = |obj - dual| / (1 + |obj| + |dual|)`` is printed in the iteration line and returned
      in ``data["gap"]`` (``data["dual"]`` the dual value);
    * the loop stops only when ``max(dinf, gap) < tol`` and the cold check certifies.  With ``dinf < tol <= gap`` the point is
      not stationary (the translation part is ill-conditioned: trustregions() may end at its iteration cap with S PSD already),
      and trustregions() runs again on the same factor, without a cut or widening;
    * the polar re-orthonormalisation after a cut or widening touches the rotation rows only.

    Returns (Y, obj, data); ``data["Lambda"]`` holds the multiplier blocks (n, d, d), S = C - blockdiag(Lambda_i (+) 0).  For a
    pose-graph C the global shift is in the null space of S, so lambda_min of a certified point is 0.
    ``options["block_persist"]`` as for ManiSDP_onlyunitblockdiag.
    ``options["precon"] = "blockjacobi"`` runs every tCG with the block-Jacobi preconditioner M_i = sym(C_[ii]) of the diagonal
    blocks (msdp_set_option "precon": the preconditioned branch of tCG.m, the trust region in the M-norm); default None, the
    identity.  With it the handle runs the generic trips also under ``block_persist``.  Any other value raises ValueError
    before the library is loaded; a block the library cannot invert surfaces as its own MsdpError.
    ``options["block_factor"]`` and ``options["round_blocks"]`` as for ManiSDP_onlyunitblockdiag (the polar factors are those
    of the rotation rows; a rerun leaves the resident factor where it is; ``data["R"]`` and ``data["t"]``, from
    problems.round_poses on a fallback).
    ``options["escape_method"]`` as for ManiSDP_onlyunitblockdiag (0 / 1 = Lanczos, the default; 2 = the block eigen-solver on
    block storage where N = n (d + 1) >= 256; ``data["escape_method"]`` reports what ran; any other value raises ValueError
    before a handle is created).
    ``line_search = 1``, ``device_factor``, ``round`` and ``comm`` raise ValueError before the library is loaded."""
    with _host_threads():
        return _posegraph_impl(C, d, options, verbose, rng)


def _posegraph_impl(C, d, options, verbose, rng):
    d = int(d)
    if d not in (2, 3):
        raise ValueError(f"the dimension d must be 2 or 3, not {d}")
    B = d + 1
    o = dict(options or {})
    for k, v in posegraph_defaults(d).items():
        o.setdefault(k, v)
    for name, what in (("round", "poses are rounded on the host (problems.round_poses)"), ("comm", "a single-rank solve is needed")):
        if o.get(name) is not None:
            raise ValueError(f"options[{name!r}] is not available for the pose-graph problem: {what}")
    if o["line_search"] == 1:
        raise ValueError("options['line_search'] = 1 is not available for the pose-graph problem")
    if o.get("precon") not in (None, "blockjacobi"):
        raise ValueError(f"options['precon'] must be None or 'blockjacobi' for the pose-graph problem, not {o.get('precon')!r}")
    if o.get("device_factor"):
        raise ValueError("options['device_factor'] is not available for the pose-graph problem: the rank cut stays on the host")
    device = _block_factor_option(o, "pose-graph") == "device"
    escape_method = _block_escape_method_option(o, "pose-graph")
    if C.shape[0] != C.shape[1] or C.shape[0] % B:
        raise ValueError(f"the cost matrix must be square of an order that is a multiple of d + 1 = {B}, not {C.shape}")
    dense_X_max = int(o.get("dense_X_max", 4000))
    N = C.shape[0]
    nb = N // B
    eig_mode = o.get("eig", "host" if N <= int(o.get("dense_eig_default", 600)) else "device")
    if eig_mode not in ("host", "device"):
        raise ValueError(f"options['eig'] must be 'host' or 'device' for the pose-graph problem, not {eig_mode!r}")
    p = int(o["p0"])
    Y = o.get("Y0", None)
    if Y is None and p < d:
        raise ValueError(f"options['p0'] = {p} is below the dimension d = {d}")
    Csp = sp.csr_matrix(C, dtype=np.float64)
    rng = rng or np.random.default_rng(0)
    _say(verbose, "ManiSDP is starting...")
    _say(verbose, f"SDP size: n = {N}, m = {nb * d * (d + 1) // 2} ({nb} blocks of order {B}, the leading {d} x {d} part pinned)")
    if Y is None:
        Y = np.zeros((nb, B, p))
        for i in range(nb):                                # stiefelstackedfactory.m:142-150; the free rows start at zero
            Y[i, :d] = np.linalg.qr(rng.standard_normal((p, d)))[0].T
        Y = Y.reshape(N, p)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    p = Y.shape[1]
    h = _lib.Handle.posegraph(Csp, d, pcap=min(256, max(32, p + 2 * int(o["delta"]))))

    def setup():
        if o.get("block_persist"):                         # the tCG of a TR iteration in one persistent launch where it applies
            h.set_option("block_persist", 1)
        if o.get("precon") == "blockjacobi":               # block-Jacobi preconditioned tCG (msdp_set_option "precon"); a refusal
            h.set_option("precon", 1)                      # (a diagonal block without a Cholesky factor) is the library's own error
        if escape_method is not None:                      # 0 auto and 1: Lanczos; 2: block eigen-solver on block storage (N >= 256)
            h.set_option("escape_method", escape_method)
        _set_device_options(h, o)

    def evaluate(blocks):
        Lam = h.get_blockmult() if blocks else None        # Lambda_i = sym(G_i Y_i'), d x d
        z = h.get_z()                                      # its diagonals, 0 in the free-row entries
        dual = float(np.sum(z))
        obj = 2.0 * h.cost()                               # <C, Y Y'> = dual + sum <g_i, tau_i>
        return z, Lam, obj, abs(obj - dual) / (1.0 + abs(obj) + abs(dual))

    host_S = lambda z, Lam: Csp - _pad_blocks(Lam)
    kind = _block_kind(h, o, d, device, evaluate, host_S, _polar_rotation_rows, setup, rerun=True)
    run = _manifold_loop(h, o, kind, Y, p, eig_mode, verbose)
    run.data.update(_block_kind_data(run, host_S(None, run.Lam) if run.Lam is not None else None, N, dense_X_max))
    run.data.update({"gap": run.gap, "dual": float(np.sum(run.z)) if run.z is not None else None, "reruns": run.reruns})
    return run.Y, run.obj, run.data


def _line_search(h, U):
    """line_search(Y, U) (ManiSDP_onlyunitdiag.m:103-115, ManiSDP_unitdiag.m:138-150,
    ManiSDP_unittrace.m:142-154) with every co() evaluated on the device; leaves the
    accepted trial point resident."""
    alpha = 1.0
    cost0 = h.linesearch_cost(None, 0.0)
    i = 1
    val = h.linesearch_cost(U, alpha)
    while i <= 15 and val - cost0 > -1e-3:
        alpha = 0.8 * alpha
        val = h.linesearch_cost(U, alpha)
        i += 1
    h.linesearch_accept()


def _count_rtr(data, st):
    """The counters of one trustregions() call, added to those of the solve."""
    data["rtr_seconds"] += st.seconds
    data["hessvecs"] += st.hessvecs
    data["cost_evals"] += st.cost_evals
    data["rejected"] += st.rejected


# ============================================================ one outer loop for the four manifold-only kinds
# ManiSDP_onlyunitdiag with a real and with a complex Hermitian C, ManiSDP_onlyunitblockdiag and ManiSDP_posegraph have no multipliers
# and no penalty -- the constraint is the manifold -- and share the loop of ManiSDP_onlyunitdiag.m:38-84: trustregions(), z or Lambda
# and the objective, lambda_min / lambda_max of S with the independent check, the rank decision, the stop and slow-progress tests,
# the cut and the widening.  _manifold_loop holds it once; a kind states what is its own in a _Manifold record.
def _obj_sum_z(z):
    """The evaluation of the kinds whose objective is the dual value: (z, no multiplier blocks, obj = sum z, no gap)."""
    return z, None, float(np.sum(z)), None


class _Manifold:
    """What _manifold_loop needs to know of a kind.
    ``evaluate(blocks)`` -> (z, Lambda or None, obj, gap or None) at the resident point after trustregions(); ``blocks``: the host
    needs the multiplier blocks of this evaluation (it builds S, or holds the factor).  A kind with a gap ends on max(dinf, gap)
    and prints it.  ``host_S(z, Lambda)``: S for the host eigen-solver.
    The factor: ``fetch()`` brings it to the host; ``host_gram(Y)``: its Gram matrix for the rank decision (None: Y'Y);
    ``normalise(Y)``: back onto the manifold after the widening; ``device``: None = the factor is re-shaped on the host and
    uploaded before every trustregions() call, else (gram, rotate, append) of the handle = it stays resident and is re-shaped
    there; rotate / append may answer with a count of degenerate blocks, which means the point is unchanged.
    ``setup()`` / ``finish(run)``: the handle's options before the loop, the kind's own work at its end (rounding, a last fetch)
    -- both run under the loop's ``finally: close``.
    ``min_rank``: the cut happens only for min_rank <= r <= p - 1 (block kinds: d orthonormal rows need d columns).
    ``polar_cut``: the factor is normalised after the cut as well (block kinds; a cut leaves unit-diagonal rows as they are).
    ``max_width``: widest factor the handle takes (block kinds: 256), beyond it RuntimeError.
    ``verify_at_end``: a solve that stopped on "Slow progress" gets the independent lambda_min check once more (real C only).
    ``reshape_last``: the last pass re-shapes the resident factor like any other (unit-diagonal kinds); False: it stops before.
    ``rerun``: with dinf < tol <= gap trustregions() runs again on the same factor, no cut, no widening (pose-graph only).
    ``line_search``: the widening hands its directions to line_search() instead of appending them (real C, host factor only)."""

    def __init__(self, evaluate, host_S, fetch, normalise, host_gram=None, device=None, setup=None, finish=None, min_rank=0,
                 polar_cut=False, max_width=None, verify_at_end=False, reshape_last=False, rerun=False, line_search=False):
        self.evaluate, self.host_S, self.fetch, self.normalise, self.host_gram = evaluate, host_S, fetch, normalise, host_gram
        self.device, self.setup, self.finish, self.min_rank, self.polar_cut, self.max_width = device, setup, finish, min_rank, polar_cut, max_width
        self.verify_at_end, self.reshape_last, self.rerun, self.line_search = verify_at_end, reshape_last, rerun, line_search


_MANIFOLD_LINE = "Iter %d, obj:%0.8f, dinf:%0.1e, r:%d, p:%d, time:%0.2fs"
_MANIFOLD_LINE_GAP = "Iter %d, obj:%0.8f, dinf:%0.1e, gap:%0.1e, r:%d, p:%d, time:%0.2fs"


def _manifold_reshape(k, o, run, Y, p, Q, e, r, vS, nne):
    """The factor between two trustregions() calls (ManiSDP_onlyunitdiag.m:70-83): cut to r columns where the kind allows it,
    widened by alpha vS(:, 1:nne) and normalised.  On the device (msdp_factor_* / msdp_hfactor_* / msdp_blockfactor_*) the new
    point stays resident and (None, None, p) is returned.  A device call that reports degenerate blocks or exceeds the handle's
    capacity hands this iteration to the host: the factor comes down as the device holds it (cut or not) and takes the host
    steps.  The host returns (Y, U, p) for set_point, U the direction of line_search() or None."""
    cut = k.min_rank <= r <= p - 1
    if k.device is not None:
        _, rotate, append = k.device
        try:
            ok = True
            if cut:                                        # :70-73
                ok = not rotate(Q[:, :r])
                if ok:
                    cut, p = False, r
                    run.device_calls += 1
            if ok:
                if k.max_width is not None and p + nne > k.max_width:
                    raise RuntimeError(f"the factor width would exceed the device's {k.max_width} columns (p = {p}, {nne} more)")
                if not append(vS[:, :nne], float(o["alpha"])):   # :78-83
                    run.device_calls += 1
                    return None, None, p + nne
        except _lib.MsdpError as err:                      # wider than the handle's buffers: re-enter through set_point
            if "allocated capacity" not in str(err):
                raise
        run.host_fallbacks += 1
        Y = k.fetch()
        if cut:
            Y = _cut_on_host(k, Y, Q, e, r)
        Y = np.ascontiguousarray(k.normalise(np.hstack([Y, o["alpha"] * vS[:, :nne]])))
        return Y, None, Y.shape[1]
    if cut:                                              # :70-73
        Y, p = _cut_on_host(k, Y, Q, e, r), r
    if k.max_width is not None and p + nne > k.max_width:
        raise RuntimeError(f"the factor width would exceed the device's {k.max_width} columns (p = {p}, {nne} more)")
    U = None
    if k.line_search:                                      # :75-80
        U = np.hstack([np.zeros((Y.shape[0], p)), vS[:, :nne]])
        Y = np.hstack([Y, np.zeros((Y.shape[0], nne))])
    else:
        Y = k.normalise(np.hstack([Y, o["alpha"] * vS[:, :nne]]))   # :82-83
    return np.ascontiguousarray(Y), U, p + nne


def _cut_on_host(k, Y, Q, e, r):
    Y = _rank_cut(Y, Q, e, r)
    return k.normalise(Y) if k.polar_cut else Y


def _manifold_loop(h, o, k, Y, p, eig_mode, verbose):
    """The outer loop of the manifold-only kinds on the handle `h` from the start point Y of width p; closes `h`.  Returns the
    state of the solve: obj, dinf, gap, gradnorm, z, Lam, S (the host's, where it built one), r of the last evaluation, Y = the
    point they belong to, data, t0 and the counters device_calls, host_fallbacks, reruns and factor_seconds (the wall time of the
    factor between the trustregions() calls: its transfers after the first upload, the rank decision, the cut and the widening)."""
    from types import SimpleNamespace
    tol, delta, maxiter, theta = o["tol"], int(o["delta"]), int(o["AL_maxiter"]), float(o["theta"])
    dense_max = int(o.get("dense_eig_max", 3000))          # the host eig(S) is allowed up to this order (options['eig'] = 'host')
    device = k.device is not None
    data = {"status": 0, "hessvecs": 0, "cost_evals": 0, "rejected": 0, "rtr_seconds": 0.0, "eig_seconds": 0.0, "log": []}
    run = SimpleNamespace(obj=None, dinf=None, gap=None, gradnorm=None, z=None, Lam=None, S=None, r=None, Y=Y, data=data,
                          t0=time.time(), device_calls=0, host_fallbacks=0, reruns=0, factor_seconds=0.0)
    t0 = run.t0
    obj = dinf = gap = res = res0 = U = None
    certified = last_verified = True
    resident = False
    escape = lambda kk: (lambda tol, maxit: h.escape_eigs(kk, tol=tol, maxit=maxit))

    def verify():
        # the regular escape call is warm-started (columns of Y and the previous call's vectors in its start block, or
        # span(Y) deflated): before dinf may end the solve -- always, the estimate of the same call is never taken as a
        # certificate -- lambda_min is recomputed by a cold-started, undeflated run
        lam_v, v_v, lmax_v, conv = _verify_lambda_min(h, escape(1), o, data, 1e-9, 60000)
        return max(0.0, -lam_v) / (1.0 + lmax_v), v_v, conv

    try:
        if k.setup is not None:
            k.setup()
        topts = _rtr_opts(o)
        for it in range(1, maxiter + 1):                   # :38
            if not resident:
                tf = time.time()
                h.set_point(Y)
                if it > 1:                                 # part of a re-shape on the host
                    run.factor_seconds += time.time() - tf
            if U is not None:                              # :40-42 line_search
                _line_search(h, U)
            st = h.rtr(topts)                              # :43
            _count_rtr(data, st)
            run.gradnorm = st.gradnorm                     # :44
            if not device:
                tf = time.time()
                Y = run.Y = k.fetch()                      # X = Y'*Y of :45 -- what the reference returns (:86)
                run.factor_seconds += time.time() - tf
            run.z, run.Lam, obj, gap = k.evaluate(not device or eig_mode == "host")   # :46-48
            run.obj, run.gap = obj, gap
            t1 = time.time()
            certified = True
            run.S = None
            if eig_mode == "host":
                run.S = k.host_S(run.z, run.Lam)           # :49
                dS, vS, nneg = _extreme_eigs_host(run.S, delta, dense_max)   # :50
                lam_min, lam_max = dS[0], dS[-1]
            elif eig_mode == "host_sparse":
                # diagnostic: ARPACK shift-invert on the host (sparse LU of S - sigma I), k bottom eigenpairs
                import scipy.sparse.linalg as spla
                run.S = k.host_S(run.z, run.Lam).tocsc()
                lam_max = float(spla.eigsh(run.S, k=1, which="LA", return_eigenvectors=False, tol=1e-6)[0])
                lam, vS = spla.eigsh(run.S, k=delta, sigma=-1e-3 - 0.0 * lam_max, which="LM", tol=1e-12)
                order = np.argsort(lam); lam = lam[order]; vS = vS[:, order]
                lam_min = lam[0]
                nneg = int(np.sum(lam < 0))
            else:
                lam, vS, lam_max, _, certified = _device_escape(h, escape(delta), o, data, 1e-9, 60000)
                lam_min = lam[0]
                nneg = int(np.sum(lam < 0))                # missing pairs come back as +inf
                data["escape_method"] = h.escape_method()  # 1: block eigen-solver, 0: Lanczos
            data["eig_seconds"] += time.time() - t1
            dinf = max(0.0, -lam_min) / (1.0 + lam_max)    # :51
            res = dinf if gap is None else max(dinf, gap)  # what ends the solve and feeds the slow-progress watch
            last_verified = eig_mode != "device"
            if eig_mode == "device" and certified and (res < tol or it == maxiter):
                last_verified = True
                dinf_v, v_v, certified = verify()
                if dinf_v >= tol > dinf:                   # the deflated run had missed the bottom of the spectrum
                    vS = np.hstack([v_v, vS[:, :max(delta - 1, 0)]])
                    nneg = max(nneg, 1)
                dinf = dinf_v
                res = dinf if gap is None else max(dinf, gap)
            run.dinf = dinf
            tf = time.time()
            if device:                                     # :52-54 from the device's Gram matrix
                Q, e, r = _thin_svd_rank(None, theta, gram=k.device[0]())
            else:
                Q, e, r = _thin_svd_rank(Y, theta, gram=k.host_gram(Y) if k.host_gram is not None else None)
            run.r = r
            run.factor_seconds += time.time() - tf
            row = (it, obj, dinf) + (() if gap is None else (gap,)) + (r, p, time.time() - t0)
            _say(verbose, (_MANIFOLD_LINE if gap is None else _MANIFOLD_LINE_GAP) % row)
            data["log"].append(row + (st.hessvecs,))
            data["iters"] = it
            stop = res < tol and certified                 # :57-60 (an unconverged Lanczos run certifies nothing)
            if stop:
                _say(verbose, "Optimality is reached!")
            elif it % 20 == 0:                             # :61-69
                if it > 50 and res > res0:
                    data["status"] = 2
                    _say(verbose, "Slow progress!")
                    stop = True
                else:
                    res0 = res
            if device and (stop or it == maxiter):         # the evaluated point, before the last pass re-shapes it
                run.Y = k.fetch()
            if stop or (device and it == maxiter and not k.reshape_last):
                break
            if k.rerun and dinf < tol <= gap:              # S is PSD but the point is not stationary: trustregions() again
                run.reruns += 1
                resident = device                          # (the device path: on the factor where it is)
                continue
            nne = max(min(nneg, delta), 1)                 # :74
            tf = time.time()
            Y, U, p = _manifold_reshape(k, o, run, Y, p, Q, e, r, vS, nne)
            resident = Y is None
            run.factor_seconds += time.time() - tf
        if k.verify_at_end and obj is not None and not last_verified and certified:   # stopped on "Slow progress": the true dinf
            run.dinf, _, certified = verify()
            res = run.dinf if gap is None else max(run.dinf, gap)
        if k.finish is not None:
            k.finish(run)
    finally:
        h.close()
    if data["status"] == 0 and (res is None or res > tol or not certified):   # :92-95
        data["status"] = 1
        _say(verbose, "Iteration maximum is reached!")
    if obj is not None:
        _say(verbose, "ManiSDP: optimum = %0.8f, time = %0.2fs" % (obj, time.time() - t0))
    return run


# ============================================================ one AL loop for the affine, multiblock and dual kinds
# The reference's entry points other than ManiSDP_onlyunitdiag are copies of one scheme (as matlab/msdp_al_engine.m says):
# solve the subproblem, update the multipliers, measure the KKT residues, cut the rank, add escape directions, adapt sigma.
# _al_loop holds that scheme once.  What sets a kind apart is data: a factor geometry (_OneFactor / _Blocks), a multiplier
# side (_primal_side / _dual_side) and the numbers and rules of a _Kind record.
def _dense_vec(v):
    if sp.issparse(v):
        return np.asarray(v.todense()).ravel()
    return np.asarray(v, dtype=np.float64).ravel()


def _with_defaults(options, defaults):
    o = dict(options or {})
    for k, v in defaults.items():
        o.setdefault(k, v)
    return o


def _rows(Y):                       # oblique factor: unit rows (ManiSDP_unitdiag.m:106)
    return Y / np.sqrt(np.sum(Y * Y, axis=1, keepdims=True))


def _frobenius(Y):                  # sphere factor (spherefactory.m:249-254, ManiSDP_unittrace.m:110)
    return Y / np.linalg.norm(Y)


def _euclidean(Y):                  # euclideanfactory.m:82 (M.rand = randn), ManiSDP.m:107: no normalisation
    return Y


def _dinf_primal(lam_min, lam_max):     # ManiSDP_unitdiag.m:69
    return max(0.0, -lam_min) / (1.0 + lam_max)


def _dinf_abs(lam_min, lam_max):        # ManiDSDP_unitdiag.m:86, ManiSDP_multiblock.m:87
    return max(0.0, -lam_min) / (1.0 + abs(lam_max))


def _gap_primal(obj, by):               # ManiSDP_unitdiag.m:71
    return abs(obj - by) / (abs(by) + abs(obj) + 1.0)


def _gap_dual(obj, by):                 # ManiDSDP_unitdiag.m:87
    return abs(obj - by) / (1.0 + abs(obj) + abs(by))


def _factor_rank(Y, theta, strict):
    """svd(Y) and the rank estimate: r = sum(e >= theta*e(1)) in the primal kinds, strict ``>`` in the dual ones
    (ManiDSDP_unitdiag.m:88-90)."""
    Q, e, r = _thin_svd_rank(Y, theta)
    if strict:
        r = int(np.sum(e > theta * e[0]))
    return Q, e, r


def _widen(Y, p, V, nne, o, normalise):
    """Add nne escape directions V to the (already cut) factor (ManiSDP_unitdiag.m:97-106): with line_search they
    become the direction U next to p zero columns and Y gets zero columns; otherwise they are appended with weight alpha
    and the factor is normalised.  Returns (Y, U or None, p + nne)."""
    U = None
    if o["line_search"] == 1:
        U = np.hstack([np.zeros((Y.shape[0], p)), V[:, :nne]])
        Y = np.hstack([Y, np.zeros((Y.shape[0], nne))])
    else:
        Y = normalise(np.hstack([Y, o["alpha"] * V[:, :nne]]))
    return Y, U, p + nne


def _eig_host(h, o, S, data):
    """eig(S) of the reference on the host: of the S the host built (affine kinds, ManiSDP_unitdiag.m:68), else of the
    dual slack the device holds (dual kinds, ManiDSDP_unitdiag.m:82).  Returns (lam, V, lam_max, certified)."""
    if S is None:
        X = h.get_dual_slack()
        S = 0.5 * (X + X.T)
    dS, vS = np.linalg.eigh(S)
    return dS, vS, dS[-1], True


def _eig_device(h, o, S, data):
    """The few-eigenvector device escape instead of the O(n^3) eig: the `delta` bottom pairs and lambda_max of an
    explicit S from the host, else of the S resident after al_dual / dual_outer_step."""
    k = int(o["delta"])
    if S is None:
        run = lambda tol, maxit: h.escape_eigs_dual(k, tol=tol, maxit=maxit)
    else:
        run = lambda tol, maxit: h.escape_eigs_matrix(S, k, tol=tol, maxit=maxit)
    lam, vS, lam_max, _, certified = _device_escape(h, run, o, data, 1e-10, 20000)
    return lam, vS, lam_max, certified


class _OneFactor:
    """Factor geometry of the kinds with one (n, p) factor Y.  ``eig``: _eig_host or _eig_device; ``dinf``: the
    kind's dinf formula; ``nne_floor``: least number of escape directions; ``miss_nneg(lam, nneg)``: the escape count
    after the independent check found a lambda_min the regular escape had missed; ``layout``: the memory order Y is
    kept in; ``comm``: row-sharded handle (the point is all-gathered)."""
    line = "Iter %d, obj:%0.8f, gap:%0.1e, pinf:%0.1e, dinf:%0.1e, gradnorm:%0.1e, r:%d, p:%d, sigma:%0.3f, time:%0.2fs"

    def __init__(self, h, o, n, normalise, eig, dinf, strict_rank, nne_floor, miss_nneg, layout=np.ascontiguousarray,
                 comm=None):
        self.h, self.o, self.n, self.normalise, self.eig, self.dinf = h, o, n, normalise, eig, dinf
        self.strict_rank, self.nne_floor, self.miss_nneg, self.layout, self.comm = strict_rank, nne_floor, miss_nneg, layout, comm
        self.rtr_opts = _rtr_opts(o)

    def start(self, rng, p):                               # trustregions.m:390-392 -> M.rand()
        Y = self.o.get("Y0", None)
        if Y is None:
            Y = self.normalise(rng.standard_normal((self.n, p)))
        return self.layout(Y, dtype=np.float64)

    def pack(self, Y, p):
        return Y

    def topts(self, p):
        return self.rtr_opts

    def fetch(self, p):
        return self.h.get_point_all() if self.comm is not None else self.h.get_point()

    def spectrum(self, S, data):
        lam, vS, lam_max, certified = self.eig(self.h, self.o, S, data)
        return self.dinf(lam[0], lam_max), certified, (lam, vS, int(np.sum(lam < 0)))

    def missed(self, esc, lam_v, v_v):
        lam, vS, nneg = esc
        return lam, np.hstack([v_v, vS[:, :max(int(self.o["delta"]) - 1, 0)]]), self.miss_nneg(lam, nneg)

    def keep(self, Y, p):
        return Y

    def shape(self, Y, p):                                 # ManiSDP_unitdiag.m:72-74
        Q, e, r = _factor_rank(Y, float(self.o["theta"]), self.strict_rank)
        return (r, p), (Q, e, r)

    def reshape(self, Y, p, cut, esc):
        Q, e, r = cut
        if r <= p - 1:                                     # ManiSDP_unitdiag.m:93-96
            Y = _rank_cut(Y, Q, e, r)
            p = r
        nne = max(min(esc[2], int(self.o["delta"])), self.nne_floor)    # :97
        Y, U, p = _widen(Y, p, esc[1], nne, self.o, self.normalise)
        return self.layout(Y), U, p


_RESIDENT = object()               # stands for "the factor is the handle's resident point" between _Blocks.fetch / reshape / pack


def _block_reshape_option(o):
    """options["block_reshape"]: "host" (default) = the per-block loop of _Blocks.reshape, "device" = msdp_block_reshape."""
    br = o.get("block_reshape", "host")
    if br not in ("host", "device"):
        raise ValueError(f"options['block_reshape'] must be 'host' or 'device', not {br!r}")
    return br


BLOCK_EIG_SMALL, BLOCK_EIG_LARGE, BLOCK_EIG_LARGE_K = 256, 1024, 8     # msdp_block_eigs / msdp_block_eigs_large: orders, vectors


def _block_eig_auto(nset):
    """Whether block_eig = "auto" takes the device for the block orders `nset`.  All orders <= 256: from 16 blocks on (msdp_block_eigs
    wins there; below, the host loop keeps the iterates the oracle-parity tests compare).  A set that contains a
    block of order above 256: the host loop, whatever its size -- msdp_block_eigs_large has not been timed against the host loop
    (tools/time_block_eigs_large.py makes the comparison), and "auto" moves a set to the device only where the device has won a
    measurement.  block_eig = "device" takes such sets."""
    if max(nset) <= BLOCK_EIG_SMALL:
        return len(nset) >= 16
    return False


class _Blocks:
    """Factor geometry of the multiblock kinds: factors (n_i, p_i), oblique for the first ``nob`` blocks and Euclidean
    after them, packed into ONE zero-padded (sum n_i, max p_i) factor on the device; the per-block bookkeeping
    (eig(S_i), svd(Y_i), escape directions; ManiSDP_multiblock.m:78-147) stays on the host -- the blocks are small by
    construction.  ``block_eig``: "host" = the reference's loop of eig(S_i) on the host, "device" = all blocks in one
    launch (msdp_block_eigs: one workgroup per block; Householder tridiagonalisation, bisection, inverse iteration for the
    `delta` <= 8 vectors the loop uses) and the blocks of order 257 .. 1024 in one msdp_block_eigs_large call (the same method,
    a group of workgroups per block; needs delta <= 8; larger orders raise), "auto" (default) = device from 16 blocks of order
    <= 256 on, host below -- where the oracle-parity tests compare iterate by iterate: the eigenvectors of two eigen-solvers
    differ by signs / rotations inside eigenspaces; a set that contains a block of order above 256 stays on the host under "auto" (not yet timed).
    ``block_reshape``: "host" (default) = the per-block loop of :meth:`reshape` on the fetched factor, "device" = one
    msdp_block_reshape call per outer iteration on the resident factor (widths <= 64): `fetch` then hands the loop _RESIDENT
    instead of the factor, `pack` has nothing to upload, and the factor comes to the host once, at the end (:meth:`final`); an
    iteration the call refuses as unsupported runs the host loop and re-enters through set_point."""
    line = "Iter %d, obj:%0.8f, gap:%0.1e, pinf:%0.1e, dinf:%0.1e, gradnorm:%0.1e, p_max:%d, sigma:%0.3f, time:%0.2fs"

    def __init__(self, h, o, nset, nob, strict_rank):
        self.h, self.o, self.nset, self.nob, self.strict_rank = h, o, nset, nob, strict_rank
        self.reshape_device = _block_reshape_option(o) == "device"
        self.wV = None                                     # (w, V) of all blocks as the device eigen route returned them
        self.r0 = np.concatenate([[0], np.cumsum(nset)]).astype(int)
        self.N = int(self.r0[-1])
        be = o.get("block_eig", "auto")
        self.eig_forced = be == "device"
        self.eig_device = be == "device" or (be == "auto" and _block_eig_auto(nset))
        self.S = None                                      # the blocks of S the host eig last fetched

    def normalise(self, i):
        return _rows if i < self.nob else _euclidean

    def start(self, rng, p):                               # trustregions.m:390-392 -> M.rand() (randc.cpp)
        Yb = self.o.get("Y0", None)
        if Yb is None:
            Yb = [self.normalise(i)(rng.standard_normal((self.nset[i], p[i]))) for i in range(len(self.nset))]
        return [np.ascontiguousarray(Yi, dtype=np.float64) for Yi in Yb]

    def pack(self, Yb, p):
        if Yb is _RESIDENT:
            return None
        if isinstance(Yb, np.ndarray):                     # the direction U of the device reshape: already one (N, max p) array
            return Yb
        return _pack_blocks(Yb, self.r0, self.N, max(p))

    def topts(self, p):                                    # M.typicaldist of multiblockmanifold.m:11-15
        nset, nob = self.nset, self.nob
        tdist = math.sqrt(math.pi * sum(nset[:nob]) + sum(pi * ni for pi, ni in zip(p[nob:], nset[nob:])))
        o = self.o
        return _lib.default_opts(maxiter=int(o["TR_maxiter"]), maxinner=int(o["TR_maxinner"]),
                                 tolgradnorm=float(o["tolgradnorm"]), Delta_bar=tdist)

    def fetch(self, p):
        # block_reshape = "device": the factor stays where it is (the loop asks for it with keep() / final() when it returns it)
        return _RESIDENT if self.reshape_device else self.download(p)

    def keep(self, Yb, p):
        """The iterate itself, on the host: the loop calls this before a reshape whose input it is going to return."""
        return self.download(p) if Yb is _RESIDENT else Yb

    def download(self, p):
        Yfull = self.h.get_point()
        return [np.ascontiguousarray(Yfull[self.r0[i]:self.r0[i + 1], :p[i]]) for i in range(len(self.nset))]

    def spectrum(self, S, data):                           # ManiSDP_multiblock.m:78-89
        h, r0, nset = self.h, self.r0, self.nset
        if self.eig_device:
            try:
                wall, Vall = self._device_eigs()
            except _lib.MsdpError:
                if self.eig_forced:
                    raise
                self.eig_device = False
        dS, vS = [], []
        self.S = []
        self.wV = (wall, Vall) if self.eig_device else None
        for i in range(len(nset)):
            if self.eig_device:
                dS.append(wall[r0[i]:r0[i + 1]]); vS.append(Vall[r0[i]:r0[i + 1], :])
            else:                                          # only the diagonal blocks come to the host
                Si = h.get_dual_slack_block(r0[i], nset[i])
                w, V = np.linalg.eigh(0.5 * (Si + Si.T))   # :86
                self.S.append(Si); dS.append(w); vS.append(V)
        return max(_dinf_abs(w[0], w[-1]) for w in dS), True, (dS, vS)   # :87-89

    def _device_eigs(self):
        """(w, V) of all blocks, rows in block order: the blocks of order <= 256 in one msdp_block_eigs call, the larger ones in one
        msdp_block_eigs_large call."""
        h, r0, nset, delta = self.h, self.r0, self.nset, int(self.o["delta"])
        small = [i for i, n in enumerate(nset) if n <= BLOCK_EIG_SMALL]
        large = [i for i, n in enumerate(nset) if n > BLOCK_EIG_SMALL]
        if not large:
            return h.block_eigs(r0[:-1], nset, delta)
        if max(nset) > BLOCK_EIG_LARGE or delta > BLOCK_EIG_LARGE_K:
            raise _lib.MsdpError(f"block_eig = 'device': blocks of order above {BLOCK_EIG_SMALL} need orders <= {BLOCK_EIG_LARGE} and "
                                 f"delta <= {BLOCK_EIG_LARGE_K} (largest order {max(nset)}, delta {delta})")
        wall, Vall = np.empty(self.N), np.empty((self.N, delta))
        for idx, call in ((small, h.block_eigs), (large, h.block_eigs_large)):
            if not idx:
                continue
            w, V = call([r0[i] for i in idx], [nset[i] for i in idx], delta)
            at = 0
            for i in idx:
                wall[r0[i]:r0[i + 1]] = w[at:at + nset[i]]; Vall[r0[i]:r0[i + 1]] = V[at:at + nset[i]]
                at += nset[i]
        return wall, Vall

    def shape(self, Yb, p):
        return (max(p),), None

    def reshape(self, Yb, p, cut, esc):                    # ManiSDP_multiblock.m:109-147
        if self.reshape_device:
            try:
                return self._reshape_device(p, esc)
            except _lib.MsdpError as e:                    # a width beyond the call's or the handle's (or a Jacobi iteration that did
                if e.code not in (_lib.EUNSUPPORTED, _lib.ESTATE):   # not converge): the point is untouched, this iteration runs on
                    raise                                  # the host and comes back in through set_point (which re-allocates)
            if Yb is _RESIDENT:
                Yb = self.download(p)
        dS, vS = esc
        o, delta, p = self.o, int(self.o["delta"]), list(p)
        newY, newU = [], []
        for i, n in enumerate(self.nset):
            Yi, Ui = Yb[i], None
            if n >= o["min_facsize"]:
                if p[i] > 1:
                    Q, e, r = _factor_rank(Yi, float(o["theta"]), self.strict_rank)   # :112-121
                    r = max(r, 1)
                    if r < p[i]:
                        Yi = _rank_cut(Yi, Q, e, r)        # :125
                        p[i] = r
                nneg = int(np.sum(dS[i] < 0))
                nne = max(min(nneg, delta), 1 if i < self.nob else 0)    # :129-133
                if p[i] + nne > n:
                    nne = 0                                # :134-136
                Yi, Ui, p[i] = _widen(Yi, p[i], vS[i], nne, o, self.normalise(i))   # :137-147
            newY.append(np.ascontiguousarray(Yi))
            newU.append(Ui if Ui is not None else np.zeros_like(Yi))
        return newY, (newU if o["line_search"] == 1 else None), p


    def _reshape_device(self, p, esc):
        """The same lines in one msdp_block_reshape call on the resident factor: (w, V) of the device eigen route as they came, the
        host route's eigh results repacked into that layout."""
        o, delta = self.o, int(self.o["delta"])
        if self.wV is not None:
            w, V = self.wV
        else:
            dS, vS = esc
            w = np.concatenate(dS)
            V = np.zeros((self.N, delta))
            for i, Vi in enumerate(vS):
                V[self.r0[i]:self.r0[i + 1], :min(delta, Vi.shape[1])] = Vi[:, :delta]
        mode = 1 if o["line_search"] == 1 else 0
        p_out, _, _, U = self.h.block_reshape(self.r0[:-1], self.nset, p, w, V, float(o["theta"]), self.strict_rank, delta,
                                              float(o["alpha"]), int(o["min_facsize"]), mode)
        return _RESIDENT, U, [int(v) for v in p_out]

    def final(self, Yb, p):
        """The iterate the loop returned, on the host (block_reshape = "device" leaves it on the device when the loop stops early)."""
        return self.keep(Yb, p)


def _by(b, y, z):                                          # ManiSDP_unitdiag.m:70 (no z term in the generic kind)
    return float(b @ y) if z is None else float(b @ y) + float(np.sum(z))


def _primal_side(h, b):
    """Multiplier side of the primal kinds on the device: obj and A x (msdp_al_primal), the y update,
    then S and z (msdp_al_dual; S stays on the device).  Returns (set_penalty, outer_step)."""
    normb = 1.0 + np.linalg.norm(b)

    def outer_step(Y, y, sigma):
        obj, Ax = h.al_primal(b.size)                      # ManiSDP_unitdiag.m:59-61
        Axb = Ax - b                                       # :62
        pinf = float(np.linalg.norm(Axb)) / normb          # :63
        y = y - sigma * Axb                                # :64
        z = h.al_dual(y)                                   # :65-67
        return obj, _by(b, y, z), pinf, y, z, None
    return h.set_multipliers, outer_step


def _dual_side(h, call, nf):
    """Multiplier side of the dual kinds (ManiDSDP_unitdiag.m:70-85): x <- x - sigma*As on the device
    (msdp_dual_outer_step), the w update and obj = <C, eX> + cf'w (+ sum z where the kind has z).
    Returns (set_penalty, outer_step)."""
    normc = 1.0 + np.linalg.norm(call)                     # :32
    cf = call[:nf]

    def outer_step(Y, w, sigma):
        by, cex, as2, Af, z = h.dual_outer_step()
        pinf = (math.sqrt(as2) + float(np.linalg.norm(Af))) / normc    # :75
        w = w - sigma * Af                                 # :78
        obj = cex + float(cf @ w)                          # :85
        if z is not None:
            obj = obj + float(np.sum(z))
        return obj, by, pinf, w, z, None
    return (lambda w, sigma: h.dual_set_penalty(sigma, w)), outer_step


class _Kind:
    """What the outer loop needs to know of a kind beyond its geometry and multiplier side.
    ``gap``: _gap_primal / _gap_dual; ``slow``: (every, after) of the slow-progress watch; ``verify``: the device escape
    is checked by _verify_lambda_min before dinf may end the solve, once the KKT residues (``verify_on_kkt``) or dinf
    alone are below tol; ``verify_at_end``: a solve that stopped without that check gets it once more (both need the
    single-factor geometry: the check is of one n x n S, and its result goes through _OneFactor.dinf / .missed);
    ``log``: the slice of (it, obj, gap, pinf, dinf, gradnorm, <shape>, sigma, time) that goes to data["log"]."""

    def __init__(self, geo, side, maxiter, gap, slow, message, verify=False, verify_on_kkt=False, verify_at_end=False,
                 log=slice(None), iter_hook=None):
        assert not (verify or verify_at_end) or isinstance(geo, _OneFactor), "the lambda_min check needs one factor"
        self.geo, (self.set_penalty, self.outer_step) = geo, side
        self.maxiter, self.gap, self.slow, self.message = maxiter, gap, slow, message
        self.verify, self.verify_on_kkt, self.verify_at_end = verify, verify_on_kkt, verify_at_end
        self.log, self.iter_hook = log, iter_hook


def _al_loop(h, o, t, Y, p, mult, verbose):
    """The augmented-Lagrangian outer loop (ManiSDP_unitdiag.m:55-113 and its copies in the other entry points):
    trustregions() on the device, multiplier update, KKT residues, stop and slow-progress tests, rank cut, escape
    directions, sigma update.  Returns (obj, data, last) with ``last`` = (Y, multipliers, z, S) of the last evaluated
    point, p at its end and the per-iteration lists fac_size and seta."""
    geo, tol = t.geo, o["tol"]
    every, after = t.slow
    sigma = float(o["sigma0"]); gama = float(o["gama"])
    data = {"status": 0, "hessvecs": 0, "cost_evals": 0, "rejected": 0, "rtr_seconds": 0.0, "eig_seconds": 0.0, "log": []}
    fac_size, seta = [], []
    U = None
    t0 = time.time()
    gap0 = pinf0 = dinf0 = None
    obj = gap = pinf = dinf = gradnorm = eta = None
    Y_eval = z = S = None
    certified = last_verified = True

    def verify():
        # the regular escape call is warm-started (columns of Y and the previous call's vectors in its start block, or
        # span(Y) deflated): before dinf may end the solve, lambda_min is recomputed by a cold-started, undeflated run
        return _verify_lambda_min(h, lambda tol, maxit: h.escape_eigs_dual(1, tol=tol, maxit=maxit), o, data, 1e-10, 20000,
                                  dense_n=geo.n)

    for it in range(1, t.maxiter + 1):
        fac_size.append(p)
        t.set_penalty(mult, sigma)
        Yp = geo.pack(Y, p)
        if Yp is not None:                                 # None: the geometry reshaped the resident point on the device
            h.set_point(Yp)
        if U is not None:
            _line_search(h, geo.pack(U, p))
        st = h.rtr(geo.topts(p))                           # ManiSDP_unitdiag.m:57
        _count_rtr(data, st)
        gradnorm = st.gradnorm
        Y = Y_eval = geo.fetch(p)                          # what the reference returns (:114)
        obj, by, pinf, mult, z, S = t.outer_step(Y, mult, sigma)
        t1 = time.time()
        dinf, certified, esc = geo.spectrum(S, data)       # :68-69
        data["eig_seconds"] += time.time() - t1
        gap = t.gap(obj, by)                               # :71
        last_verified = not t.verify
        if t.verify and certified and ((max(gap, pinf, dinf) if t.verify_on_kkt else dinf) < tol or it == t.maxiter):
            last_verified = True
            lam_v, v_v, lmax_v, certified = verify()
            dinf_v = geo.dinf(lam_v, lmax_v)
            if dinf_v >= tol > dinf:                       # the deflated run had missed the bottom of the spectrum
                esc = geo.missed(esc, lam_v, v_v)
            dinf = dinf_v
        shape, cut = geo.shape(Y, p)
        row = (it, obj, gap, pinf, dinf, gradnorm) + shape + (sigma, time.time() - t0)
        _say(verbose, geo.line % row)
        data["log"].append(row[t.log])
        eta = max(gap, pinf, dinf)                         # :77
        seta.append(eta)
        data["iters"] = it
        if t.iter_hook is not None:                        # diagnostics (tools/): sees the loop's local state
            t.iter_hook(locals())
        if eta < tol and certified:                        # an unconverged Lanczos run certifies nothing
            _say(verbose, "Optimality is reached!")
            break
        if it % every == 0:                                # :82-92
            if it > after and gap > gap0 and pinf > pinf0 and dinf > dinf0:
                data["status"] = 2
                _say(verbose, "Slow progress!")
                break
            gap0, pinf0, dinf0 = gap, pinf, dinf
        if it == t.maxiter:                                # the loop ends here and returns Y_eval: a geometry that keeps the factor
            Y = Y_eval = geo.keep(Y, p)                    # on the device hands it over before the reshape below rewrites it
        Y, U, p = geo.reshape(Y, p, cut, esc)              # :93-106
        if pinf < o["tau1"] * gradnorm:                    # :108-112
            sigma = max(sigma / gama, float(o["sigma_min"]))
        elif pinf > o["tau2"] * gradnorm:
            sigma = min(sigma * gama, float(o["sigma_max"]))
    if t.verify_at_end and obj is not None and not last_verified and certified:   # stopped on "Slow progress": report the true dinf
        lam_v, _, lmax_v, certified = verify()
        dinf = geo.dinf(lam_v, lmax_v)
    data.update({"Y": Y_eval, "gap": gap, "pinf": pinf, "dinf": dinf, "gradnorm": gradnorm, "time": time.time() - t0,
                 "sigma": sigma})
    if data["status"] == 0 and (eta is None or eta > tol or not certified):
        data["status"] = 1
        _say(verbose, "Iteration maximum is reached!")
    _say(verbose, t.message % (obj, time.time() - t0))
    return obj, data, (Y_eval, mult, z, S, p, fac_size, seta)


# =================================================================== affine kinds
def _affine_impl(kind, At, b, c, K, options, verbose, rng, defaults):
    o = _with_defaults(options, defaults)
    escape_rr = _escape_rr_option(o)                       # (a bad value is refused before anything is built)
    n = int(K["s"])
    rng = rng or np.random.default_rng(0)
    b = _dense_vec(b)
    c = _dense_vec(c)
    Atc = sp.csc_matrix(At)
    A = Atc.T.tocsr()
    sphere = kind == _lib.KIND_UNITTRACE
    generic = kind == _lib.KIND_GENERIC                # src/primal/ManiSDP.m: Euclidean manifold, no z term
    eig_mode = o.get("eig", "host" if n <= int(o.get("dense_eig_max", 400)) else "device")
    _say(verbose, "ManiSDP is starting...")
    _say(verbose, f"SDP size: n = {n}, m = {b.size}")
    h = _lib.Handle.affine(kind, Atc, b, c, n, pcap=max(32, int(o["p0"]) + 2 * int(o["delta"])))
    try:
        # options['comm'] = (nranks, rank, unique_id): one process per GPU, rows of the factor sharded over the ranks
        # (msdp_comm_init).  Every rank runs this same host loop on identical data -- the operator state is replicated on
        # the device, the start point must be the same on all ranks (pass Y0 or seed rng identically) -- and reaches the
        # same decisions; collectives happen inside the library calls.
        comm = o.get("comm")
        if comm is not None:
            _join_comm(h, comm)
        if "escape_method" in o:                           # 0 auto (Lanczos on the explicit S of these kinds), 1 Lanczos, 2 block eigen-solver
            h.set_option("escape_method", int(o["escape_method"]))
        if escape_rr:
            h.set_option("escape_rr", escape_rr)
        for name, value in (o.get("device_options") or {}).items():     # run-time switches of the handle (msdp_set_option): A/B runs, tests
            h.set_option(name, int(value))
        dev_al = eig_mode == "device" and bool(o.get("device_al", True))
        normb = 1.0 + np.linalg.norm(b)

        def host_step(Y, y, sigma):                        # the reference's n x n arithmetic on the host
            X = Y @ Y.T                                    # unitdiag :59 / unittrace :59
            x = X.ravel(order="F")
            obj = float(c @ x)                             # :61
            Axb = A @ x - b                                # :62
            pinf = float(np.linalg.norm(Axb)) / normb      # :63
            y = y - sigma * Axb                            # :64
            eS = (c - Atc @ y).reshape((n, n), order="F")  # :65
            if generic:
                z, S = None, eS                            # ManiSDP.m:64
            elif sphere:
                z = float(np.sum(eS * X))                  # unittrace :66
                S = eS - z * np.eye(n)                     # :67
            else:
                z = np.sum(X * eS, axis=0)                 # unitdiag :66
                S = eS - np.diag(z)                        # :67
            return obj, _by(b, y, z), pinf, y, z, S

        set_penalty, dev_step = _primal_side(h, b)
        geo = _OneFactor(h, o, n, _euclidean if generic else _frobenius if sphere else _rows,
                         _eig_device if eig_mode == "device" else _eig_host, _dinf_primal, strict_rank=False,
                         nne_floor=0 if (sphere or generic) else 1,           # unittrace :101 / ManiSDP.m:99 / unitdiag :97
                         miss_nneg=lambda lam, nneg: 1 + int(np.sum(lam[:-1] < 0)),   # the missed pair goes in below the others
                         comm=comm)
        t = _Kind(geo, (set_penalty, dev_step if dev_al else host_step), int(o["AL_maxiter"]), _gap_primal,
                  (20, 50) if (sphere or generic) else (50, 100), "ManiSDP: optimum = %0.8f, time = %0.2fs",
                  verify=dev_al, verify_on_kkt=True, verify_at_end=True, iter_hook=o.get("iter_hook"))
        p = int(o["p0"])
        obj, data, (Y, y, z, S, _, fac_size, _) = _al_loop(h, o, t, geo.start(rng, p), p, np.zeros(b.size), verbose)
        if S is None and obj is not None and n <= int(o.get("dense_X_max", 6000)):
            S = h.get_dual_slack()                         # data.S of the reference (:116), from the device
        if eig_mode == "device":
            data["escape_rr_stages"] = h.ritz_stages()     # Rayleigh-Ritz stages: (device, host, host after fallback)
    finally:
        h.close()
    data.update({"X": (Y @ Y.T if n <= int(o.get("dense_X_max", 6000)) else None), "y": y, "S": S, "z": z})
    if not sphere and not generic:
        data["fac_size"] = fac_size
    return Y, obj, data


def ManiSDP_unitdiag(At, b, c, K, options=None, verbose=True, rng=None):
    """``[X, obj, data] = ManiSDP_unitdiag(At, b, c, K, options)`` (reference
    src/primal/ManiSDP_unitdiag.m:7; defaults :10-26)."""
    with _host_threads():
        return _affine_impl(_lib.KIND_UNITDIAG, At, b, c, K, options, verbose, rng, DEFAULTS["unitdiag"])


def ManiSDP_unittrace(At, b, c, K, options=None, verbose=True, rng=None):
    """``[X, obj, data] = ManiSDP_unittrace(At, b, c, K, options)`` (reference
    src/primal/ManiSDP_unittrace.m:7; defaults :10-25)."""
    with _host_threads():
        return _affine_impl(_lib.KIND_UNITTRACE, At, b, c, K, options, verbose, rng, DEFAULTS["unittrace"])


def ManiSDP(At, b, c, K, options=None, verbose=True, rng=None):
    """``[X, obj, data] = ManiSDP(At, b, c, K, options)`` -- the generic entry point on the Euclidean manifold
    (reference src/primal/ManiSDP.m:6; defaults :9-25).  Same device kernels as the two structured affine entry
    points with the projection / retraction terms switched off."""
    with _host_threads():
        return _affine_impl(_lib.KIND_GENERIC, At, b, c, K, options, verbose, rng, DEFAULTS["generic"])


# ================================================================= multiblock
DEFAULTS["multiblock"] = dict(min_facsize=2, AL_maxiter=1000, gama=2, sigma0=1e-1, sigma_min=1e-2, sigma_max=1e7,
                              tol=1e-8, theta=1e-2, delta=8, alpha=0.1, tolgradnorm=1e-8, TR_maxinner=20,
                              TR_maxiter=4, tau1=1e1, tau2=1e1, line_search=0)       # ManiSDP_multiblock.m:10-27 (+ p0 = ones)
DATA_FIELDS["multiblock"] = ("X", "y", "S", "gap", "pinf", "dinf", "gradnorm", "time", "status")   # :156-163


def _pack_blocks(blocks, r0, N, pmax):
    """Cell array of factors (n_i, p_i) -> one (N, pmax) array, zero beyond each block's own width."""
    Y = np.zeros((N, pmax))
    for i, Yi in enumerate(blocks):
        Y[r0[i]:r0[i + 1], :Yi.shape[1]] = Yi
    return Y


def _block_widths(o, nset):                                # ManiSDP_multiblock.m:34-39
    p0 = [int(v) for v in np.atleast_1d(o.get("p0", np.ones(len(nset), int)))]
    return [p0[i] if nset[i] >= o["min_facsize"] else nset[i] for i in range(len(nset))]


def ManiSDP_multiblock(At, b, c, K, options=None, verbose=True, rng=None):
    """``[X, obj, data] = ManiSDP_multiblock(At, b, c, K, options)`` (reference src/primal/ManiSDP_multiblock.m:7):
    block-diagonal X with unit diagonal on the first ``K['nob']`` blocks of orders ``K['s']``.  The product manifold
    of ``multiblockmanifold.m`` lives on the device as ONE factor of N = sum n_i rows whose blocks are zero-padded to a
    common width; the per-block bookkeeping of the outer loop (eig(S{i}), svd(Y{i}), escape directions; :78-147) stays
    on the host -- the blocks are small by construction; ``options['block_reshape'] = "device"`` moves the rank cut and the
    escape widening (:109-147) of all blocks into one device call per outer iteration (default "host").  Returns (list of
    factors, obj, data)."""
    with _host_threads():
        return _multiblock_impl(At, b, c, K, options, verbose, rng)


def _multiblock_impl(At, b, c, K, options, verbose, rng):
    o = _with_defaults(options, DEFAULTS["multiblock"])
    nset = [int(v) for v in np.atleast_1d(K["s"])]
    rng = rng or np.random.default_rng(0)
    b = _dense_vec(b)
    c = _dense_vec(c)
    _say(verbose, "ManiSDP is starting...")
    _say(verbose, f"SDP size: n = {max(nset)}, m = {b.size}")
    p = _block_widths(o, nset)
    _block_reshape_option(o)                               # (a bad value is refused before anything is built)
    h = _lib.Handle.multiblock(sp.csc_matrix(At), b, c, nset, int(K.get("nob", 0)), pcap=max(32, max(p) + 2 * int(o["delta"])))
    try:
        geo = _Blocks(h, o, nset, int(K.get("nob", 0)), strict_rank=False)
        t = _Kind(geo, _primal_side(h, b), int(o["AL_maxiter"]), _gap_primal, (50, 100),
                  "ManiSDP: optimum = %0.8f, time = %0.2fs")
        obj, data, (Yb, y, _, _, p, _, _) = _al_loop(h, o, t, geo.start(rng, p), p, np.zeros(b.size), verbose)
        Yb = data["Y"] = geo.final(Yb, p)
        S = geo.S                                          # data.S (:158): the blocks of the last iterate
        if geo.eig_device and Yb is not None:
            S = [h.get_dual_slack_block(geo.r0[i], nset[i]) for i in range(len(nset))]
    finally:
        h.close()
    data.update({"X": ([Yi @ Yi.T for Yi in Yb] if Yb is not None else None), "y": y, "S": S,   # :65-69, 156
                 "p": [Yi.shape[1] for Yi in (Yb or [])]})
    return Yb, obj, data


# ================================================================= dual approach
DEFAULTS["dual_unitdiag"] = dict(ADMM_maxiter=300, gama=2, sigma0=1e-3, sigma_min=1e-3, sigma_max=1e7, tol=1e-8, theta=1e-3,
                                 delta=8, alpha=0.1, tolgradnorm=1e-8, TR_maxinner=20, TR_maxiter=4, tau1=1e1, tau2=1e2,
                                 line_search=0)      # ManiDSDP_unitdiag.m:10-26 (+ p0 = ceil(log(m)), :11)
DATA_FIELDS["dual_unitdiag"] = ("X", "y", "S", "w", "gap", "pinf", "dinf", "gradnorm", "time", "fac_size", "seta", "status")   # :132-144


def _dual_matrices(A, c, nf, o):
    """[B A_psd] and c = [cf; c_psd] split at the K['f'] free columns (ManiDSDP_unitdiag.m:32-37); dAAt = options['dAAt'],
    default diag(A_psd A_psd') (:37), as a flat float64 vector (the bytes the handle reads)."""
    call = _dense_vec(c)
    Aall = sp.csc_matrix(A)
    B = Aall[:, :nf]; Apsd = sp.csr_matrix(Aall[:, nf:])
    dAAt = o.get("dAAt", None)
    if dAAt is None:
        dAAt = np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel()
    return call, (B if nf else None), Apsd, call[nf:], _dense_vec(dAAt)


def ManiDSDP_unitdiag(A, b, c, K, options=None, verbose=True, rng=None):
    """``[X, obj, data] = ManiDSDP_unitdiag(A, b, c, K, options)`` (reference src/dual/ManiDSDP_unitdiag.m:8): the dual
    approach for SDPs whose dual slack has a unit diagonal.  ``A`` is m x (K['f'] + K['s']^2) -- free columns first --
    and ``c`` has K['f'] + K['s']^2 entries.  The Riemannian subproblem (cost/grad/hess :174-194 on the oblique factor
    of S), the line search and the outer-step bookkeeping (:70-81) run on the device; the multiplier matrix x never
    leaves it.  Returns (X, obj, data); ``data['Y']`` is the factor of S (n x p)."""
    with _host_threads():
        return _dual_unitdiag_impl(A, b, c, K, options, verbose, rng)


def _dual_unitdiag_impl(A, b, c, K, options, verbose, rng):
    o = _with_defaults(options, DEFAULTS["dual_unitdiag"])
    n = int(K["s"]); nf = int(K.get("f", 0))
    b = _dense_vec(b)
    m = b.size
    o.setdefault("p0", int(math.ceil(math.log(m))))        # :11
    rng = rng or np.random.default_rng(0)
    _say(verbose, "ManiSDP is starting...")
    _say(verbose, f"SDP size: n = {n}, m = {m}")
    call, B, Apsd, cpsd, dAAt = _dual_matrices(A, c, nf, o)
    # eig(X) (:82): the reference's dense eig on the host up to n = 600 (0.5 ms there), beyond that the device escape on
    # the resident X with the independent lambda_min check before the solve may stop (d = 60, n = 1831: 1.6 s instead of 5.0 s)
    eig_mode = o.get("eig", "host" if n <= int(o.get("dense_eig_max", 600)) else "device")
    p = int(o["p0"])
    h = _lib.Handle.dual_unitdiag(Apsd, b, cpsd, dAAt, B, call[:nf], pcap=max(32, p + 2 * int(o["delta"])))
    try:
        geo = _OneFactor(h, o, n, _rows, _eig_host if eig_mode == "host" else _eig_device, _dinf_abs, strict_rank=True,
                         nne_floor=1, miss_nneg=lambda lam, nneg: max(nneg, 1))          # :114
        t = _Kind(geo, _dual_side(h, call, nf), int(o["ADMM_maxiter"]), _gap_dual, (50, 100),   # :99-109
                  "ManiDSDP: optimum = %0.8f, time = %0.2fs", verify=eig_mode != "host", log=slice(1, -1))
        obj, data, (Y, w, _, _, _, fac_size, seta) = _al_loop(h, o, t, geo.start(rng, p), p, np.zeros(nf), verbose)
        X = h.get_dual_slack() if obj is not None else None
        y = h.dual_get_y() if obj is not None else None
    finally:
        h.close()
    data.update({"X": X, "y": y, "S": (Y @ Y.T if Y is not None and n <= int(o.get("dense_X_max", 4000)) else None),
                 "w": w, "fac_size": fac_size, "seta": seta})
    return X, obj, data


DEFAULTS["dual"] = dict(p0=1, ADMM_maxiter=1000, gama=2, sigma0=1e-1, sigma_min=1e-2, sigma_max=1e7, tol=1e-8, theta=1e-2,
                        delta=8, alpha=0.01, tolgradnorm=1e-8, TR_maxinner=20, TR_maxiter=4, tau1=0.1, tau2=1,
                        line_search=1)       # ManiDSDP.m:10-25
DATA_FIELDS["dual"] = ("X", "y", "S", "w", "gap", "pinf", "dinf", "gradnorm", "time", "status")   # :125-133


def ManiDSDP(A, b, c, K, options=None, verbose=True, rng=None):
    """``[X, obj, data] = ManiDSDP(A, b, c, K, options)`` (reference src/dual/ManiDSDP.m:7): the dual approach
    ``sup <C, X> + <cf, w>  s.t.  A(X) + B(w) = b, X psd`` with S = Y Y' on the Euclidean factor Y (n x p).  ``A`` is
    m x (K['f'] + K['s']^2) -- free columns first -- and ``c`` has K['f'] + K['s']^2 entries; ``options['dAAt']`` as in
    the reference (default diag(A A') of the PSD part).  The Riemannian subproblem (costgrad / hess :162-177), the line
    search (:141-160) and the outer step (:66-77) run on the device; the multiplier matrix x never leaves it.
    Returns (X, obj, data); ``data['Y']`` is the factor of S."""
    with _host_threads():
        return _dual_impl(A, b, c, K, options, verbose, rng)


def _dual_impl(A, b, c, K, options, verbose, rng):
    o = _with_defaults(options, DEFAULTS["dual"])
    n = int(K["s"]); nf = int(K.get("f", 0))
    b = _dense_vec(b)
    rng = rng or np.random.default_rng(0)
    _say(verbose, "ManiSDP is starting...")                # :28-29
    _say(verbose, f"SDP size: n = {n}, m = {b.size}")
    call, B, Apsd, cpsd, dAAt = _dual_matrices(A, c, nf, o)
    # eig(X) (:76) as in ManiDSDP_unitdiag: the host's dense eig up to n = 600, the device escape with the independent
    # lambda_min check beyond
    eig_mode = o.get("eig", "host" if n <= int(o.get("dense_eig_max", 600)) else "device")
    p = int(o["p0"])
    h = _lib.Handle.dual(Apsd, b, cpsd, dAAt, B, call[:nf], pcap=max(32, p + 2 * int(o["delta"])))
    try:
        g_identity = h.dual_g_identity()
        geo = _OneFactor(h, o, n, _euclidean, _eig_host if eig_mode == "host" else _eig_device, _dinf_abs, strict_rank=True,
                         nne_floor=0, miss_nneg=lambda lam, nneg: max(nneg, 1),     # :109 (no lower bound)
                         layout=np.asfortranarray)
        t = _Kind(geo, _dual_side(h, call, nf), int(o["ADMM_maxiter"]), _gap_dual, (20, 50),   # :94-104
                  "ManiDSDP: optimum = %0.8f, time = %0.2fs", verify=eig_mode != "host", log=slice(1, -1))
        obj, data, (Y, w, _, _, p, fac_size, _) = _al_loop(h, o, t, geo.start(rng, p), p, np.zeros(nf), verbose)
        X = h.get_dual_slack() if obj is not None else None
        y = h.dual_get_y() if obj is not None else None
    finally:
        h.close()
    data.update({"X": X, "y": y, "S": (Y @ Y.T if Y is not None and n <= int(o.get("dense_X_max", 4000)) else None),
                 "w": w, "g_identity": g_identity, "p_max": max(fac_size + [p])})
    return X, obj, data


DEFAULTS["dual_multiblock"] = dict(min_facsize=2, ADMM_maxiter=1000, gama=2, sigma0=1e-1, sigma_min=1e-2, sigma_max=1e7, tol=1e-8,
                                   theta=1e-2, delta=8, alpha=0.2, tolgradnorm=1e-8, TR_maxinner=20, TR_maxiter=4, tau1=1e1,
                                   tau2=1e1, line_search=1)       # ManiDSDP_multiblock.m:12-28 (+ p0 = ones, :13)
DATA_FIELDS["dual_multiblock"] = ("X", "y", "S", "w", "gap", "pinf", "dinf", "gradnorm", "time", "status")   # :188-197


def ManiDSDP_multiblock(A, b, c, K, options=None, verbose=True, rng=None):
    """``[X, obj, data] = ManiDSDP_multiblock(A, b, c, K, options)`` (reference src/dual/ManiDSDP_multiblock.m:8): the dual
    approach ``sup <C, X> + <cf, w>  s.t.  A(X) + B(w) = b, X_i psd`` for block-diagonal X of orders ``K['s']``, the dual
    slacks S_i = Y_i Y_i' with unit diagonal on the first ``K['nob']`` blocks.  ``A`` is m x (K['f'] + sum n_i^2) -- free
    columns first, then the concatenated column-major vecs of the blocks -- and ``c`` has as many entries;
    ``options['dAAt']`` as in the reference.  The costgrad / hess closures (:243-296), the line search and the outer step
    (:86-124) run on the device on the blocks' own storage; the per-block bookkeeping (eig(X_i), svd(Y_i), escape
    directions; :121-181) follows :func:`ManiSDP_multiblock` (``block_eig`` option).  Returns (list of X_i, obj, data);
    ``data['Y']`` is the list of factors (n_i, p_i)."""
    with _host_threads():
        return _dual_multiblock_impl(A, b, c, K, options, verbose, rng)


def _dual_multiblock_impl(A, b, c, K, options, verbose, rng):
    o = _with_defaults(options, DEFAULTS["dual_multiblock"])
    nset = [int(v) for v in np.atleast_1d(K["s"])]
    nob = int(K.get("nob", 0)); nf = int(K.get("f", 0))
    b = _dense_vec(b)
    rng = rng or np.random.default_rng(0)
    _say(verbose, "ManiSDP is starting...")                # :30-31
    _say(verbose, f"SDP size: n = {max(nset)}, m = {b.size}")
    call, B, Apsd, cpsd, dAAt = _dual_matrices(A, c, nf, o)    # :33-44
    p = _block_widths(o, nset)                             # :50-55
    _block_reshape_option(o)
    h = _lib.Handle.dual_multiblock(Apsd, b, cpsd, dAAt, nset, nob, B, call[:nf], pcap=max(32, max(p) + 2 * int(o["delta"])))
    try:
        geo = _Blocks(h, o, nset, nob, strict_rank=True)  # :146-155 (r = sum(e > theta*e(1)), at least 1)
        t = _Kind(geo, _dual_side(h, call, nf), int(o["ADMM_maxiter"]), _gap_dual, (50, 100),   # :133-143
                  "ManiDSDP: optimum = %0.8f, time = %0.2fs")
        obj, data, (Yb, w, _, _, p, _, _) = _al_loop(h, o, t, geo.start(rng, p), p, np.zeros(nf), verbose)
        Yb = data["Y"] = geo.final(Yb, p)
        X = [h.get_dual_slack_block(geo.r0[i], nset[i]) for i in range(len(nset))] if obj is not None else None
        y = h.dual_get_y() if obj is not None else None
    finally:
        h.close()
    data.update({"X": X, "y": y, "S": ([Yi @ Yi.T for Yi in Yb] if Yb is not None else None), "w": w,
                 "p": [Yi.shape[1] for Yi in (Yb or [])]})
    return X, obj, data
