#!/usr/bin/env python
"""Times the saddle escape of the G81 solve bench.py measures (ManiSDP_onlyunitdiag, options.p0 = 40, KKT 1e-8) with the dense
algebra of the block eigen-solver's Rayleigh-Ritz stages on the host (options["escape_rr"] = "host", the default) against the
device stage ("device": k_be_ritz + k_be_res_sum), both in the same process, runs of the two settings alternating:
  * the cold independent check alone (the escape_eigs call with k = 1 that precedes "Optimality is reached!"),
  * the regular escape calls of the solve (four on G81), summed,
  * the whole solve.
Every escape_eigs call of a solve is timed around the C call; one warm-up solve per setting, then the median over --runs solves
(at least five), with the smallest and largest value beside it.  Also printed: the Rayleigh-Ritz stages of a solve by where they ran, and the difference per stage.
Usage: python tools/time_ritz_stage.py [--runs N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _instance():
    from manisdp_matlab_amd import problems
    g81 = os.path.join(ROOT, "tests", "golden", "G81.txt.gz")
    return problems.maxcut_cost_matrix(g81) if os.path.exists(g81) else problems.toroidal_grid_maxcut(100, 200, seed=81)


def _solve(C, mode, calls):
    from manisdp_matlab_amd import solvers
    del calls[:]
    t0 = time.perf_counter()
    _, obj, data = solvers.ManiSDP_onlyunitdiag(C, {"p0": 40, "escape_rr": mode}, verbose=False)
    total = time.perf_counter() - t0
    if data["status"] != 0 or not data["dinf"] < 1e-8:
        raise RuntimeError(f"escape_rr = {mode}: the solve did not reach KKT 1e-8 (status {data['status']}, dinf {data['dinf']:.1e})")
    cold = [t for k, t in calls if k == 1]
    regular = [t for k, t in calls if k != 1]
    return dict(solve_ms=1e3 * total, cold_ms=1e3 * sum(cold), cold_calls=len(cold), regular_ms=1e3 * sum(regular),
                regular_calls=len(regular), stages=data["escape_rr_stages"], obj=obj, iters=data["iters"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    runs = max(5, a.runs)
    from manisdp_matlab_amd import _lib
    _lib.load()
    C = _instance()
    calls = []
    real = _lib.Handle.escape_eigs

    def timed(self, k, *args, **kw):
        t0 = time.perf_counter()
        out = real(self, k, *args, **kw)
        calls.append((k, time.perf_counter() - t0))
        return out

    _lib.Handle.escape_eigs = timed
    try:
        res = {"host": [], "device": []}
        for rep in range(runs + 1):                                  # rep 0 warms both settings up
            for mode in ("host", "device"):
                r = _solve(C, mode, calls)
                if rep:
                    res[mode].append(r)
    finally:
        _lib.Handle.escape_eigs = real
    out = {"instance": "G81, p0 = 40, KKT 1e-8", "runs": runs}
    for mode in ("host", "device"):
        rs = res[mode]
        out[mode] = {key: float(np.median([r[key] for r in rs])) for key in ("cold_ms", "regular_ms", "solve_ms")}
        out[mode]["spread_min_max"] = {key: [float(min(r[key] for r in rs)), float(max(r[key] for r in rs))] for key in ("cold_ms", "regular_ms", "solve_ms")}
        out[mode].update(cold_calls=rs[0]["cold_calls"], regular_calls=rs[0]["regular_calls"], iters=rs[0]["iters"], obj=rs[0]["obj"],
                         stages_device_host_fallback=list(rs[0]["stages"]))
    nst = sum(out["device"]["stages_device_host_fallback"])
    esc = lambda m: out[m]["cold_ms"] + out[m]["regular_ms"]
    out["stages_per_solve"] = nst
    out["escape_ms_per_stage_host_minus_device"] = (esc("host") - esc("device")) / max(nst, 1)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
