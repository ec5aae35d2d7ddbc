#!/usr/bin/env python
"""Times options["hermitian_factor"] = "device" of the complex unit-diagonal solver (msdp_hfactor_gram / _rotate / _append: the
rank decision, the cut and the widening of the factor on the device between the trustregions() calls) against the host path of
the same tree -- the method of tools/time_block_factor.py: "host" and "device" alternate, the median of --runs solves each after
one warm-up solve per setting.  Instance: problems.phase_synchronization(--n, 8, --sigma) at the solver's defaults (sigma = 1:
four outer iterations at n = 20 000, so the re-shaping runs three times).  Per setting: whole solve seconds, factor_seconds per
outer iteration (transfers of the factor, rank decision, cut, widening), outer iterations, optimum; a progress line per solve
goes to stderr.  No ratio is asserted.  Prints one JSON line.
--escape-method 2 runs every solve with the block eigen-solver of the escape on a complex panel (options["escape_method"]; 0, the
default, keeps the Lanczos path on the real view); the output names the method the last escape call ran.
Usage: python tools/time_hermitian_factor.py [--n N] [--sigma S] [--runs K] [--escape-method {0,2}]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--escape-method", type=int, choices=(0, 2), default=0)
    a = ap.parse_args()
    from manisdp_matlab_amd import problems, solvers
    C = problems.phase_synchronization(a.n, 8, a.sigma, np.random.default_rng(0))[0]
    ts = {"host": [], "device": []}
    res = {}
    for rep in range(a.runs + 1):
        for mode in ("host", "device"):
            t0 = time.perf_counter()
            res[mode] = solvers.ManiSDP_onlyunitdiag(C, {"tol": 1e-8, "hermitian_factor": mode, "escape_method": a.escape_method}, verbose=False)
            if rep:
                ts[mode].append(time.perf_counter() - t0)
            print("solve %d (%s): %.2f s, %d outer iterations" % (rep, mode, time.perf_counter() - t0, res[mode][2]["iters"]),
                  file=sys.stderr, flush=True)
    out = {"date": time.strftime("%Y-%m-%d"), "n": a.n, "sigma": a.sigma, "runs": a.runs, "escape_method": a.escape_method}
    for mode in ("host", "device"):
        Y, obj, data = res[mode]
        out[mode] = {"solve_seconds": float(np.median(ts[mode])), "all_solve_seconds": [float(t) for t in ts[mode]],
                     "factor_seconds_per_iter": float(data["factor_seconds"]) / max(int(data["iters"]), 1),
                     "factor_seconds": float(data["factor_seconds"]), "rtr_seconds": float(data["rtr_seconds"]),
                     "eig_seconds": float(data["eig_seconds"]), "escape_method_ran": int(data.get("escape_method", -1)), "iters": int(data["iters"]), "obj": float(obj),
                     "dinf": float(data["dinf"]), "status": int(data["status"]), "p_final": int(Y.shape[1])}
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
