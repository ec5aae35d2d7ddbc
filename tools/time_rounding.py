#!/usr/bin/env python
"""Times msdp_round_hyperplane (Handle.round_hyperplane) on the solutions of the G1 and G81 MaxCut relaxations
(ManiSDP_onlyunitdiag, options.p0 = 40, KKT 1e-8): the call at T = 64, 1024 and 4096 trials, with sweeps = 0 (rounding and
values only) and with the 1-opt sweeps run to convergence, next to the time of the solve, the best value and the sweeps used.
Every figure is the median over --runs calls after one warm-up call; wall time around the C call, uploads of R and downloads of
the results included.  Both visiting orders of the sweeps (set_option("round_order", 0 / 1): rows in index order, rows by colour
class) run on one handle, alternating call by call; per order the time of a sweep, (call with sweeps - call without) / sweeps
run by the slowest word.  One JSON line.
Usage: python tools/time_rounding.py [--runs N] [--graphs G1,G81]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_SWEEPS = 1000


ORDERS = ("index", "color")


def _time(h, R, sweeps, runs):
    """{order: (median ms, result)}: the two orders alternate call by call after one warm-up call each."""
    ts, res = {o: [] for o in ORDERS}, {}
    for rep in range(runs + 1):
        for k, o in enumerate(ORDERS):
            h.set_option("round_order", k)
            t0 = time.perf_counter()
            res[o] = h.round_hyperplane(R, sweeps=sweeps)
            if rep:
                ts[o].append(time.perf_counter() - t0)
    h.set_option("round_order", 0)
    return {o: (1e3 * float(np.median(ts[o])), res[o]) for o in ORDERS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--graphs", default="G1,G81")
    a = ap.parse_args()
    from manisdp_matlab_amd import _lib, problems, solvers
    _lib.load()
    out = {"runs": a.runs, "options": "p0 = 40, tol = 1e-8", "graphs": {}}
    for name in a.graphs.split(","):
        C = problems.maxcut_cost_matrix(os.path.join(ROOT, "tests", "golden", name + ".txt.gz"))
        solve = []
        for rep in range(3):
            t0 = time.perf_counter()
            Y, fval, data = solvers.ManiSDP_onlyunitdiag(C, {"p0": 40, "tol": 1e-8}, verbose=False)
            solve.append(time.perf_counter() - t0)
        g = {"n": int(C.shape[0]), "p": int(Y.shape[1]), "fval": float(fval), "solve_ms": 1e3 * float(np.median(solve[1:])), "T": {}}
        h = _lib.Handle.onlyunitdiag(C.tocsr(), pcap=max(32, Y.shape[1]))
        try:
            h.set_point(Y)
            g["colors"] = int(h.round_coloring()[0])
            for T in (64, 1024, 4096):
                R = np.random.default_rng(T).standard_normal((T, Y.shape[1]))
                t0, t1 = _time(h, R, 0, a.runs), _time(h, R, MAX_SWEEPS, a.runs)
                g["T"][str(T)] = {}
                for o in ORDERS:
                    (ms0, r0), (ms1, r1) = t0[o], t1[o]
                    g["T"][str(T)][o] = {"round_ms": ms0, "best0": float(r0["values"].min()), "ratio0": float(r0["values"].min() / fval),
                                         "round_1opt_ms": ms1, "best": float(r1["values"].min()), "ratio": float(r1["values"].min() / fval),
                                         "sweeps_max": int(r1["info"][0].max()), "sweeps_mean": float(r1["info"][0].mean()),
                                         "sweep_ms": (ms1 - ms0) / max(1, int(r1["info"][0].max())),
                                         "converged": bool(not r1["info"][1].any())}
        finally:
            h.close()
        out["graphs"][name] = g
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
