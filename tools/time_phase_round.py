#!/usr/bin/env python
"""Times msdp_round_phases (Handle.round_phases) after a solve, on problems.phase_synchronization(--n, 8, 1.0) (rounded with M = 0)
and problems.mpsk_synchronization(--n, 8, 0.5, 4) (rounded with M = 4): the rounding alone (sweeps = 0) and with --sweeps sweeps,
at T in {64, 256, 1024}; beside them the time of the solve that precedes the rounding and the NumPy restatement
(tests/phase_round_ref.py) at T = 64.  Host timing around the synchronous call, the median of --runs calls after one warm-up
call.  No figure is asserted.  Prints one JSON line.
Both visiting orders of the sweeps (set_option("round_order", 0 / 1): rows in index order, rows by colour class) run on one handle,
alternating call by call; per order the time of a sweep, (call with sweeps - call without) / sweeps run by the slowest word.
The synchronisation instance is also rounded with M = 4, so that both kinds of sweep are timed on one matrix.
Usage: python tools/time_phase_round.py [--n N] [--sweeps S] [--runs K] [--no-ref]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


ORDERS = ("index", "color")


def _med(h, fn, runs):
    """{order: (median seconds, result)}: the two orders alternate call by call after one warm-up call each."""
    ts, out = {o: [] for o in ORDERS}, {}
    for rep in range(runs + 1):
        for k, o in enumerate(ORDERS):
            h.set_option("round_order", k)
            t0 = time.perf_counter()
            out[o] = fn()
            if rep:
                ts[o].append(time.perf_counter() - t0)
    h.set_option("round_order", 0)
    return {o: (float(np.median(ts[o])), out[o]) for o in ORDERS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    from manisdp_matlab_amd import _lib, problems, solvers
    out = {"date": time.strftime("%Y-%m-%d"), "n": a.n, "sweeps": a.sweeps, "runs": a.runs}
    for name, M in (("sync", 0), ("sync_M4", 4), ("mpsk4", 4)):
        g = np.random.default_rng(0)
        C = (problems.mpsk_synchronization(a.n, 8, 0.5, 4, g) if name == "mpsk4" else problems.phase_synchronization(a.n, 8, 1.0, g))[0]
        if name == "sync_M4":                                  # the solve of "sync" again would only repeat its figures
            Y, res = out["sync"]["Y"], {"M": M, "p": int(out["sync"]["p"])}
        else:
            t0 = time.perf_counter()
            Y, obj, data = solvers.ManiSDP_onlyunitdiag(C, {"tol": 1e-8}, verbose=False)
            res = {"M": M, "solve_seconds": time.perf_counter() - t0, "obj": float(obj), "p": int(Y.shape[1]), "iters": int(data["iters"])}
        h = _lib.Handle.onlyunitdiag_hermitian(C, pcap=max(32, Y.shape[1]))
        try:
            h.set_point(Y)
            res["colors"] = int(h.round_coloring()[0])
            for T in (64, 256, 1024):
                R = solvers._draw_phase_R(np.random.default_rng(1), T, Y.shape[1])
                t0 = _med(h, lambda: h.round_phases(R, M=M, sweeps=0), a.runs)
                t1 = _med(h, lambda: h.round_phases(R, M=M, sweeps=a.sweeps), a.runs)
                res["T%d" % T] = {}
                for o in ORDERS:
                    (t_r, r0), (t_s, r1) = t0[o], t1[o]
                    res["T%d" % T][o] = {"round_ms": 1e3 * t_r, "round_sweeps_ms": 1e3 * t_s, "value0": float(r0["values"].min()),
                                         "value": float(r1["values"].min()), "sweeps_run": int(r1["info"][0].max()),
                                         "sweep_ms": 1e3 * (t_s - t_r) / max(1, int(r1["info"][0].max()))}
        finally:
            h.close()
        res["Y"] = Y
        if not a.no_ref:
            import phase_round_ref as PR
            R = solvers._draw_phase_R(np.random.default_rng(1), 64, Y.shape[1])
            t0 = time.perf_counter()
            PR.round_phases(C, Y, R, M, 0)
            t1 = time.perf_counter()
            PR.round_phases(C, Y, R, M, a.sweeps)
            res["numpy_T64"] = {"round_ms": 1e3 * (t1 - t0), "round_sweeps_ms": 1e3 * (time.perf_counter() - t1)}
        out[name] = res
    for name in ("sync", "sync_M4", "mpsk4"):
        del out[name]["Y"]
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
