#!/usr/bin/env python
"""Times msdp_round_phases (Handle.round_phases) after a solve, on problems.phase_synchronization(--n, 8, 1.0) (rounded with M = 0)
and problems.mpsk_synchronization(--n, 8, 0.5, 4) (rounded with M = 4): the rounding alone (sweeps = 0) and with --sweeps sweeps,
at T in {64, 256, 1024}; beside them the time of the solve that precedes the rounding and the NumPy restatement
(tests/phase_round_ref.py) at T = 64.  Host timing around the synchronous call, the median of --runs calls after one warm-up
call.  No figure is asserted.  Prints one JSON line.
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


def _med(fn, runs):
    ts = []
    for rep in range(runs + 1):
        t0 = time.perf_counter()
        out = fn()
        if rep:
            ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    from manisdp_matlab_amd import _lib, problems, solvers
    out = {"date": time.strftime("%Y-%m-%d"), "n": a.n, "sweeps": a.sweeps, "runs": a.runs}
    for name, M in (("sync", 0), ("mpsk4", 4)):
        g = np.random.default_rng(0)
        C = (problems.phase_synchronization(a.n, 8, 1.0, g) if M == 0 else problems.mpsk_synchronization(a.n, 8, 0.5, 4, g))[0]
        t0 = time.perf_counter()
        Y, obj, data = solvers.ManiSDP_onlyunitdiag(C, {"tol": 1e-8}, verbose=False)
        res = {"M": M, "solve_seconds": time.perf_counter() - t0, "obj": float(obj), "p": int(Y.shape[1]), "iters": int(data["iters"])}
        h = _lib.Handle.onlyunitdiag_hermitian(C, pcap=max(32, Y.shape[1]))
        try:
            h.set_point(Y)
            for T in (64, 256, 1024):
                R = solvers._draw_phase_R(np.random.default_rng(1), T, Y.shape[1])
                t_r, r0 = _med(lambda: h.round_phases(R, M=M, sweeps=0), a.runs)
                t_s, r1 = _med(lambda: h.round_phases(R, M=M, sweeps=a.sweeps), a.runs)
                res["T%d" % T] = {"round_ms": 1e3 * t_r, "round_sweeps_ms": 1e3 * t_s, "value0": float(r0["values"].min()),
                                  "value": float(r1["values"].min()), "sweeps_run": int(r1["info"][0].max())}
        finally:
            h.close()
        if not a.no_ref:
            import phase_round_ref as PR
            R = solvers._draw_phase_R(np.random.default_rng(1), 64, Y.shape[1])
            t0 = time.perf_counter()
            PR.round_phases(C, Y, R, M, 0)
            t1 = time.perf_counter()
            PR.round_phases(C, Y, R, M, a.sweeps)
            res["numpy_T64"] = {"round_ms": 1e3 * (t1 - t0), "round_sweeps_ms": 1e3 * (time.perf_counter() - t1)}
        out[name] = res
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
