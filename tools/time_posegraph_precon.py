#!/usr/bin/env python
"""Times the block-Jacobi preconditioned tCG of the pose-graph kind (msdp_set_option "precon", msdp_pose_precon.hip) against
the unpreconditioned generic path, option off and on on the SAME handle, alternating, the median of --runs runs each:
  trip     one tCG trip (msdp_bench_tcg_trip: exits disabled, device events around graph replays of the three launches)
  rtr      one trustregions() call from a fixed start at width p: Hess-vecs, TR iterations, seconds (msdp_rtr_stats)
  solve    solvers.ManiSDP_posegraph with its defaults (wall clock, one warm-up solve per setting, then alternating): Hess-vecs,
           outer iterations, seconds, optimum, dinf, gap
Steps: `large` = problems.pose_graph(n, d, degree, sigma, sigma, 0) with --n (default 10 000); `small` the same at --small (1000,
the instance of the README row); `weighted` = pose_graph(--small, ..., kappa = 100): rotation and translation terms of the
diagonal blocks two orders of magnitude apart.  No ratio is asserted: the figures are reported as they come out.
Without --step this process opens no device: it runs every step as a child process of its own under `timeout`, one after the
other, stops at the first step that fails or runs out of time, and prints one JSON line with what the steps returned.
Usage: python tools/time_posegraph_precon.py [--n N] [--small N] [--d D] [--degree K] [--sigma S] [--p P] [--reps R] [--runs K] [--step NAME]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("large", 420), ("small", 240), ("weighted", 240))   # (name, seconds)


def _point(n, d, p):
    g = np.random.default_rng(1)
    Y = np.zeros((n, d + 1, p))
    for i in range(n):
        Y[i, :d] = np.linalg.qr(g.standard_normal((p, d)))[0].T
    return Y.reshape(n * (d + 1), p)                         # the solver's kind of start: zeros in the free rows


def _med(xs):
    return float(np.median(xs))


def _measure(a, n, kappa):
    from manisdp_matlab_amd import _lib, problems, solvers
    d, p = a.d, a.p
    C = problems.pose_graph(n, d, a.degree, a.sigma, a.sigma, 0, kappa=kappa)[0]
    out = {"n": n, "N": int(C.shape[0]), "p": p, "kappa": kappa, "nnz": int(C.nnz), "runs": a.runs, "reps": a.reps}
    Y = _point(n, d, p)
    opts = _lib.default_opts(maxiter=40, maxinner=100, tolgradnorm=1e-8)
    trip = {0: [], 1: []}
    rtr = {0: [], 1: []}
    last = {}
    h = _lib.Handle.posegraph(C, d, pcap=p)
    try:
        for on in (0, 1):                                    # warm-up: code objects, the graph instantiation, M_i^-1
            h.set_option("precon", on)
            h.set_point(Y)
            h.bench_tcg_trip(a.reps)
            h.rtr(opts)
        for _ in range(a.runs):
            for on in (0, 1):
                h.set_option("precon", on)
                h.set_point(Y)
                trip[on].append(1e3 * h.bench_tcg_trip(a.reps))
                h.set_point(Y)
                st = h.rtr(opts)
                rtr[on].append(st.seconds)
                last[on] = st
        for on in (0, 1):
            st = last[on]
            out["on" if on else "off"] = {
                "trip_us": _med(trip[on]), "all_trip_us": [float(x) for x in trip[on]],
                "rtr_seconds": _med(rtr[on]), "all_rtr_seconds": [float(x) for x in rtr[on]],
                "rtr_hessvecs": int(st.hessvecs), "rtr_iters": int(st.iters), "rtr_cost": float(st.cost),
                "rtr_gradnorm": float(st.gradnorm), "tcg_path": h.tcg_path()}
    finally:
        h.close()
    settings = {"off": None, "on": "blockjacobi"}
    ts = {k: [] for k in settings}
    res = {}
    for rep in range(a.runs + 1):                            # one warm-up solve each, then alternate
        for k, v in settings.items():
            t0 = time.perf_counter()
            res[k] = solvers.ManiSDP_posegraph(C, d, {"tol": 1e-8, "precon": v}, verbose=False)
            if rep:
                ts[k].append(time.perf_counter() - t0)
    for k in settings:
        Ys, obj, data = res[k]
        out[k].update(solve_seconds=_med(ts[k]), all_solve_seconds=[float(t) for t in ts[k]], solve_hessvecs=int(data["hessvecs"]),
                      solve_iters=int(data["iters"]), obj=float(obj), dinf=float(data["dinf"]), gap=float(data["gap"]),
                      status=int(data["status"]), p_final=int(Ys.shape[1]))
    return out


def run_step(a):
    from manisdp_matlab_amd import _lib
    _lib.load()
    if a.step == "large":
        return _measure(a, a.n, 1.0)
    if a.step == "small":
        return _measure(a, a.small, 1.0)
    if a.step == "weighted":
        return _measure(a, a.small, 100.0)
    raise SystemExit("unknown step %r" % a.step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--small", type=int, default=1000)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--degree", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(run_step(a)), flush=True)
        return 0
    out = {"date": time.strftime("%Y-%m-%d"), "d": a.d, "degree": a.degree, "sigma": a.sigma}
    passed = [x for x in sys.argv[1:]]
    for name, seconds in STEPS:
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__)] + passed + ["--step", name]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:                                # a failed or timed-out step: nothing more is started on the device
            out[name] = {"failed": r.returncode}
            print(json.dumps(out), flush=True)
            return 1
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
