#!/usr/bin/env python
"""Times the persistent single-launch tCG of the block kinds (option "block_persist", msdp_blockpersist.hip) against the generic
three-launch trips of the SAME handle on the SAME tree -- the option-off path is the yardstick.
Instances: problems.rotation_synchronization(n, 3, 8, 0.5, 0) ("rot") and problems.pose_graph(n, 3, 8, 0.1, 0.1, 0) ("pose") at
n = --n (10 000) and --small (1000).
  trips_KIND_N   at p = 8 and p = 32 on one handle: the trip time of msdp_bench_tcg_trip (--reps trips, exits disabled), option
                 off and on in alternating rounds -- median of --rounds with the range; then ONE trustregions() call per path from
                 the same start (maxiter 40, maxinner 100, tolgradnorm 1e-8): its counts, last_rtr_device_ms, and the split the
                 option "timing" prints (tCG phase against retract + cost + decide + sync); and the trip time with the A/B
                 switch "block_persist_wide" (the largest grid at the same row slots)
  solve_KIND_N   the whole solve (solvers.ManiSDP_onlyunitblockdiag / ManiSDP_posegraph, defaults, tol 1e-8), option off and on
                 alternating: wall clock, one warm-up solve each, median of --runs
No ratio is asserted.  Without --step this process opens no device: it runs every step as a child process of its own under
`timeout`, one after the other, stops at the first step that fails or runs out of time, and prints one JSON line.
Usage: python tools/time_block_persist.py [--n N] [--small N] [--reps R] [--rounds K] [--runs K] [--only SUBSTRING] [--step NAME]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, DEGREE = 3, 8


def steps(a):
    out = []
    for n in (a.n, a.small):
        for kind in ("rot", "pose"):
            out.append(("trips_%s_%d" % (kind, n), 240))
    for n in (a.n, a.small):
        for kind in ("rot", "pose"):
            out.append(("solve_%s_%d" % (kind, n), 420))
    return out


def _instance(kind, n):
    from manisdp_matlab_amd import problems
    if kind == "rot":
        return problems.rotation_synchronization(n, D, DEGREE, 0.5, 0)[0]
    return problems.pose_graph(n, D, DEGREE, 0.1, 0.1, 0)[0]


def _point(kind, n, p):
    g = np.random.default_rng(1)
    B = D + (kind == "pose")
    Y = np.zeros((n, B, p))
    for i in range(n):
        Y[i, :D] = np.linalg.qr(g.standard_normal((p, D)))[0].T
    return Y.reshape(n * B, p)


def _with_stderr(fn):
    """fn() with the process's stderr (the library's timing lines) captured; returns (result, text)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            res = fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        return res, tmp.read().decode(errors="replace")


def _trips(a, kind, n):
    from manisdp_matlab_amd import _lib
    C = _instance(kind, n)
    h = _lib.Handle.onlyunitblockdiag(C, D, pcap=32) if kind == "rot" else _lib.Handle.posegraph(C, D, pcap=32)
    out = {"kind": kind, "n": n, "N": int(C.shape[0]), "reps": a.reps, "rounds": a.rounds}
    try:
        for p in (8, 32):
            Y = _point(kind, n, p)
            rec = {}
            us = {0: [], 1: []}
            for on in (0, 1):                               # warm-up: clocks, graph instantiation, occupancy query
                h.set_option("block_persist", on)
                h.set_point(Y)
                rec["tcg_path_%s" % ("on" if on else "off")] = h.tcg_path()
                h.bench_tcg_trip(a.reps)
            for _ in range(a.rounds):                       # alternate the paths
                for on in (0, 1):
                    h.set_option("block_persist", on)
                    h.set_point(Y)
                    us[on].append(1e3 * h.bench_tcg_trip(a.reps))
            for on, name in ((0, "off"), (1, "on")):
                rec["trip_us_" + name] = {"median": float(np.median(us[on])), "min": float(min(us[on])), "max": float(max(us[on]))}
            h.set_option("block_persist", 1)
            h.set_point(Y)
            rec["plan"] = h.block_persist_plan()
            h.set_option("block_persist_wide", 1)           # A/B: the largest grid at the same row slots
            h.set_point(Y)
            rec["plan_wide"] = h.block_persist_plan()
            h.bench_tcg_trip(a.reps)
            w = [1e3 * h.bench_tcg_trip(a.reps) for _ in range(a.rounds)]
            rec["trip_us_on_wide"] = {"median": float(np.median(w)), "min": float(min(w)), "max": float(max(w))}
            h.set_option("block_persist_wide", 0)
            h.set_option("timing", 1)
            for on, name in ((0, "off"), (1, "on"), (0, "off2"), (1, "on2")):      # the second pair: warm
                h.set_option("block_persist", on)
                h.set_point(Y)
                t0 = time.perf_counter()
                st, text = _with_stderr(lambda: h.rtr(_lib.default_opts(maxiter=40, maxinner=100, tolgradnorm=1e-8)))
                wall = time.perf_counter() - t0
                m = re.search(r"tCG phase ([0-9.]+) ms\s+\(retract\+cost\+decide\+sync\) ([0-9.]+) ms", text)
                rec["rtr_" + name] = {"iters": st.iters, "hessvecs": st.hessvecs, "accepted": st.accepted, "rejected": st.rejected,
                                      "cost": st.cost, "gradnorm": st.gradnorm, "wall_ms": 1e3 * wall,
                                      "device_ms": h.last_rtr_device_ms(),
                                      "tcg_phase_ms": float(m.group(1)) if m else None, "rest_ms": float(m.group(2)) if m else None}
            h.set_option("timing", 0)
            out["p%d" % p] = rec
    finally:
        h.close()
    return out


def _solve(a, kind, n):
    from manisdp_matlab_amd import solvers
    C = _instance(kind, n)
    fn = solvers.ManiSDP_onlyunitblockdiag if kind == "rot" else solvers.ManiSDP_posegraph
    ts = {False: [], True: []}
    last = {}
    for rep in range(a.runs + 1):                           # one warm-up solve each, then alternate
        for on in (False, True):
            t0 = time.perf_counter()
            last[on] = fn(C, D, {"tol": 1e-8, "block_persist": on}, verbose=False)
            if rep:
                ts[on].append(time.perf_counter() - t0)
    out = {"kind": kind, "n": n, "runs": a.runs}
    for on, name in ((False, "off"), (True, "on")):
        Y, obj, data = last[on]
        out[name] = {"seconds": float(np.median(ts[on])), "all_seconds": [float(t) for t in ts[on]], "obj": float(obj),
                     "dinf": float(data["dinf"]), "status": int(data["status"]), "iters": int(data["iters"]),
                     "hessvecs": int(data["hessvecs"]), "rtr_seconds": float(data["rtr_seconds"]), "p": int(Y.shape[1])}
    return out


def run_step(a):
    from manisdp_matlab_amd import _lib
    _lib.load()
    what, kind, n = a.step.split("_")
    if what == "trips":
        return _trips(a, kind, int(n))
    if what == "solve":
        return _solve(a, kind, int(n))
    raise SystemExit("unknown step %r" % a.step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--small", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step:
        print(json.dumps(run_step(a)), flush=True)
        return 0
    out = {"date": time.strftime("%Y-%m-%d"), "d": D, "degree": DEGREE}
    passed = [x for x in sys.argv[1:]]
    for name, seconds in steps(a):
        if a.only and a.only not in name:
            continue
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__)] + passed + ["--step", name]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:                               # a failed or timed-out step: nothing more is started on the device
            out[name] = {"failed": r.returncode}
            print(json.dumps(out), flush=True)
            return 1
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps({name: out[name]}), flush=True)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
