#!/usr/bin/env python
"""Times options["block_factor"] = "device" of the two block kinds (msdp_blockfactor.hip: the rank decision, cut, widening and
re-orthonormalisation of the factor on the device between the trustregions() calls) against the host path of the same tree,
"host" and "device" alternating, the median of --runs solves each after one warm-up solve per setting:
  pose_large   problems.pose_graph(--n, d, degree, sigma, sigma, 0) with ManiSDP_posegraph at its defaults and with
               precon = "blockjacobi", each with and without block_persist
  rot_large    problems.rotation_synchronization(--n, d, degree, noise, 0) with ManiSDP_onlyunitblockdiag from p0 = d, the noise
               raised along NOISES until a certified solve takes at least two outer iterations (the staircase has to fire); the
               last noise is kept where none does, and the reported status says so
  small        both at --small
  calls        at --n and width --p, per kind: blockfactor_gram, blockfactor_rotate (p -> p - 1) and blockfactor_append (k = 1)
               timed singly (the point is uploaded again before every call, outside the timing), the host's polar
               re-orthonormalisation of the same factor, and the rounding: problems.round_rotations / round_poses against
               Handle.round_blocks() (wall clock, W from the device's Gram matrix included)
Per solve setting: whole solve seconds, factor_seconds per outer iteration, outer iterations, device calls, host fallbacks,
optimum, and eig_seconds, the escape's steps and calls and the trustregions() seconds.  --escape-method 2: every solve runs the
block eigen-solver of the escape on block storage (0: Lanczos).  No ratio is asserted: the figures are reported as they come out.
Without --step this process opens no device: it runs every step as a child process of its own under `timeout`, one after the
other, stops at the first step that fails or runs out of time, and prints one JSON line with what the steps returned.
Usage: python tools/time_block_factor.py [--n N] [--small N] [--d D] [--degree K] [--sigma S] [--p P] [--runs K] [--step NAME] [--escape-method {0,2}]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("pose_large", 420), ("rot_large", 420), ("small", 300), ("calls", 240))   # (name, seconds)
NOISES = (0.5, 1.0, 1.5, 2.0, 3.0)


def _med(xs):
    return float(np.median(xs))


def _solves(solve, C, d, base, runs):
    """host against device for one option set: one warm-up solve each, then alternating."""
    ts = {"host": [], "device": []}
    res = {}
    for rep in range(runs + 1):
        for mode in ("host", "device"):
            t0 = time.perf_counter()
            res[mode] = solve(C, d, dict(base, block_factor=mode), verbose=False)
            if rep:
                ts[mode].append(time.perf_counter() - t0)
    out = {}
    for mode in ("host", "device"):
        Y, obj, data = res[mode]
        out[mode] = {"solve_seconds": _med(ts[mode]), "all_solve_seconds": [float(t) for t in ts[mode]],
                     "factor_seconds_per_iter": float(data["factor_seconds"]) / max(int(data["iters"]), 1),
                     "factor_seconds": float(data["factor_seconds"]), "rtr_seconds": float(data["rtr_seconds"]),
                     "eig_seconds": float(data["eig_seconds"]), "eig_calls": int(data.get("eig_calls", 0)), "eig_steps": int(data.get("eig_steps", 0)),
                     "eig_verify_steps": int(data.get("eig_verify_steps", 0)), "escape_method_ran": int(data.get("escape_method", -1)), "iters": int(data["iters"]), "reruns": int(data.get("reruns", 0)),
                     "device_calls": int(data["factor_device_calls"]), "host_fallbacks": int(data["factor_host_fallbacks"]),
                     "obj": float(obj), "dinf": float(data["dinf"]), "status": int(data["status"]), "p_final": int(Y.shape[1])}
    return out


def _pose(a, n):
    from manisdp_matlab_amd import problems, solvers
    C = problems.pose_graph(n, a.d, a.degree, a.sigma, a.sigma, 0)[0]
    out = {"n": n, "N": int(C.shape[0]), "runs": a.runs}
    for name, base in (("default", {}), ("persist", {"block_persist": True}), ("precon", {"precon": "blockjacobi"}),
                       ("precon_persist", {"precon": "blockjacobi", "block_persist": True})):
        out[name] = _solves(solvers.ManiSDP_posegraph, C, a.d, dict(base, tol=1e-8, escape_method=a.escape_method, escape_stats=True), a.runs)
    return out


def _rot(a, n):
    from manisdp_matlab_amd import problems, solvers
    out = {"n": n, "runs": a.runs}
    for noise in NOISES:                                     # raised until the staircase fires from p0 = d
        C = problems.rotation_synchronization(n, a.d, a.degree, noise, 0)[0]
        _, _, data = solvers.ManiSDP_onlyunitblockdiag(C, a.d, {"tol": 1e-8, "p0": a.d, "block_factor": "device", "escape_method": a.escape_method, "escape_stats": True}, verbose=False)
        if data["iters"] >= 2 and data["status"] == 0:
            break
    out.update(noise=noise, N=int(C.shape[0]))
    for name, base in (("default", {}), ("persist", {"block_persist": True})):
        out[name] = _solves(solvers.ManiSDP_onlyunitblockdiag, C, a.d, dict(base, tol=1e-8, p0=a.d, escape_method=a.escape_method, escape_stats=True), a.runs)
    return out


def _timed(fn, prepare, runs):
    ts = []
    for rep in range(runs + 1):
        prepare()
        t0 = time.perf_counter()
        fn()
        if rep:
            ts.append(time.perf_counter() - t0)
    return _med(ts)


def _calls(a):
    from manisdp_matlab_amd import _lib, problems, solvers
    n, d, p = a.n, a.d, a.p
    g = np.random.default_rng(1)
    out = {"n": n, "p": p, "runs": a.runs}
    for kind in ("rotations", "poses"):
        ef = 1 if kind == "poses" else 0
        B = d + ef
        if ef:
            C = problems.pose_graph(n, d, a.degree, a.sigma, a.sigma, 0)[0]
            h = _lib.Handle.posegraph(C, d, pcap=p + 2)
            polar, rounding = solvers._polar_rotation_rows, problems.round_poses
        else:
            C = problems.rotation_synchronization(n, d, a.degree, a.sigma, 0)[0]
            h = _lib.Handle.onlyunitblockdiag(C, d, pcap=p + 2)
            polar, rounding = solvers._polar_blocks, problems.round_rotations
        Y = np.zeros((n, B, p))
        for i in range(n):
            Y[i, :d] = np.linalg.qr(g.standard_normal((p, d)))[0].T
        if ef:
            Y[:, d] = g.standard_normal((n, p))
        Y = Y.reshape(n * B, p)
        Q = np.linalg.qr(g.standard_normal((p, p)))[0][:, :p - 1]
        V = g.standard_normal((n * B, 1))
        try:
            put = lambda: h.set_point(Y)
            out[kind] = {
                "gram_ms": 1e3 * _timed(lambda: h.blockfactor_gram(), put, a.runs),
                "rotate_ms": 1e3 * _timed(lambda: h.blockfactor_rotate(Q), put, a.runs),
                "append_ms": 1e3 * _timed(lambda: h.blockfactor_append(V, 0.5), put, a.runs),
                "set_point_ms": 1e3 * _timed(put, lambda: None, a.runs),
                "get_point_ms": 1e3 * _timed(lambda: h.get_point(), put, a.runs),
                "host_polar_ms": 1e3 * _timed(lambda: polar(Y, d), lambda: None, a.runs),
                "host_gram_eigh_ms": 1e3 * _timed(lambda: solvers._thin_svd_rank(Y, 0.1), lambda: None, a.runs),
                "round_device_ms": 1e3 * _timed(lambda: h.round_blocks(), put, a.runs),
                "round_host_ms": 1e3 * _timed(lambda: rounding(Y, d), lambda: None, a.runs)}
        finally:
            h.close()
    return out


def run_step(a):
    from manisdp_matlab_amd import _lib
    _lib.load()
    if a.step == "pose_large":
        return _pose(a, a.n)
    if a.step == "rot_large":
        return _rot(a, a.n)
    if a.step == "small":
        return {"pose": _pose(a, a.small), "rot": _rot(a, a.small)}
    if a.step == "calls":
        return _calls(a)
    raise SystemExit("unknown step %r" % a.step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--small", type=int, default=1000)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--degree", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--step", default=None)
    ap.add_argument("--escape-method", type=int, choices=(0, 2), default=0)
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
