#!/usr/bin/env python
"""Times the pose-graph kind (msdp_create_posegraph_csc: block CSR of block order d + 1 on stacked Stiefel x Euclidean) and, as
the yardstick, the only other way to pose the same SDP here: the generic affine ManiSDP handle with the n d (d + 1) / 2
constraints X_kk = 1, X_kl = 0 on the leading d x d part of every diagonal block.
  hessvec_pose   the Hess-vec of the pose handle on problems.pose_graph(10 000, 3, 8, 0.1, 0.1, 0) at p = 8
                 (msdp_bench_hessvec: device events around graph replays; one warm-up call, the median of --rounds calls of --reps),
                 with the algorithmic bytes of the block-CSR product and the rate they give
  solve_pose     solvers.ManiSDP_posegraph on the same instance with its defaults (wall clock, one warm-up solve, median of --runs)
  hessvec_small  the Hess-vec of both handles at n = 1000 (alternating rounds)
  solve_small    both solves at n = 1000 (solvers.ManiSDP_posegraph / solvers.ManiSDP, alternating)
The affine handle holds dense order-N operands, which is why it is timed at n = 1000 only.  No ratio is asserted: the affine
route is the yardstick, not the code under test.
Without --step this process opens no device: it runs every step as a child process of its own under `timeout`, one after the
other, stops at the first step that fails or runs out of time, and prints one JSON line with what the steps returned.
--escape-method 2: the solves of the pose handle run the block eigen-solver of the escape on block storage (0: Lanczos); a solve
row carries eig_seconds, the escape's steps and calls and the trustregions() seconds beside the total.
Usage: python tools/time_posegraph.py [--n N] [--small N] [--d D] [--p P] [--reps R] [--rounds K] [--runs K] [--step NAME] [--escape-method {0,2}]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("hessvec_pose", 120), ("solve_pose", 240), ("hessvec_small", 120), ("solve_small", 300))   # (name, seconds)


def affine_formulation(C, d):
    """(At, b, c) of the same SDP for the generic affine handle: per block X_kk = 1 for its d rotation rows and X_kl = 0 for
    k < l among them (entries 1/2 at (k, l) and (l, k)); the free row carries no constraint."""
    N = C.shape[0]
    B = d + 1
    n = N // B
    ka, la = np.triu_indices(d, 0)
    k = (np.arange(n)[:, None] * B + ka[None]).ravel().astype(np.int64)
    l = (np.arange(n)[:, None] * B + la[None]).ravel().astype(np.int64)
    m = k.size
    rows = np.concatenate([k + l * N, l + k * N])
    cols = np.concatenate([np.arange(m), np.arange(m)])
    At = sp.csc_matrix((np.full(2 * m, 0.5), (rows, cols)), shape=(N * N, m))      # a diagonal entry gets 1/2 + 1/2
    return At, (k == l).astype(np.float64), C.toarray().ravel()


def _point(n, d, p):
    g = np.random.default_rng(1)
    Y = np.empty((n, d + 1, p))
    for i in range(n):
        Y[i, :d] = np.linalg.qr(g.standard_normal((p, d)))[0].T
    Y[:, d, :] = g.standard_normal((n, p))
    return Y.reshape(n * (d + 1), p)


def _hessvec(a, n, with_affine):
    from manisdp_matlab_amd import _lib, problems
    d, p = a.d, a.p
    C, _, _, edges, _, _ = problems.pose_graph(n, d, a.degree, a.sigma, a.sigma, 0)
    N = C.shape[0]
    out = {"n": n, "N": N, "p": p, "edges": int(edges.shape[0]), "nnz": int(C.nnz), "reps": a.reps, "rounds": a.rounds}
    handles = {"pose": _lib.Handle.posegraph(C, d, pcap=p)}
    if with_affine:
        At, b, c = affine_formulation(C, d)
        handles["affine"] = _lib.Handle.affine(_lib.KIND_GENERIC, At, b, c, N, pcap=p)
    try:
        Y = _point(n, d, p)
        for h in handles.values():
            h.set_point(Y)
            h.bench_hessvec(a.reps)                      # warm-up: clocks, caches, the graph instantiation
        us = {k: [] for k in handles}
        algo = {}
        for _ in range(a.rounds):                        # alternate the handles
            for k, h in handles.items():
                ms, by, fl = h.bench_hessvec(a.reps)
                us[k].append(1e3 * ms)
                algo[k] = (by, fl)
        for k in handles:
            med = float(np.median(us[k]))
            out[k] = {"us": med, "all_us": [float(x) for x in us[k]], "algo_bytes": algo[k][0], "algo_flops": algo[k][1],
                      "algo_GBps": algo[k][0] / (1e-6 * med) / 1e9, "tcg_path": handles[k].tcg_path()}
    finally:
        for h in handles.values():
            h.close()
    return out


def _solve(a, n, with_affine):
    from manisdp_matlab_amd import problems, solvers
    d = a.d
    C, R_true, t_true, edges, _, _ = problems.pose_graph(n, d, a.degree, a.sigma, a.sigma, 0)
    N = C.shape[0]

    def solve_pose():
        return solvers.ManiSDP_posegraph(C, d, {"tol": 1e-8, "escape_method": a.escape_method, "escape_stats": True}, verbose=False)

    solves = {"pose": solve_pose}
    if with_affine:
        At, b, c = affine_formulation(C, d)
        solves["affine"] = lambda: solvers.ManiSDP(At, b, c, {"s": N}, {"tol": 1e-8}, verbose=False)
    ts = {k: [] for k in solves}
    last = {}
    for rep in range(a.runs + 1):                        # one warm-up solve each, then alternate
        for k, fn in solves.items():
            t0 = time.perf_counter()
            last[k] = fn()
            if rep:
                ts[k].append(time.perf_counter() - t0)
    out = {"n": n, "N": N, "runs": a.runs}
    for k in solves:
        Ys, obj, data = last[k]
        out[k] = {"seconds": float(np.median(ts[k])), "all_seconds": [float(t) for t in ts[k]], "obj": float(obj),
                  "dinf": float(data.get("dinf", float("nan"))), "status": int(data.get("status", -1)),
                  "iters": int(data.get("iters", 0)), "hessvecs": int(data.get("hessvecs", 0)),
                  "rtr_seconds": float(data.get("rtr_seconds", 0.0)), "eig_seconds": float(data.get("eig_seconds", 0.0)),
                  "eig_calls": int(data.get("eig_calls", 0)), "eig_steps": int(data.get("eig_steps", 0)),
                  "eig_verify_steps": int(data.get("eig_verify_steps", 0)), "escape_method_ran": int(data.get("escape_method", -1))}
    Ys, obj, data = last["pose"]
    er, et = problems.pose_error(*problems.round_poses(Ys, d), R_true, t_true)
    out["pose"].update(gap=float(data["gap"]), p=int(Ys.shape[1]), rotation_error=er, position_error=et)
    return out


def run_step(a):
    from manisdp_matlab_amd import _lib
    _lib.load()
    if a.step == "hessvec_pose":
        return _hessvec(a, a.n, False)
    if a.step == "solve_pose":
        return _solve(a, a.n, False)
    if a.step == "hessvec_small":
        return _hessvec(a, a.small, True)
    if a.step == "solve_small":
        return _solve(a, a.small, True)
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
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
        if r.returncode != 0:                            # a failed or timed-out step: nothing more is started on the device
            out[name] = {"failed": r.returncode}
            print(json.dumps(out), flush=True)
            return 1
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
