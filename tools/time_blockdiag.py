#!/usr/bin/env python
"""Times the unit-block-diagonal kind (msdp_create_onlyunitblockdiag_csc, block CSR on the stacked Stiefel manifold) against the
only other way to pose the same SDP, the affine ManiSDP_unitdiag handle with the n d (d - 1) / 2 constraints X_kl = 0 on the
off-diagonal entries of the diagonal blocks, on problems.rotation_synchronization(10 000, 3, 8, 0.5, 0) at p = 8:
  (a) the Hess-vec of both handles (msdp_bench_hessvec: device events around graph replays of 50 launches) -- one warm-up call
      per handle, then --rounds alternating rounds, the median per handle; for the new handle also the algorithmic bytes of the
      block-CSR product and the rate they give,
  (b) with --solve: the whole solve of both (solvers.ManiSDP_onlyunitblockdiag / ManiSDP_unitdiag with their defaults, wall
      clock, alternating, median of --runs after one warm-up solve each).
The affine handle holds dense order-N operands (N = n d): 8 N^2 bytes each, 7.2 GB at the default size.  --no-affine leaves
it out (the new handle alone).  --escape-method 2: the solves of the block handle run the block eigen-solver of the escape on
block storage (0: Lanczos); the solve row carries eig_seconds, the escape's steps and calls and the trustregions() seconds beside
the total.  One JSON line.
Usage: python tools/time_blockdiag.py [--n N] [--d D] [--p P] [--reps R] [--rounds K] [--solve] [--runs K] [--no-affine] [--escape-method {0,2}]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def affine_formulation(C, d):
    """(At, b, c): one constraint X_kl = 0 per off-diagonal entry k < l of every diagonal block (entries 1/2 at (k, l), (l, k))."""
    N = C.shape[0]
    n = N // d
    ka, la = np.triu_indices(d, 1)
    k = (np.arange(n)[:, None] * d + ka[None]).ravel().astype(np.int64)
    l = (np.arange(n)[:, None] * d + la[None]).ravel().astype(np.int64)
    m = k.size
    rows = np.concatenate([k + l * N, l + k * N])
    cols = np.concatenate([np.arange(m), np.arange(m)])
    At = sp.csc_matrix((np.full(2 * m, 0.5), (rows, cols)), shape=(N * N, m))
    return At, np.zeros(m), C.toarray().ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--degree", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--no-affine", action="store_true")
    ap.add_argument("--escape-method", type=int, choices=(0, 2), default=0)
    a = ap.parse_args()
    from manisdp_matlab_amd import _lib, problems, solvers
    _lib.load()
    d, p = a.d, a.p
    C, R_true, edges = problems.rotation_synchronization(a.n, d, a.degree, a.sigma, 0)
    N = C.shape[0]
    g = np.random.default_rng(1)
    Y = np.empty((a.n, d, p))
    for i in range(a.n):
        Y[i] = np.linalg.qr(g.standard_normal((p, d)))[0].T
    Y = Y.reshape(N, p)
    out = {"n": a.n, "d": d, "N": N, "p": p, "edges": int(edges.shape[0]), "nnz": int(C.nnz), "reps": a.reps, "rounds": a.rounds,
           "date": time.strftime("%Y-%m-%d")}
    handles = {"block": _lib.Handle.onlyunitblockdiag(C, d, pcap=p)}
    aff = None
    if not a.no_affine:
        aff = affine_formulation(C, d)
        handles["affine"] = _lib.Handle.affine(_lib.KIND_UNITDIAG, aff[0], aff[1], aff[2], N, pcap=p)
    try:
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
            out["hessvec_" + k] = {"us": med, "all_us": [float(x) for x in us[k]], "algo_bytes": algo[k][0], "algo_flops": algo[k][1],
                                   "algo_GBps": algo[k][0] / (1e-6 * med) / 1e9, "tcg_path": handles[k].tcg_path()}
        if "affine" in handles:
            out["hessvec_affine_over_block"] = out["hessvec_affine"]["us"] / out["hessvec_block"]["us"]
    finally:
        for h in handles.values():
            h.close()
    if a.solve:
        def solve_block():
            Ys, obj, data = solvers.ManiSDP_onlyunitblockdiag(C, d, {"tol": 1e-8, "escape_method": a.escape_method, "escape_stats": True}, verbose=False)
            return obj, data, Ys

        def solve_affine():
            Ys, obj, data = solvers.ManiSDP_unitdiag(aff[0], aff[1], aff[2], {"s": N}, {"tol": 1e-8}, verbose=False)
            return obj, data, Ys

        solves = {"block": solve_block}
        if aff is not None:
            solves["affine"] = solve_affine
        ts = {k: [] for k in solves}
        last = {}
        for rep in range(a.runs + 1):                    # one warm-up solve each, then alternate
            for k, fn in solves.items():
                t0 = time.perf_counter()
                last[k] = fn()
                if rep:
                    ts[k].append(time.perf_counter() - t0)
        for k in solves:
            obj, data, Ys = last[k]
            out["solve_" + k] = {"seconds": float(np.median(ts[k])), "all_seconds": [float(t) for t in ts[k]], "obj": float(obj),
                                 "dinf": float(data["dinf"]), "status": int(data["status"]), "p": int(Ys.shape[1]),
                                 "iters": int(data["iters"]), "hessvecs": int(data["hessvecs"]),
                                 "rtr_seconds": float(data["rtr_seconds"]), "eig_seconds": float(data["eig_seconds"]),
                                 "eig_calls": int(data.get("eig_calls", 0)), "eig_steps": int(data.get("eig_steps", 0)),
                                 "eig_verify_steps": int(data.get("eig_verify_steps", 0)), "escape_method_ran": int(data.get("escape_method", -1))}
        Rr = problems.round_rotations(last["block"][2], d)
        out["solve_block"]["rotation_error"] = problems.rotation_error(Rr, R_true)
        if "affine" in solves:
            out["solve_affine_over_block"] = out["solve_affine"]["seconds"] / out["solve_block"]["seconds"]
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
