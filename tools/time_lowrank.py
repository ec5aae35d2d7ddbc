#!/usr/bin/env python
"""Times the sparse-plus-low-rank cost kind (msdp_create_onlyunitdiag_csc_lowrank) on G81 plus a rank-one term
gamma d d' / (2m) (d the vertex degrees; n = 20 000) at p = 32:
  (a) msdp_bench_hessvec of the low-rank handle, with its algorithmic bytes,
  (b) the same for the plain sparse handle on the generic per-iteration kernels (persist = 0, trip1 = trip2 = 0, window = 0),
  (c) the same for the dense handle of the same matrix -- the only way to pass this problem without the low-rank kind,
  (d) the time of ManiSDP_onlyunitdiag to KKT 1e-8 with the low-rank cost and with the dense one (--solve; median of --runs
      solves after one warm-up solve).
(a) - (b) is the cost of the low-rank term, (c) / (a) what the kind buys.  One JSON line.
Usage: python tools/time_lowrank.py [--reps N] [--runs N] [--solve] [--no-dense] [--graph G81]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(h, Y, reps):
    h.set_point(Y)
    ms, by, fl = h.bench_hessvec(reps)
    return {"us": 1e3 * ms, "algo_bytes": by, "algo_GBps": by / (1e-3 * ms) / 1e9, "algo_flops": fl}


def _solve(solvers, C, runs):
    ts, out = [], None
    for rep in range(runs + 1):
        t0 = time.perf_counter()
        Y, fval, data = solvers.ManiSDP_onlyunitdiag(C, {"tol": 1e-8, "eig": "device"}, verbose=False)
        if rep:
            ts.append(time.perf_counter() - t0)
        out = {"fval": float(fval), "dinf": float(data["dinf"]), "status": int(data["status"]), "p": int(Y.shape[1]),
               "hessvecs": int(data["hessvecs"]), "iters": int(data["iters"])}
    out["seconds"] = float(np.median(ts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--p", type=int, default=32)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--graph", default="G81")
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--no-dense", action="store_true")
    a = ap.parse_args()
    from manisdp_matlab_amd import _lib, problems, solvers
    _lib.load()
    Cs = problems.maxcut_cost_matrix(os.path.join(ROOT, "tests", "golden", a.graph + ".txt.gz")).tocsr()
    n = Cs.shape[0]
    d = np.asarray((Cs != 0).sum(axis=1)).ravel().astype(np.float64) - (Cs.diagonal() != 0)      # vertex degrees
    C = problems.SparsePlusLowRank(Cs, d, [a.gamma / d.sum()])
    Y = np.random.default_rng(0).standard_normal((n, a.p))
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    out = {"graph": a.graph, "n": int(n), "p": a.p, "q": C.q, "reps": a.reps}
    h = _lib.Handle.onlyunitdiag_lowrank(C.Cs, C.V, C.s, pcap=a.p)
    try:
        out["a_lowrank"] = _bench(h, Y, a.reps)
    finally:
        h.close()
    h = _lib.Handle.onlyunitdiag(Cs, pcap=a.p)
    try:
        for name in ("persist", "trip1", "trip2", "window"):
            h.set_option(name, 0)
        out["b_sparse_generic"] = _bench(h, Y, a.reps)
    finally:
        h.close()
    out["lowrank_term_us"] = out["a_lowrank"]["us"] - out["b_sparse_generic"]["us"]
    if not a.no_dense:
        Cd = C.toarray()
        h = _lib.Handle.onlyunitdiag(Cd, pcap=a.p)
        try:
            out["c_dense"] = _bench(h, Y, a.reps)
        finally:
            h.close()
        out["dense_over_lowrank"] = out["c_dense"]["us"] / out["a_lowrank"]["us"]
    if a.solve:
        out["d_solve_lowrank"] = _solve(solvers, C, a.runs)
        if not a.no_dense:
            out["d_solve_dense"] = _solve(solvers, Cd, a.runs)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
