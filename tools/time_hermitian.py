#!/usr/bin/env python
"""Times the Hermitian cost kind (msdp_create_onlyunitdiag_csc_hermitian) against the only other way to pass the complex
problem, the real embedding C~ = [[A, -B], [B, A]] of order 2n, on problems.phase_synchronization(20 000, 8, 1.0) at complex
width p = 16:
  (a) msdp_bench_hessvec of the Hermitian handle (order n, real width 2p),
  (b) the same for the plain sparse handle of C~ (order 2n, real width 2p: the factor the embedding needs for the same X),
  (c) with --solve: ManiSDP_onlyunitdiag with the defaults on both forms (median of --runs solves after one warm-up solve).
Both Hess-vecs run the stand-alone row kernels of msdp_launch_hess; tcg_path / persist_form tell which path the handle's
trustregions() calls take (the embedded handle may take the persistent one, the Hermitian one cannot).  One JSON line.
--escape-method 2: the solves of the Hermitian form run the block eigen-solver of the escape on a complex panel (0: Lanczos).
Usage: python tools/time_hermitian.py [--reps N] [--runs N] [--solve] [--n N] [--p P] [--escape-method {0,2}]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench(h, Y, reps):
    h.set_point(Y)
    h.bench_hessvec(reps)                                # warm-up: clocks, caches, the graph instantiation
    ms, by, fl = h.bench_hessvec(reps)
    return {"us": 1e3 * ms, "algo_bytes": by, "algo_GBps": by / (1e-3 * ms) / 1e9, "algo_flops": fl,
            "tcg_path": h.tcg_path(), "persist_form": h.persist_form()}


def _solve(solvers, C, runs, extra=None):
    ts, out = [], None
    for rep in range(runs + 1):
        t0 = time.perf_counter()
        Y, fval, data = solvers.ManiSDP_onlyunitdiag(C, dict({"tol": 1e-8}, **(extra or {})), verbose=False)
        if rep:
            ts.append(time.perf_counter() - t0)
        out = {"fval": float(fval), "dinf": float(data["dinf"]), "status": int(data["status"]), "p": int(Y.shape[1]),
               "hessvecs": int(data["hessvecs"]), "iters": int(data["iters"]), "rtr_seconds": float(data["rtr_seconds"]),
               "eig_seconds": float(data["eig_seconds"]), "escape_method_ran": int(data.get("escape_method", -1))}
    out["seconds"] = float(np.median(ts))
    out["all_seconds"] = [float(t) for t in ts]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--p", type=int, default=16)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--escape-method", type=int, choices=(0, 2), default=0)
    a = ap.parse_args()
    from manisdp_matlab_amd import _lib, problems, solvers
    _lib.load()
    C, _ = problems.phase_synchronization(a.n, 8, a.sigma, np.random.default_rng(0))
    Ce = sp.bmat([[C.real, -C.imag], [C.imag, C.real]], format="csr")
    g = np.random.default_rng(1)
    Y = g.standard_normal((a.n, a.p)) + 1j * g.standard_normal((a.n, a.p))
    Y /= np.sqrt(np.sum(np.abs(Y) ** 2, axis=1, keepdims=True))
    Ye = np.ascontiguousarray(np.block([[Y.real, -Y.imag], [Y.imag, Y.real]]))
    out = {"n": a.n, "p_complex": a.p, "nnz": int(C.nnz), "nnz_embedded": int(Ce.nnz), "reps": a.reps}
    h = _lib.Handle.onlyunitdiag_hermitian(C, pcap=a.p)
    try:
        out["a_hermitian"] = _bench(h, Y, a.reps)
    finally:
        h.close()
    h = _lib.Handle.onlyunitdiag(Ce, pcap=2 * a.p)
    try:
        out["b_embedded"] = _bench(h, Ye, a.reps)
    finally:
        h.close()
    out["embedded_over_hermitian"] = out["b_embedded"]["us"] / out["a_hermitian"]["us"]
    if a.solve:
        out["c_solve_hermitian"] = _solve(solvers, C, a.runs, {"escape_method": a.escape_method})
        out["c_solve_embedded"] = _solve(solvers, Ce, a.runs)
        out["solve_embedded_over_hermitian"] = out["c_solve_embedded"]["seconds"] / out["c_solve_hermitian"]["seconds"]
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
