#!/usr/bin/env python
"""Times the rank cut / escape widening of all blocks of a multiblock factor per outer iteration: the host route of _Blocks.reshape
(get_point, the per-block NumPy loop, _pack_blocks, set_point) against one msdp_block_reshape call, on 1000 x 60, 4000 x 60,
1000 x 200 and 100 x 211 (blocks x order), and the whole ManiSDP_multiblock solve of the stacked MaxCut instance of
tests/test_gpu_multiblock.py at 1000 x 60 and 4000 x 60 under block_reshape = "host" and "device" (total, rtr_seconds, eig_seconds).

Every measurement runs in a child process of its own under a time limit; three warm-up repetitions, then the median of seven.
Usage: python tools/time_block_reshape.py [--only reshape|solve] [--limit SECONDS]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(1000, 60), (4000, 60), (1000, 200), (100, 211)]
SOLVES = [(1000, 60), (4000, 60)]


def _instance(nblk, n, seed=0):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    C0 = rng.standard_normal((n, n)); C0 = (C0 + C0.T) / 2; np.fill_diagonal(C0, 0.0)
    scale = 1.0 + (np.arange(nblk) % 2)
    c = np.concatenate([(s * C0).reshape(-1) for s in scale])
    At = sp.csc_matrix(([1.0], ([0], [0])), shape=(nblk * n * n, 1))
    return At, np.array([1.0]), c


def child_reshape(nblk, n):
    """A state as an outer iteration meets it: unit-row factors of width 12 whose last 4 columns are 1e-7 small (cut to 8), eigen-data
    with 3 negative eigenvalues per block (widened to 11)."""
    from manisdp_matlab_amd import _lib, solvers
    At, b, c = _instance(nblk, n)
    nset, p0, delta = [n] * nblk, 12, 8
    rng = np.random.default_rng(1)
    N = nblk * n
    Y = rng.standard_normal((N, p0)); Y[:, 8:] *= 1e-7
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    w = np.tile(np.sort(np.concatenate([-rng.random(3), rng.random(n - 3)])), nblk)
    V = np.vstack([np.linalg.qr(rng.standard_normal((n, delta)))[0] for _ in range(min(nblk, 50))])
    V = np.tile(V, (nblk // min(nblk, 50) + 1, 1))[:N]
    h = _lib.Handle.multiblock(At, b, c, nset, nblk, pcap=32)
    o = dict(solvers.DEFAULTS["multiblock"])
    geo = solvers._Blocks(h, o, nset, nblk, strict_rank=False)
    r0, p = geo.r0, [p0] * nblk
    esc = ([w[r0[i]:r0[i + 1]] for i in range(nblk)], [V[r0[i]:r0[i + 1]] for i in range(nblk)])

    def host():
        Yb = geo.download(p)
        newY, _, newp = geo.reshape(Yb, p, None, esc)
        h.set_point(geo.pack(newY, newp))
        return newp

    def device():
        return h.block_reshape(r0[:-1], nset, p, w, V, o["theta"], 0, delta, o["alpha"], o["min_facsize"], 0)[0]

    out = {}
    for name, fn in (("host", host), ("device", device)):
        times = []
        for rep in range(10):
            h.set_point(Y)
            t0 = time.perf_counter()
            newp = fn()
            times.append(time.perf_counter() - t0)
        out[name + "_ms"] = 1e3 * float(np.median(times[3:]))
        out[name + "_p"] = [int(min(newp)), int(max(newp))]
    h.close()
    return out


def child_solve(nblk, n, mode):
    from manisdp_matlab_amd import solvers
    At, b, c = _instance(nblk, n)
    opts = dict(tol=1e-7, p0=[4] * nblk, AL_maxiter=60, block_reshape=mode)
    runs = []
    for rep in range(3):                                             # the first run warms the library up
        t0 = time.perf_counter()
        _, obj, d = solvers.ManiSDP_multiblock(At, b, c, dict(s=[n] * nblk, nob=nblk), dict(opts), verbose=False)
        runs.append(dict(total_s=time.perf_counter() - t0, rtr_s=d["rtr_seconds"], eig_s=d["eig_seconds"], iters=d["iters"], obj=obj,
                         status=d["status"]))
    return sorted(runs[1:], key=lambda r: r["total_s"])[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["reshape", "solve"])
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        kind, nblk, n = a.child[0], int(a.child[1]), int(a.child[2])
        res = child_reshape(nblk, n) if kind == "reshape" else child_solve(nblk, n, a.child[3])
        print("RESULT " + json.dumps(dict(kind=kind, blocks=nblk, order=n, mode=(a.child[3] if kind == "solve" else None), **res)), flush=True)
        return 0
    jobs = []
    if a.only != "solve":
        jobs += [["reshape", str(nb), str(n)] for nb, n in SHAPES]
    if a.only != "reshape":
        jobs += [["solve", str(nb), str(n), m] for nb, n in SOLVES for m in ("host", "device")]
    for job in jobs:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + job, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{job}: no result within {a.limit:.0f} s", flush=True)
            return 1
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:                           # stop at the first failure: nothing more is started on the device
            print(f"{job}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return 1
        print(lines[-1][7:], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
