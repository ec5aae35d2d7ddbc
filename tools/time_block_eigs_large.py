#!/usr/bin/env python3
"""Times msdp_block_eigs_large (k = 8) against the host loop it replaces (msdp_get_dual_slack_block + numpy.linalg.eigh per block, the
route solvers._Blocks takes with block_eig = "host") on planted rank-deficient blocks, one handle with per-block storage per set:
16 x 277, 4 x 1024, 100 x 300.  Medians of warm calls.

    python tools/time_block_eigs_large.py [--reps 9]
"""
import argparse
import os
import sys
import time

os.environ["MSDP_MULTIBLOCK_BLOCKED"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

import block_eigs_ref as R  # noqa: E402
from manisdp_matlab_amd import _lib  # noqa: E402

SETS = [(16, 277), (4, 1024), (100, 300)]


def median_time(f, reps):
    f(); f()                                                         # warm: workspace allocated, caches and clocks up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    _lib.load()
    print(f"# python tools/time_block_eigs_large.py --reps {a.reps}")
    print(f"# host threads: OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '(unset)')}; times in ms: median (min .. max) of {a.reps} warm calls")
    rng = np.random.default_rng(7)
    for nb, n in SETS:
        mats = [R.dense(np.concatenate([np.zeros(8), R.upper_part(n - 8, rng)]), rng) for _ in range(nb)]
        c = np.concatenate([M.ravel(order="F") for M in mats])
        At = sp.csc_matrix(([1.0], ([0], [0])), shape=(c.size, 1))
        nset = [n] * nb
        h = _lib.Handle.multiblock(At, np.ones(1), c, nset, 0)
        r0 = np.concatenate([[0], np.cumsum(nset)]).astype(np.int64)
        h.set_multipliers(np.zeros(1), 1.0)
        h.set_point(rng.standard_normal((int(r0[-1]), 1)))
        h.cost()
        h.al_dual(np.zeros(1))

        def device():
            return h.block_eigs_large(r0[:-1], nset, 8)

        def host():
            out = []
            for i in range(nb):
                Si = h.get_dual_slack_block(int(r0[i]), n)
                out.append(np.linalg.eigh(0.5 * (Si + Si.T)))
            return out

        w, V = device()
        ref = host()
        err = max(np.abs(w[r0[i]:r0[i + 1]] - ref[i][0]).max() for i in range(nb))
        d, hst = median_time(device, a.reps), median_time(host, a.reps)
        launches, wgs = h.block_eigs_large_info()
        print(f"{nb:4d} x {n:4d}: device {1e3 * d[0]:8.2f} ({1e3 * d[1]:.2f} .. {1e3 * d[2]:.2f})   host loop {1e3 * hst[0]:8.2f} ({1e3 * hst[1]:.2f} .. {1e3 * hst[2]:.2f})"
              f"   host / device {hst[0] / d[0]:5.1f}   launches {launches}, workgroups {wgs}, max |w - w_lapack| {err:.1e}", flush=True)
        h.close()


if __name__ == "__main__":
    main()
