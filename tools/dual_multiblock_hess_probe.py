"""Hess-vec of the multiblock dual kind (MSDP_KIND_DUAL_MULTIBLOCK) on the sparse BQP SOS relaxation of
example_bqp_dual_sparse.m: t cliques of 20 variables (t blocks of order 211), K.nob = nb, factor width p.
Prints the time per Hess-vec (captured graph of 50, msdp_bench_hessvec) and how many Hess-vecs the run issued; under
`rocprofv3 --kernel-trace --stats -- python tools/dual_multiblock_hess_probe.py T` the kernel calls divided by that count
are the launches per Hess-vec (one cost/grad evaluation adds a handful).  argv = t values (default 10 100), --p P."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from manisdp_matlab_amd import _lib, problems  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
p = int(sys.argv[sys.argv.index("--p") + 1]) if "--p" in sys.argv else 8
if "--p" in sys.argv:
    args.remove(str(p))
ts = [int(a) for a in args] or [10, 100]
REPS = 1000
for t in ts:
    cliques, n = problems.chain_cliques(t, 20)
    coe = np.random.default_rng(1).standard_normal(len(problems.bqp_sparse_monomials(cliques)))
    t0 = time.time()
    A, b, c, K, dAAt = problems.bqpsos_sparse(n, cliques, problems.bqpsos_sparse_coe(cliques, coe))
    tgen = time.time() - t0
    nf = K["f"]
    Apsd = A[:, nf:]
    B = A[:, :nf]
    nb = len(K["s"])
    h = _lib.Handle.dual_multiblock(Apsd, b / np.max(np.abs(b)), c[nf:], dAAt, K["s"], nb, B, c[:nf], pcap=max(32, p))
    h.dual_set_penalty(1.0, np.zeros(nf))
    Y = np.random.default_rng(0).standard_normal((sum(K["s"]), p))
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    h.set_point(Y)
    h.bench_hessvec(50)
    ms, _, _ = h.bench_hessvec(REPS)
    issued = 2 * 3 + 50 + REPS + (0 if os.environ.get("MSDP_NO_GRAPH") else 50)     # msdp_bench_hessvec: 3 warm-up, [a graph of 50,] reps
    print("t = %d (%d blocks of order %d, m = %d, p = %d): Hess-vec %.1f us; %d Hess-vecs issued (generated in %.1fs)"
          % (t, nb, K["s"][0], b.size, p, ms * 1e3, issued, tgen), flush=True)
    h.close()
