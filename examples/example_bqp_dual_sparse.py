"""Sparse BQP (chain of cliques) through the dual approach: the sparse SOS relaxation (bqpsos_sparse) solved with
ManiDSDP_multiblock, every block unit-diagonal (K.nob = nb) -- the reference's example/dual/example_bqp_dual_sparse.m
(t = 10 cliques of q = 20 variables: 10 blocks of order 211, b/maxb).  The coefficients are drawn as in
example_bqp_sparse.py, so both scripts print the same optimum for the same t, q: argv = [t, default 10] [q, default 20]."""
import sys
import time

import numpy as np

from _common import eta
from manisdp_matlab_amd import problems, solvers

t = int(sys.argv[1]) if len(sys.argv) > 1 else 10
q = int(sys.argv[2]) if len(sys.argv) > 2 else 20
cliques, n = problems.chain_cliques(t, q)
coe = np.random.default_rng(1).standard_normal(len(problems.bqp_sparse_monomials(cliques)))
t0 = time.time()
A, b, c, K, dAAt = problems.bqpsos_sparse(n, cliques, problems.bqpsos_sparse_coe(cliques, coe))
K["nob"] = len(K["s"])
tgen = time.time() - t0
maxb = float(np.max(np.abs(b)))
t0 = time.time()
_, fval, data = solvers.ManiDSDP_multiblock(A, b / maxb, c, K, {"dAAt": dAAt, "tol": 1e-8}, verbose=False)
print("ManiDSDP: optimum = %.8f, eta = %.1e, time = %.2fs (%d variables, %d blocks of order %d, m = %d; generated in %.1fs)"
      % (fval * maxb, eta(data), time.time() - t0, n, t, K["s"][0], b.size, tgen))
