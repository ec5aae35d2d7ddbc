"""Sparse quartic whose clique sub-vectors lie on unit spheres, through the dual approach: the sparse SOS relaxation
(qssos_sparse) solved with ManiDSDP_multiblock, K.nob = 0 -- the reference's example/dual/example_qsphere_dual_sparse.m
(t = 4 cliques of 10 variables: 4 blocks of order 66; gama 2, alpha 0.01, sigma0 1e-2, theta 1e-2, delta 6, line_search 0,
b/maxb).  The coefficients are drawn as in example_qsphere_sparse.py: argv = [t, default 4] [q, default 10]."""
import sys
import time

import numpy as np

from _common import eta
from manisdp_matlab_amd import problems, solvers

t = int(sys.argv[1]) if len(sys.argv) > 1 else 4
q = int(sys.argv[2]) if len(sys.argv) > 2 else 10
cliques, n = problems.chain_cliques(t, q)
coe = np.random.default_rng(1).standard_normal(len(problems.quartic_sparse_monomials(cliques)))
A, b, c, K, dAAt = problems.qssos_sparse(n, cliques, problems.qssos_sparse_coe(cliques, coe))
K["nob"] = 0
maxb = float(np.max(np.abs(b)))
opts = {"dAAt": dAAt, "tol": 1e-8, "gama": 2, "alpha": 0.01, "sigma0": 1e-2, "theta": 1e-2, "delta": 6,
        "line_search": 0}                                   # example_qsphere_dual_sparse.m:24-33
t0 = time.time()
_, fval, data = solvers.ManiDSDP_multiblock(A, b / maxb, c, K, opts, verbose=False)
print("ManiDSDP: optimum = %.8f, eta = %.1e, time = %.2fs (%d variables, %d blocks of order %d, m = %d)"
      % (fval * maxb, eta(data), time.time() - t0, n, t, K["s"][0], b.size))
