"""A quartic on the sphere through the dual approach: the SOS relaxation (qssos) solved with the generic ManiDSDP --
the reference's example/dual/example_qsphere_dual.m:1-21 (b/maxb, theta = 1e-1, tau2 = 0.5).  argv = [d]: without it
d = 10 with the reference's coefficient file qs_c_10_1; with it random coefficients (seed 1)."""
import os
import sys
import time

import numpy as np

from _common import GOLDEN, eta
from manisdp_matlab_amd import problems, solvers

if len(sys.argv) > 1:
    d = int(sys.argv[1])
    coe = np.random.default_rng(1).standard_normal(problems.get_basis(d, 4).shape[1])
else:
    d = 10
    coe = np.loadtxt(os.path.join(GOLDEN, "qs_c_10_1.txt.gz"), delimiter=",").ravel()
A, b, c, K, dAAt = problems.qssos(d, coe)
maxb = float(np.max(np.abs(b)))
t = time.time()
_, fval, data = solvers.ManiDSDP(A, b / maxb, c, K, {"dAAt": dAAt, "tol": 1e-8, "theta": 1e-1, "tau2": 0.5}, verbose=False)
print("ManiDSDP: optimum = %.8f, eta = %.1e, time = %.2fs" % (fval * maxb, eta(data), time.time() - t))
