"""Community detection by modularity on a planted two-community graph: the cost -(A - gamma d d'/(2m)) is sparse plus rank one
(problems.modularity, a problems.SparsePlusLowRank -- the dense n x n matrix is never formed on the device); the SDP bound of
ManiSDP_onlyunitdiag, then +1/-1 labels by hyperplane rounding with 1-opt local search on the device (options["round"]):
argv = [n, default 2000; p_in, default 0.02; p_out, default 0.004; seed, default 0]."""
import sys
import time

import numpy as np
import scipy.sparse as sp

import _common  # noqa: F401  (puts the repository root on sys.path)
from manisdp_matlab_amd import problems, solvers

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
p_in = float(sys.argv[2]) if len(sys.argv) > 2 else 0.02
p_out = float(sys.argv[3]) if len(sys.argv) > 3 else 0.004
rng = np.random.default_rng(int(sys.argv[4]) if len(sys.argv) > 4 else 0)
labels = np.where(np.arange(n) < n // 2, 1.0, -1.0)
same = labels[:, None] == labels[None, :]
A = np.triu(rng.random((n, n)) < np.where(same, p_in, p_out), 1).astype(np.float64)
A = sp.csr_matrix(A + A.T)
C = problems.modularity(A)                                  # -(A - d d'/(2m)): minimising <C, X> maximises the modularity
two_m = float(A.sum())
t = time.time()
Y, fval, data = solvers.ManiSDP_onlyunitdiag(C, {"tol": 1e-8, "round": {"trials": 256, "sweeps": 50, "seed": 0}})
x = data["round"]["x"].astype(np.float64)
Q = -float(x @ C.matvec(x)) / (2.0 * two_m)                 # x' B x / (4m)
print("ManiSDP: modularity bound = %.6f, time = %.2fs (rank %d)" % (-fval / (2.0 * two_m), time.time() - t, Y.shape[1]))
print("rounding: modularity of the labels = %.6f (planted partition: %.6f)" % (Q, -float(labels @ C.matvec(labels)) / (2.0 * two_m)))
print("labels recovered (up to sign): %.4f" % max(np.mean(x == labels), np.mean(x == -labels)))
