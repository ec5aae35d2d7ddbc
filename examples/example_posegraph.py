"""Pose-graph optimisation: recover poses (R_i, t_i) in SE(d) from noisy relative poses on a connected random graph
(problems.pose_graph).  The relaxation  min <C, X>  s.t. X PSD of order n (d + 1), (X_[ii])_{1..d,1..d} = I_d  keeps the
positions in the SDP (the non-marginalised form of SE-Sync / Cartan-Sync): ManiSDP_posegraph runs it on stacked Stiefel x
Euclidean, d orthonormal rows and one free row per block of the factor (no multipliers, no penalty, no elimination of the
positions).  The poses are then rounded on the host (problems.round_poses) and compared with the planted ones up to the global
rotation and shift the problem cannot see (problems.pose_error).
argv = [n, default 2000; d, default 3; degree, default 8; sigma_r, default 0.1; sigma_t, default 0.1; seed, default 0]; --persist anywhere on the line: the tCG of every trust-region iteration as one
persistent launch where the handle is eligible (options["block_persist"]); --precon anywhere on the line: block-Jacobi preconditioned tCG
(options["precon"] = "blockjacobi": the diagonal blocks of C; the handle then runs the generic trips); --device-factor anywhere on the
line: the factor stays on the device between the trustregions() calls and the poses are rounded there too
(options["block_factor"] = "device", options["round_blocks"]: data["R"] and data["t"], which the printed errors are then taken from);
--block-escape anywhere on the line: the device escape and its cold check run the block eigen-solver on block storage instead of
Lanczos (options["escape_method"] = 2; the device escape serves orders n (d + 1) above 600, data["escape_method"] says what ran)."""
import sys
import time

import numpy as np

import _common  # noqa: F401  (puts the repository root on sys.path)
from manisdp_matlab_amd import problems, solvers

persist = "--persist" in sys.argv
precon = "--precon" in sys.argv
device_factor = "--device-factor" in sys.argv
block_escape = "--block-escape" in sys.argv
sys.argv = [a for a in sys.argv if a not in ("--persist", "--precon", "--device-factor", "--block-escape")]

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 3
degree = int(sys.argv[3]) if len(sys.argv) > 3 else 8
sigma_r = float(sys.argv[4]) if len(sys.argv) > 4 else 0.1
sigma_t = float(sys.argv[5]) if len(sys.argv) > 5 else 0.1
C, R_true, t_true, edges, _, _ = problems.pose_graph(n, d, degree, sigma_r, sigma_t, int(sys.argv[6]) if len(sys.argv) > 6 else 0)
t = time.time()
Y, fval, data = solvers.ManiSDP_posegraph(C, d, {"tol": 1e-8, "block_persist": persist, "precon": "blockjacobi" if precon else None,
                                               "block_factor": "device" if device_factor else "host", "round_blocks": device_factor,
                                               **({"escape_method": 2} if block_escape else {})})
e = np.sqrt(np.maximum(np.linalg.eigvalsh(Y.T @ Y), 0.0))
rank = int(np.sum(e >= 1e-3 * e.max()))
R, pos = (data["R"], data["t"]) if "R" in data else problems.round_poses(Y, d)
print("ManiSDP: optimum = %.8f, gap = %.1e, dinf = %.1e, time = %.2fs (rank %d, factor width %d, %d edges, %d Hess-vecs)"
      % (fval, data["gap"], data["dinf"], time.time() - t, rank, Y.shape[1], len(edges), data["hessvecs"]))
print("rounded poses: max_i |R_i Q - R_true_i|_F = %.3e, max_i |t_i Q - s - t_true_i| = %.3e"
      % problems.pose_error(R, pos, R_true, t_true))
