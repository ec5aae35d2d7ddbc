"""Rotation synchronisation: recover R_1 .. R_n in SO(d) from noisy relative rotations R_i R_j' on a connected random graph
(problems.rotation_synchronization).  The relaxation  min <C, X>  s.t. X PSD of order n d, X_[ii] = I_d  is the
unit-block-diagonal SDP: ManiSDP_onlyunitblockdiag runs it on the stacked Stiefel manifold of the factor (no multipliers, no
penalty).  The rotations are then rounded on the host (problems.round_rotations) and compared with the planted ones up to the
global rotation the problem cannot see (problems.rotation_error).
argv = [n, default 2000; d, default 3; degree, default 8; sigma, default 0.5; seed, default 0]; --persist anywhere on the line: the tCG of every trust-region iteration as one
persistent launch where the handle is eligible (options["block_persist"]); --device-factor anywhere on the line: the factor stays on
the device between the trustregions() calls and the rotations are rounded there too (options["block_factor"] = "device",
options["round_blocks"]: data["R"], which the printed error is then taken from); --block-escape anywhere on the line: the device
escape and its cold check run the block eigen-solver on block storage instead of Lanczos (options["escape_method"] = 2; the
device escape serves orders n d above 600, data["escape_method"] says what ran)."""
import sys
import time

import numpy as np

import _common  # noqa: F401  (puts the repository root on sys.path)
from manisdp_matlab_amd import problems, solvers

persist = "--persist" in sys.argv
device_factor = "--device-factor" in sys.argv
block_escape = "--block-escape" in sys.argv
sys.argv = [a for a in sys.argv if a not in ("--persist", "--device-factor", "--block-escape")]

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 3
degree = int(sys.argv[3]) if len(sys.argv) > 3 else 8
sigma = float(sys.argv[4]) if len(sys.argv) > 4 else 0.5
C, R_true, edges = problems.rotation_synchronization(n, d, degree, sigma, int(sys.argv[5]) if len(sys.argv) > 5 else 0)
t = time.time()
Y, fval, data = solvers.ManiSDP_onlyunitblockdiag(C, d, {"tol": 1e-8, "block_persist": persist, "block_factor": "device" if device_factor else "host",
                                                       "round_blocks": device_factor, **({"escape_method": 2} if block_escape else {})})
e = np.sqrt(np.maximum(np.linalg.eigvalsh(Y.T @ Y), 0.0))
rank = int(np.sum(e >= 1e-3 * e.max()))
R = data["R"] if "R" in data else problems.round_rotations(Y, d)
print("ManiSDP: optimum = %.8f, dinf = %.1e, time = %.2fs (rank %d, factor width %d, %d edges, noise-free value %d)"
      % (fval, data["dinf"], time.time() - t, rank, Y.shape[1], len(edges), -2 * len(edges) * d))
print("rounded rotations: alignment error max_i |R_i Q - R_true_i|_F = %.3e" % problems.rotation_error(R, R_true))
