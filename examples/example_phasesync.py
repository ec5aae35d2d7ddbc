"""Phase (angular) synchronisation: recover unit-modulus z_1 .. z_n from noisy relative phases z_i conj(z_j) + sigma w_ij on a
circulant measurement graph (problems.phase_synchronization).  The relaxation  min <C, X>  s.t. X Hermitian PSD, X_ii = 1  is
the complex unit-diagonal SDP: ManiSDP_onlyunitdiag takes the complex Hermitian C directly (Handle.onlyunitdiag_hermitian --
no real embedding of order 2n).  The phases are then rounded on the host: x_i = u_i / |u_i| with u the leading left singular
vector of Y.  argv = [n, default 2000; degree, default 8; sigma, default 1.0; seed, default 0]; the flag --block-escape, anywhere
on the line, runs the saddle escape with the block eigen-solver on a complex panel (options["escape_method"] = 2) instead of
Lanczos on the real view."""
import sys
import time

import numpy as np

import _common  # noqa: F401  (puts the repository root on sys.path)
from manisdp_matlab_amd import problems, solvers

argv = [s for s in sys.argv[1:] if s != "--block-escape"]
block_escape = "--block-escape" in sys.argv[1:]
n = int(argv[0]) if len(argv) > 0 else 2000
degree = int(argv[1]) if len(argv) > 1 else 8
sigma = float(argv[2]) if len(argv) > 2 else 1.0
C, z = problems.phase_synchronization(n, degree, sigma, np.random.default_rng(int(argv[3]) if len(argv) > 3 else 0))
t = time.time()
Y, fval, data = solvers.ManiSDP_onlyunitdiag(C, dict({"tol": 1e-8}, **({"escape_method": 2} if block_escape else {})))
e = np.sqrt(np.maximum(np.linalg.eigvalsh(Y.conj().T @ Y), 0.0))
rank = int(np.sum(e >= 1e-3 * e.max()))
u = np.linalg.svd(Y, full_matrices=False)[0][:, 0]
x = u / np.maximum(np.abs(u), 1e-300)
print("ManiSDP: optimum = %.8f, time = %.2fs (rank %d, factor width %d)" % (fval, time.time() - t, rank, Y.shape[1]))
print("rounded phases: <C, x x^H> = %.8f (planted z: %.8f)" % (np.real(np.conj(x) @ (C @ x)), np.real(np.conj(z) @ (C @ z))))
print("correlation |<z, x>| / n = %.6f" % (abs(np.vdot(z, x)) / n))
