"""M-PSK synchronisation: recover symbols z_i in {exp(2 pi i k / M)} from noisy relative phases z_i conj(z_j) + sigma w_ij on a
circulant measurement graph (problems.mpsk_synchronization).  The relaxation  min <C, X>  s.t. X Hermitian PSD, X_ii = 1  gives
a bound and a factor (ManiSDP_onlyunitdiag with a complex C, the factor re-shaped on the device); the factor is then rounded on
the device (msdp_round_phases): to the M-th roots of unity, which answers the problem posed, and to the unit circle (M = 0) for
comparison.  Prints the bound, the two rounded values and the phase errors against the planted symbols.
argv = [n, default 2000; M, default 4; sigma, default 0.5; degree, default 8; seed, default 0]; --order index|color anywhere among
them: the order in which a sweep of the local search visits the rows (default index; color: by colour class, one launch per
colour over the whole device)."""
import sys
import time

import numpy as np

import _common  # noqa: F401  (puts the repository root on sys.path)
from manisdp_matlab_amd import problems, solvers

argv = list(sys.argv)
order = "index"
if "--order" in argv:
    k = argv.index("--order")
    order = argv[k + 1]
    del argv[k:k + 2]
n = int(argv[1]) if len(argv) > 1 else 2000
M = int(argv[2]) if len(argv) > 2 else 4
sigma = float(argv[3]) if len(argv) > 3 else 0.5
degree = int(argv[4]) if len(argv) > 4 else 8
C, z = problems.mpsk_synchronization(n, degree, sigma, M, np.random.default_rng(int(argv[5]) if len(argv) > 5 else 0))
t = time.time()
Y, fval, data = solvers.ManiSDP_onlyunitdiag(C, {"tol": 1e-8, "hermitian_factor": "device",
                                                 "round_phases": {"M": M, "trials": 256, "sweeps": 20, "seed": 0, "order": order}})
print("ManiSDP: bound = %.8f, time = %.2fs (factor width %d)" % (fval, time.time() - t, Y.shape[1]))
rm = data["round"]
t = time.time()
zc, vc, info = solvers.round_phases(C, Y, M=0, trials=256, sweeps=20, rng=np.random.default_rng(0), order=order)
tc = time.time() - t
print("planted symbols:            <C, z z^H> = %.8f" % np.real(np.conj(z) @ (C @ z)))
print("rounded to %2d-PSK:          <C, z z^H> = %.8f, phase error %.3e (%d of %d symbols right)"
      % (M, rm["value"], problems.phase_error(rm["z"], z, M), max(int(np.sum(np.abs(g * rm["z"] - z) < 1e-6))
                                                                  for g in np.exp(2j * np.pi * np.arange(M) / M)), n))
print("rounded to the unit circle: <C, z z^H> = %.8f, phase error %.3e (%.2fs, handle set-up included)"
      % (vc, problems.phase_error(zc, z, 0), tc))
