"""MaxCut of a Gset graph: the SDP bound of examples/example_maxcut.py (C = -L/4, options.p0 = 40, tol = 1e-8), then a cut --
Goemans-Williamson hyperplane rounding of the solution with 1-opt local search, on the device (options["round"]):
argv = [graph name, default G81; trials, default 256]; --order index|color anywhere among them: the order in which a sweep
of the local search visits the rows (default index; color: by colour class, one launch per colour over the whole device)."""
import sys
import time

import numpy as np

from _common import GOLDEN
from manisdp_matlab_amd import problems, solvers

argv = list(sys.argv)
order = "index"
if "--order" in argv:
    k = argv.index("--order")
    order = argv[k + 1]
    del argv[k:k + 2]
name = argv[1] if len(argv) > 1 else "G81"
trials = int(argv[2]) if len(argv) > 2 else 256
C = problems.maxcut_cost_matrix("%s/%s.txt.gz" % (GOLDEN, name))
t = time.time()
Y, fval, data = solvers.ManiSDP_onlyunitdiag(C, {"p0": 40, "tol": 1e-8, "round": {"trials": trials, "sweeps": 50, "seed": 0, "order": order}})
r = data["round"]
x = r["x"].astype(np.float64)
cut = -float(x @ (C @ x))                                  # -x'Cx = x'Lx/4: the weight of the cut (S, V \ S), S = {i: x_i = +1}
print("ManiSDP: bound = %.8f, time = %.2fs (rank %d)" % (-fval, time.time() - t, Y.shape[1]))
print("rounding (%s order): best of %d trials cuts %.1f, cut / bound = %.4f, sweeps per word of 64 trials %s"
      % (order, trials, cut, cut / -fval, r["info"][0].tolist()))
