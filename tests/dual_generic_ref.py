"""NumPy restatement of the reference's generic dual solver src/dual/ManiDSDP.m (closures :141-177, driver :7-139), on the
oracle's trust-region method (oracle.manopt_rtr.trustregions) and Euclidean manifold (oracle.manisdp_ref.EuclidNP).
A helper of the tests of the generic dual kind, not a conftest.

``q1`` selects how the closures share X: ``'reference'`` follows problem.costgrad of the
reference, where every cost evaluation -- a rejected proposal included -- overwrites the X the next hess uses;
``'correct'`` keeps the X of the point the Hessian is taken at (what the device does with its two slots)."""
import numpy as np
import scipy.sparse as sp

from oracle.manisdp_ref import EuclidNP
from oracle.manopt_rtr import trustregions

DEFAULTS = dict(p0=1, ADMM_maxiter=1000, gama=2, sigma0=1e-1, sigma_min=1e-2, sigma_max=1e7, tol=1e-8, theta=1e-2,
                delta=8, alpha=0.01, tolgradnorm=1e-8, TR_maxinner=20, TR_maxiter=4, tau1=0.1, tau2=1,
                line_search=1)                                   # ManiDSDP.m:10-25


class DualGenericProblem:
    """costgrad / hess / co of ManiDSDP.m.  ``A`` is the m x n^2 PSD part, ``B`` the m x nf free part (:32-35)."""

    def __init__(self, A, B, b, c, cf, dAAt, n, p, q1="correct"):
        assert q1 in ("reference", "correct")
        self.A = sp.csr_matrix(A)
        self.At = self.A.T.tocsr()
        self.B = sp.csr_matrix(B)
        self.iAt = sp.diags(1.0 / np.asarray(dAAt, dtype=np.float64)) @ self.A     # iA' = D\A   (:38)
        self.bA = self.iAt.T @ b                                                # :39
        self.iAB = sp.csr_matrix(self.iAt.T @ self.B)                          # :40
        self.b, self.c, self.cf, self.n = np.asarray(b, float), np.asarray(c, float), np.asarray(cf, float), n
        self.M = EuclidNP(n, p)
        self.x = np.zeros(n * n)                                                # :45
        self.w = np.zeros(self.cf.size)                                         # :46
        self.sigma = 1.0
        self.q1 = q1
        self.X = None
        self.nhess = 0

    def set_width(self, p):
        self.M = EuclidNP(self.n, p)

    def _state(self, Y):
        S = Y @ Y.T                                                  # :163
        sc = S.ravel(order="F") - self.c                             # :164
        y = self.iAt @ sc                                            # :165
        As = self.At @ y - sc - self.x / self.sigma                  # :166
        Af = self.B.T @ y - self.cf - self.w / self.sigma            # :167
        f = float(self.b @ y) + 0.5 * self.sigma * (float(As @ As) + float(Af @ Af))     # :168
        X = (self.bA + self.sigma * (self.iAB @ Af + self.At @ (self.iAt @ As) - As)).reshape((self.n, self.n), order="F")   # :169
        return f, X

    def co(self, Y):                                                 # :141-148
        return self._state(Y)[0]

    def cost(self, Y):
        f, X = self._state(Y)
        if self.q1 == "reference":                                   # costgrad: the closure's X follows every evaluation
            self.X = X
        return f

    def grad(self, Y):
        _, self.X = self._state(Y)
        return 2.0 * self.X @ Y                                      # :170

    def hess(self, Y, U):
        self.nhess += 1
        n = self.n
        YU = U @ Y.T                                                 # :174
        a = self.iAt @ YU.ravel(order="F")
        yAU = (self.At @ a).reshape((n, n), order="F")               # :175
        inner = self.At @ (self.iAt @ yAU.ravel(order="F"))
        if self.B.shape[1]:
            inner = inner + self.iAB @ (self.B.T @ a)
        T = inner.reshape((n, n), order="F") - 2.0 * yAU
        return 2.0 * self.X @ U + 2.0 * self.sigma * (U @ (Y.T @ Y) + Y @ (U.T @ Y)) + 4.0 * self.sigma * T @ Y   # :176


def line_search(prob, Y, U):                                         # :150-160
    alpha = 1.0
    cost0 = prob.co(Y)
    i = 1
    nY = Y + alpha * U
    while i <= 15 and prob.co(nY) - cost0 > -1e-3:
        alpha = 0.8 * alpha
        nY = Y + alpha * U
        i += 1
    return nY


def ManiDSDP(A, b, c, K, options=None, rng=None, q1="correct", verbose=False):
    """``[X, obj, data] = ManiDSDP(A, b, c, K, options)`` (:7).  ``options['Y0']`` replaces trustregions' M.rand() start."""
    o = dict(DEFAULTS)
    o.update(options or {})
    n = int(K["s"]); nf = int(K.get("f", 0))
    b = np.asarray(b, dtype=np.float64).ravel()
    call = np.asarray(c, dtype=np.float64).ravel()
    rng = rng or np.random.default_rng(0)
    normc = 1.0 + np.linalg.norm(call)                              # :31
    Ac = sp.csc_matrix(A)
    B = Ac[:, :nf]; Apsd = Ac[:, nf:]                               # :32-33
    cf = call[:nf]; cp = call[nf:]                                  # :34-35
    dAAt = o.get("dAAt")
    if dAAt is None:
        dAAt = np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel()  # :37
    p = int(o["p0"])
    prob = DualGenericProblem(Apsd, B, b, cp, cf, dAAt, n, p, q1=q1)
    prob.sigma = float(o["sigma0"])
    gama = float(o["gama"])
    Y = o.get("Y0")
    Y = rng.standard_normal((n, p)) if Y is None else np.array(Y, dtype=np.float64)
    U = None
    data = {"status": 0, "hessvecs": 0, "log": [], "p_max": p}
    gap0 = pinf0 = dinf0 = None
    for it in range(1, int(o["ADMM_maxiter"]) + 1):                 # :59
        prob.set_width(p)                                           # :60
        if U is not None:
            Y = line_search(prob, Y, U)                             # :61-63
        Y, _, info = trustregions(prob, Y, int(o["TR_maxiter"]), int(o["TR_maxinner"]), float(o["tolgradnorm"]))   # :64
        data["hessvecs"] += info.hessvecs
        gradnorm = info.gradnorm                                    # :65
        S = Y @ Y.T                                                 # :66
        sc = S.ravel(order="F") - cp
        y = prob.iAt @ sc                                           # :68
        As = prob.At @ y - sc                                       # :69
        Af = B.T @ y - cf                                           # :70
        pinf = (np.linalg.norm(As) + np.linalg.norm(Af)) / normc    # :71
        by = float(b @ y)                                           # :72
        sig = prob.sigma
        prob.x = prob.x + sig * (prob.iAB @ (Af - prob.w / sig) + prob.At @ (prob.iAt @ (As - prob.x / sig)) - As)   # :73
        prob.w = prob.w - sig * Af                                  # :74
        X = (prob.x + prob.bA).reshape((n, n), order="F")           # :75
        dX, vX = np.linalg.eigh(0.5 * (X + X.T))                    # :76
        obj = float(cp @ (prob.x + prob.bA) + cf @ prob.w)          # :77
        dinf = max(0.0, -dX[0]) / (1.0 + abs(dX[-1]))               # :78
        gap = abs(obj - by) / (1.0 + abs(obj) + abs(by))            # :79
        V, e, _ = np.linalg.svd(Y, full_matrices=False)             # :80-85
        r = int(np.sum(e > o["theta"] * e[0]))                      # :86
        data["log"].append((obj, gap, pinf, dinf, gradnorm, r, p, sig))
        if verbose:
            print("Iter %d, obj:%0.8f, gap:%0.1e, pinf:%0.1e, dinf:%0.1e, gradnorm:%0.1e, r:%d, p:%d, sigma:%0.3f"
                  % (it, obj, gap, pinf, dinf, gradnorm, r, p, sig))
        eta = max(gap, pinf, dinf)                                  # :89
        data["iters"] = it
        if eta < o["tol"]:
            break
        if it % 20 == 0:                                            # :94-104
            if it > 50 and gap > gap0 and pinf > pinf0 and dinf > dinf0:
                data["status"] = 2
                break
            gap0, pinf0, dinf0 = gap, pinf, dinf
        if r <= p - 1:                                              # :105-108
            Y = V[:, :r] * e[:r]
            p = r
        nne = min(int(np.sum(dX < 0)), int(o["delta"]))             # :109
        if o["line_search"] == 1:
            U = np.hstack([np.zeros((n, p)), vX[:, :nne]])          # :111
        p = p + nne                                                 # :113
        data["p_max"] = max(data["p_max"], p)
        if o["line_search"] == 1:
            Y = np.hstack([Y, np.zeros((n, nne))])                  # :115
        else:
            Y = np.hstack([Y, o["alpha"] * vX[:, :nne]])            # :117
        if pinf < o["tau1"] * gradnorm:                             # :119-123
            prob.sigma = max(sig / gama, float(o["sigma_min"]))
        elif pinf > o["tau2"] * gradnorm:
            prob.sigma = min(sig * gama, float(o["sigma_max"]))
    data.update({"X": X, "y": y, "S": S, "w": prob.w, "gap": gap, "pinf": pinf, "dinf": dinf, "gradnorm": gradnorm,
                 "Y": Y})                                           # :125-133
    if data["status"] == 0 and eta > o["tol"]:
        data["status"] = 1
    return X, obj, data
