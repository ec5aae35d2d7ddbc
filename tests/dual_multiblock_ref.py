"""NumPy restatement of the reference's multiblock dual solver src/dual/ManiDSDP_multiblock.m (closures :204-296, driver
:8-202), on the oracle's trust-region method (oracle.manopt_rtr.trustregions) and product manifold
(oracle.manisdp_ref.MultiBlockManifold: the first ``nob`` blocks oblique, the others Euclidean).  A helper of the tests of the
multiblock dual kind, not a conftest.  Factors are lists of (n_i, p_i) arrays (the bytes of MATLAB's p_i x n_i Y{i}).

Where the reference cannot be followed literally ("ManiDSDP_multiblock"):
  * [L] line_search :220-241 stacks rows ([nY{i}; alpha*U{i}] on an empty cell, then [Y{i}; alpha*U{i}]); here, as in the
    two sibling solvers (ManiDSDP_unitdiag.m:160-172, ManiDSDP.m:150-160), the trial point is Y_i + alpha*U_i with the rows of
    the first nob blocks renormalised, and U_i = 0 for the blocks below min_facsize;
  * [F] f (:255, co :216) and obj (:109) are set only when nf != 0: with nf = 0 the Af terms are dropped;
  * [O] obj uses <c, x + bA> (ManiDSDP_unitdiag.m:87, ManiDSDP.m:77) instead of c'*x (:109)."""
import math

import numpy as np
import scipy.sparse as sp

from oracle.manisdp_ref import BlockVec, MultiBlockManifold
from oracle.manopt_rtr import trustregions

DEFAULTS = dict(min_facsize=2, ADMM_maxiter=1000, gama=2, sigma0=1e-1, sigma_min=1e-2, sigma_max=1e7, tol=1e-8, theta=1e-2,
                delta=8, alpha=0.2, tolgradnorm=1e-8, TR_maxinner=20, TR_maxiter=4, tau1=1e1, tau2=1e1,
                line_search=1)                                   # ManiDSDP_multiblock.m:12-28 (+ p0 = ones, :13)


class DualMultiblockProblem:
    """costgrad / hess / co of ManiDSDP_multiblock.m.  ``A`` is the m x sum(n_i^2) PSD part, ``B`` the m x nf free part."""

    def __init__(self, A, B, b, c, cf, dAAt, nset, nob):
        self.A = sp.csr_matrix(A)
        self.At = self.A.T.tocsr()
        self.B = sp.csr_matrix(B) if B is not None else sp.csr_matrix((self.A.shape[0], 0))
        self.nf = self.B.shape[1]
        self.iAt = sp.diags(1.0 / np.asarray(dAAt, dtype=np.float64)) @ self.A     # iA' = D\A   (:45)
        self.bA = self.iAt.T @ b                                                # :47
        self.iAB = sp.csr_matrix(self.iAt.T @ self.B)                          # :48
        self.b, self.c = np.asarray(b, float), np.asarray(c, float)
        self.cf = np.asarray(cf, float) if cf is not None else np.zeros(0)
        self.nset, self.nob = list(nset), int(nob)
        self.nb = len(self.nset)
        self.off = np.concatenate([[0], np.cumsum([n * n for n in self.nset])]).astype(int)
        self.x = np.zeros(int(self.off[-1]))                                    # :58
        self.w = np.zeros(self.nf)                                              # :61
        self.sigma = 1.0
        self.M = None
        self.X = None
        self.eG = None
        self.nhess = 0

    def set_widths(self, p):
        self.M = MultiBlockManifold(p, self.nset, self.nob)                     # :80

    def _s(self, Y):
        return np.concatenate([(yi @ yi.T).ravel(order="F") for yi in Y.b])   # :244-249

    def state(self, Y):
        sc = self._s(Y) - self.c                                                # :250
        y = self.iAt @ sc                                                       # :251
        As = self.At @ y - sc - self.x / self.sigma                             # :252
        f = float(self.b @ y) + 0.5 * self.sigma * float(As @ As)               # :255 [F]
        Af = None
        if self.nf:
            Af = self.B.T @ y - self.cf - self.w / self.sigma                   # :254
            f += 0.5 * self.sigma * float(Af @ Af)
        if self.nob == self.nb:
            tt = self.bA - self.sigma * As                                      # :258
        else:
            inner = self.At @ (self.iAt @ As) - As
            if self.nf:
                inner = inner + self.iAB @ Af                                   # [F]
            tt = self.bA + self.sigma * inner                                   # :260
        return f, tt, y, As, Af

    def co(self, Y):                                                            # :204-218
        return self.state(Y)[0]

    def cost(self, Y):
        return self.state(Y)[0]

    def grad(self, Y):
        _, tt, _, _, _ = self.state(Y)
        self.X, self.eG, G = [], [], []
        for i, (yi, n) in enumerate(zip(Y.b, self.nset)):
            Xi = tt[self.off[i]:self.off[i + 1]].reshape((n, n), order="F")    # :264
            Gi = 2.0 * (Xi.T @ yi)                                              # :265  G{i} = 2*Y{i}*X{i}
            eGi = None
            if i < self.nob:
                eGi = np.sum(yi * Gi, axis=1, keepdims=True)                    # store.eG{i} (:267) enters only as sum(Y.*eG)
                Gi = Gi - yi * eGi                                              # :268
            self.X.append(Xi); self.eG.append(eGi); G.append(Gi)
        return BlockVec(G)

    def hess(self, Y, U):
        self.nhess += 1
        YU = np.concatenate([(ui @ yi.T).ravel(order="F") for yi, ui in zip(Y.b, U.b)])   # :277-278 T = U{i}'*Y{i}
        a = self.iAt @ YU
        if self.nob == self.nb:
            tYU = -2.0 * (self.At @ a)                                          # :283
        else:
            yAU = self.At @ a                                                   # :285
            tYU = -4.0 * yAU + 2.0 * (self.At @ (self.iAt @ yAU))               # :286
            if self.nf:
                tYU = tYU + 2.0 * (self.iAB @ (self.B.T @ a))
        H = []
        for i, (yi, ui, n) in enumerate(zip(Y.b, U.b, self.nset)):
            T = ui @ yi.T
            Hi = 2.0 * (self.X[i].T @ ui) + 2.0 * self.sigma * ((T + T.T) @ yi)          # :280
            Ri = tYU[self.off[i]:self.off[i + 1]].reshape((n, n), order="F")
            Hi = Hi + 2.0 * self.sigma * (Ri.T @ yi)                                     # :290
            if i < self.nob:
                Hi = Hi - yi * np.sum(yi * Hi, axis=1, keepdims=True) - ui * self.eG[i]    # :292
            H.append(Hi)
        return BlockVec(H)

    def outer(self, Y):
        """:86-124 at Y: returns (by, <c, x + bA>, |As|^2, Af, z, X blocks) and updates x, w."""
        S = [yi @ yi.T for yi in Y.b]                                           # :87-91
        sc = np.concatenate([Si.ravel(order="F") for Si in S]) - self.c         # :92
        y = self.iAt @ sc                                                       # :93
        As = self.At @ y - sc                                                   # :94
        Af = self.B.T @ y - self.cf if self.nf else np.zeros(0)                 # :97
        by = float(self.b @ y)                                                  # :101
        sig = self.sigma
        if self.nob == self.nb:
            self.x = self.x - sig * As                                          # :103
        else:
            inner = self.At @ (self.iAt @ (As - self.x / sig)) - As
            if self.nf:
                inner = inner + self.iAB @ (Af - self.w / sig)
            self.x = self.x + sig * inner                                       # :105
        if self.nf:
            self.w = self.w - sig * Af                                          # :108
        ex = self.x + self.bA
        cex = float(self.c @ ex)                                                # [O]
        X, z = [], []
        for i, n in enumerate(self.nset):
            Xi = ex[self.off[i]:self.off[i + 1]].reshape((n, n), order="F")    # :114
            if i < self.nob:
                zi = np.sum(S[i] * Xi, axis=0)                                  # :116
                z.append(zi)
                Xi = Xi - np.diag(zi)                                           # :118
            X.append(Xi)
        z = np.concatenate(z) if z else np.zeros(0)
        return by, cex, float(As @ As), Af, z, X, y


def line_search(prob, Y, U):                                                    # :220-241 [L]
    def trial(alpha):
        out = []
        for i, (yi, ui) in enumerate(zip(Y.b, U.b)):
            t = yi + alpha * ui
            out.append(t / np.sqrt(np.sum(t * t, axis=1, keepdims=True)) if i < prob.nob else t)
        return BlockVec(out)
    alpha = 1.0
    cost0 = prob.co(Y)
    nY = trial(alpha)
    k = 1
    while k <= 15 and prob.co(nY) - cost0 > -1e-3:
        alpha = 0.8 * alpha
        nY = trial(alpha)
        k += 1
    return nY


def ManiDSDP_multiblock(A, b, c, K, options=None, rng=None, verbose=False):
    """``[X, obj, data] = ManiDSDP_multiblock(A, b, c, K, options)`` (:8).  ``options['Y0']`` (list of (n_i, p_i)) replaces
    trustregions' M.rand() start."""
    o = dict(DEFAULTS)
    o.update(options or {})
    nset = [int(v) for v in np.atleast_1d(K["s"])]
    nb = len(nset)
    nob = int(K.get("nob", 0))
    nf = int(K.get("f", 0))
    b = np.asarray(b, dtype=np.float64).ravel()
    call = np.asarray(c, dtype=np.float64).ravel()
    rng = rng or np.random.default_rng(0)
    normc = 1.0 + np.linalg.norm(call)                                         # :33
    Ac = sp.csc_matrix(A)
    B = Ac[:, :nf] if nf else None; Apsd = Ac[:, nf:]                          # :34-41
    cf = call[:nf]; cp = call[nf:]
    dAAt = o.get("dAAt")
    if dAAt is None:
        dAAt = np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel()             # :44
    p0 = [int(v) for v in np.atleast_1d(o.get("p0", np.ones(nb, int)))]
    p = [p0[i] if nset[i] >= o["min_facsize"] else nset[i] for i in range(nb)]   # :50-55
    prob = DualMultiblockProblem(Apsd, B, b, cp, cf, dAAt, nset, nob)
    prob.sigma = float(o["sigma0"])
    gama = float(o["gama"])
    Y = o.get("Y0")
    prob.set_widths(p)
    Y = prob.M.rand(rng) if Y is None else BlockVec([np.array(yi, dtype=np.float64) for yi in Y])
    U = None
    data = {"status": 0, "hessvecs": 0, "log": []}
    gap0 = pinf0 = dinf0 = None
    for it in range(1, int(o["ADMM_maxiter"]) + 1):                            # :79
        prob.set_widths(p)                                                     # :80
        if U is not None:
            Y = line_search(prob, Y, U)                                        # :81-83
        Y, _, info = trustregions(prob, Y, int(o["TR_maxiter"]), int(o["TR_maxinner"]), float(o["tolgradnorm"]))   # :84
        data["hessvecs"] += info.hessvecs
        gradnorm = info.gradnorm                                               # :85
        sig = prob.sigma
        by, cex, as2, Af, z, X, y = prob.outer(Y)                              # :86-124
        pinf = (math.sqrt(as2) + (float(np.linalg.norm(Af)) if nf else 0.0)) / normc     # :95-100
        obj = cex + (float(cf @ prob.w) if nf else 0.0) + float(np.sum(z))     # :109, 117 [O] [F]
        dX, vX, dinfs = [], [], []
        for Xi in X:
            w_, v_ = np.linalg.eigh(0.5 * (Xi + Xi.T))                         # :121
            dX.append(w_); vX.append(v_)
            dinfs.append(max(0.0, -w_[0]) / (1.0 + abs(w_[-1])))               # :122
        dinf = max(dinfs)                                                      # :124
        gap = abs(obj - by) / (1.0 + abs(obj) + abs(by))                       # :125
        data["log"].append((obj, gap, pinf, dinf, gradnorm, max(p), sig))
        if verbose:
            print("Iter %d, obj:%0.8f, gap:%0.1e, pinf:%0.1e, dinf:%0.1e, gradnorm:%0.1e, p_max:%d, sigma:%0.3f"
                  % (it, obj, gap, pinf, dinf, gradnorm, max(p), sig))
        eta = max(gap, pinf, dinf)                                             # :128
        data["iters"] = it
        if eta < o["tol"]:
            break
        if it % 50 == 0:                                                       # :133-143
            if it > 100 and gap > gap0 and pinf > pinf0 and dinf > dinf0:
                data["status"] = 2
                break
            gap0, pinf0, dinf0 = gap, pinf, dinf
        newY, newU = [], []
        for i, n in enumerate(nset):                                           # :144-181
            yi = Y.b[i]
            ui = None
            if n >= o["min_facsize"]:
                V, e, _ = np.linalg.svd(yi, full_matrices=False)               # :146-151
                r = max(int(np.sum(e > o["theta"] * e[0])), 1)                 # :152-155
                if r < p[i]:
                    yi = V[:, :r] * e[:r]                                      # :156-159
                    p[i] = r
                nneg = int(np.sum(dX[i] < 0))
                nne = max(min(nneg, int(o["delta"])), 1) if i < nob else min(nneg, int(o["delta"]))   # :160-164
                if p[i] + nne > n:
                    nne = 0                                                    # :165-167
                if o["line_search"] == 1:
                    ui = np.hstack([np.zeros((n, p[i])), vX[i][:, :nne]])      # :169
                p[i] = p[i] + nne                                              # :171
                if o["line_search"] == 1:
                    yi = np.hstack([yi, np.zeros((n, nne))])                   # :173
                else:
                    yi = np.hstack([yi, o["alpha"] * vX[i][:, :nne]])          # :175
                    if i < nob:
                        yi = yi / np.sqrt(np.sum(yi * yi, axis=1, keepdims=True))   # :176-178
            newY.append(yi)
            newU.append(ui if ui is not None else np.zeros_like(yi))           # [L] U_i = 0 below min_facsize
        Y = BlockVec(newY)
        U = BlockVec(newU) if o["line_search"] == 1 else None
        if pinf < o["tau1"] * gradnorm:                                        # :182-186
            prob.sigma = max(sig / gama, float(o["sigma_min"]))
        elif pinf > o["tau2"] * gradnorm:
            prob.sigma = min(sig * gama, float(o["sigma_max"]))
    S = [yi @ yi.T for yi in Y.b]
    data.update({"X": X, "y": y, "S": S, "w": prob.w, "gap": gap, "pinf": pinf, "dinf": dinf, "gradnorm": gradnorm,
                 "Y": Y.b, "p": list(p)})                                      # :188-196
    if data["status"] == 0 and eta > o["tol"]:
        data["status"] = 1
    return X, obj, data
