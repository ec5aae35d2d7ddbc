"""NumPy restatement of the unit-block-diagonal problem  min <C, X>  s.t. X PSD of order N = n d, X_[ii] = I_d  on the stacked
Stiefel manifold of its factor (msdp_create_onlyunitblockdiag_csc, Handle.onlyunitblockdiag; manopt's
stiefelstackedfactory(n, d, p)): the manifold, cost / gradient / Hess-vec / multiplier blocks in the project's scaling
(f = <C, Y Y'> / 2, as _OnlyUnitDiagProblem of the oracle), a problem object that oracle.manopt_rtr.trustregions accepts, the
solver loop, the affine formulation of the same SDP for oracle.manisdp_ref.ManiSDP_unitdiag, and the instances of
tests/test_gpu_blockdiag.py.

Blocks are d consecutive rows of the (N, p) factor; sym(M) = (M + M') / 2."""
import math

import numpy as np
import scipy.sparse as sp


def to3(Y, d):
    return np.ascontiguousarray(Y).reshape(Y.shape[0] // d, d, Y.shape[1])


def sym(M):
    return 0.5 * (M + np.swapaxes(M, -1, -2))


def symbdiag(A, B, d):
    """sym(A_i B_i') of every block: (n, d, d)  (stiefelstackedfactory.m:73-76)."""
    return sym(to3(A, d) @ np.swapaxes(to3(B, d), 1, 2))


def blockmul(L, Y, d):
    """blockdiag(L) Y."""
    return (L @ to3(Y, d)).reshape(Y.shape)


def blockdiag(L):
    return sp.block_diag(list(L), format="csr")


class Op:
    """The cost matrix as an operator: Op(C) @ Y (a hook for other storages, as hermitian_ref.Op)."""

    def __init__(self, C):
        self.C = sp.csr_matrix(C)
        self.shape = self.C.shape

    def __matmul__(self, Y):
        return self.C @ Y


class StiefelStacked:
    """stiefelstackedfactory(n, d, p) on (n d, p) arrays."""

    def __init__(self, n, d, p):
        self.n, self.d, self.p = n, d, p

    def dim(self):
        return self.n * (self.p * self.d - 0.5 * self.d * (self.d + 1))            # :43

    def inner(self, x, a, b):
        return float(np.sum(a * b))                                                # :47

    def norm(self, x, a):
        return float(np.linalg.norm(a))                                            # :49

    def typicaldist(self):
        return math.sqrt(self.dim())                                               # :53

    def proj(self, Y, Z):
        return Z - blockmul(symbdiag(Z, Y, self.d), Y, self.d)                     # :81-87

    tangent = proj

    def retr(self, Y, U):
        u, _, vt = np.linalg.svd(to3(Y + U, self.d), full_matrices=False)          # :103-117
        return (u @ vt).reshape(Y.shape)

    def zerovec(self, x):
        return np.zeros((self.n * self.d, self.p))

    def rand(self, rng):
        return random_point(self.n, self.d, self.p, rng)                           # :142-150


def random_point(n, d, p, rng):
    """The Q factors of randn(p, d), transposed, block by block."""
    Y = np.empty((n, d, p))
    for i in range(n):
        Y[i] = np.linalg.qr(rng.standard_normal((p, d)))[0].T
    return Y.reshape(n * d, p)


def polar_blocks(Y, d):
    """Every block replaced by its polar factor (the nearest matrix with orthonormal rows)."""
    u, _, vt = np.linalg.svd(to3(Y, d), full_matrices=False)
    return np.ascontiguousarray((u @ vt).reshape(Y.shape))


def tangent_direction(Y, d, rng, blocknorm=None):
    """A tangent vector at Y; with blocknorm every block is scaled to that Frobenius norm."""
    M = StiefelStacked(Y.shape[0] // d, d, Y.shape[1])
    U = M.proj(Y, rng.standard_normal(Y.shape))
    if blocknorm is not None:
        U3 = to3(U, d)
        U = (U3 * (blocknorm / np.linalg.norm(U3, axis=(1, 2), keepdims=True))).reshape(Y.shape)
    return U


# ------------------------------------------------------------------ derivatives
def blockmult(C, Y, d):
    return symbdiag(C @ Y, Y, d)


def get_z(C, Y, d):
    return np.ascontiguousarray(np.diagonal(blockmult(C, Y, d), axis1=1, axis2=2)).ravel()


def cost(C, Y, d):
    return 0.5 * float(np.sum((C @ Y) * Y))


def rgrad(C, Y, d):
    CY = C @ Y
    return CY - blockmul(symbdiag(CY, Y, d), Y, d)


def hessvec(C, Y, U, d, project_lambda_term=True):
    """W = C U - blockdiag(Lambda) U, hess_i = W_i - sym(W_i Y_i') Y_i (stiefelstackedfactory.m:93-101).
    project_lambda_term=False leaves Lambda U unprojected (what the oblique kernels may do and this manifold may not)."""
    L = blockmult(C, Y, d)
    CU = C @ U
    if project_lambda_term:
        W = CU - blockmul(L, U, d)
        return W - blockmul(symbdiag(W, Y, d), Y, d)
    return CU - blockmul(symbdiag(CU, Y, d), Y, d) - blockmul(L, U, d)


def slack(C, Y, d):
    """S = C - blockdiag(Lambda)."""
    return sp.csr_matrix(C) - blockdiag(blockmult(C, Y, d))


class Problem:
    """cost / grad / hess with the per-point state (CY, Lambda) of _OnlyUnitDiagProblem(q1="correct")."""

    def __init__(self, C, n, d, p):
        self.C, self.d = C, d
        self.M = StiefelStacked(n, d, p)
        self.CY = self.L = self._bak = None
        self.nhess = 0

    def cost(self, Y):
        self._bak = (self.CY, self.L)
        self.CY = self.C @ Y
        self.L = symbdiag(self.CY, Y, self.d)
        return 0.5 * float(np.sum(np.trace(self.L, axis1=1, axis2=2)))

    def grad(self, Y):
        return self.CY - blockmul(self.L, Y, self.d)

    def hess(self, Y, U):
        self.nhess += 1
        W = self.C @ U - blockmul(self.L, U, self.d)
        return W - blockmul(symbdiag(W, Y, self.d), Y, self.d)

    def on_reject(self):
        self.CY, self.L = self._bak


def trustregions(C, Y0, d, maxiter, maxinner, tolgradnorm):
    from oracle import manopt_rtr
    prob = Problem(C, Y0.shape[0] // d, d, Y0.shape[1])
    return manopt_rtr.trustregions(prob, np.array(Y0, dtype=np.float64), maxiter, maxinner, tolgradnorm)


# ------------------------------------------------------------------ the solver loop
DEFAULTS = dict(AL_maxiter=20, tol=1e-8, theta=1e-1, alpha=0.5, tolgradnorm=1e-8, TR_maxinner=100, TR_maxiter=40)


def solve(C, d, Y0, options=None):
    """The loop of solvers.ManiSDP_onlyunitblockdiag with trustregions() of the oracle and LAPACK's eigh of S: the rank decision
    from Y'Y, the cut Y Q(:, 1:r) only for d <= r <= p - 1, widening [Y, alpha V(:, 1:nne)], the blocks re-orthonormalised by
    their polar factors after either step.  Returns (Y, obj, data)."""
    o = dict(DEFAULTS, delta=d)
    o.update(options or {})
    C = sp.csr_matrix(C)
    Y = np.ascontiguousarray(Y0, dtype=np.float64)
    p = Y.shape[1]
    data = {"status": 0, "widened": 0}
    obj = dinf = r = None
    for it in range(1, o["AL_maxiter"] + 1):
        Y, _, info = trustregions(C, Y, d, o["TR_maxiter"], o["TR_maxinner"], o["tolgradnorm"])
        Y_eval = Y
        L = blockmult(C, Y, d)
        obj = float(np.sum(np.trace(L, axis1=1, axis2=2)))
        dS, vS = np.linalg.eigh((C - blockdiag(L)).toarray())
        dinf = max(0.0, -dS[0]) / (1.0 + dS[-1])
        w, Q = np.linalg.eigh(Y.T @ Y)
        order = np.argsort(w)[::-1]
        e = np.sqrt(np.maximum(w[order], 0.0))
        Q = Q[:, order]
        r = int(np.sum(e >= o["theta"] * e[0]))
        data["iters"] = it
        if dinf < o["tol"]:
            break
        if d <= r <= p - 1:
            Y = polar_blocks(Y @ Q[:, :r], d)
            p = r
        nne = max(min(int(np.sum(dS < 0)), o["delta"]), 1)
        Y = polar_blocks(np.hstack([Y, o["alpha"] * vS[:, :nne]]), d)
        p += nne
        data["widened"] += 1
    Y = Y_eval
    data.update(dinf=dinf, p=Y.shape[1], rank=r, z=get_z(C, Y, d))
    if dinf > o["tol"]:
        data["status"] = 1
    return Y, obj, data


# ------------------------------------------------------------------ the affine formulation
def affine_formulation(C, d):
    """The same SDP for ManiSDP_unitdiag (unit diagonal on the manifold): (At, b, c, K) with one constraint X_kl = 0, b = 0, per
    off-diagonal entry k < l of every diagonal block -- n d (d - 1) / 2 of them, At in the reference's svec-free layout
    (column-major vec of the symmetric constraint matrix, entries 1/2 at (k, l) and (l, k))."""
    C = sp.csr_matrix(C)
    N = C.shape[0]
    n = N // d
    rows, cols, vals = [], [], []
    m = 0
    for i in range(n):
        for a in range(d):
            for b2 in range(a + 1, d):
                k, l = i * d + a, i * d + b2
                rows += [k + l * N, l + k * N]
                cols += [m, m]
                vals += [0.5, 0.5]
                m += 1
    At = sp.csc_matrix((vals, (rows, cols)), shape=(N * N, m))
    b = np.zeros(m)
    c = np.asarray(C.todense()).reshape(-1, order="F")
    K = {"s": N}
    return At, b, c, K


# ------------------------------------------------------------------ instances of the device tests
_CACHE = {}


def instance(n, d, degree, sigma=1.0, diag=False, seed=0):
    """rotation_synchronization(n, d, degree, sigma, seed); diag=True adds symmetric non-zero diagonal blocks."""
    key = (n, d, degree, sigma, diag, seed)
    if key not in _CACHE:
        from manisdp_matlab_amd import problems
        C, R, edges = problems.rotation_synchronization(n, d, degree, sigma, seed)
        if diag:
            g = np.random.default_rng(1000 + seed)
            B = g.standard_normal((n, d, d))
            C = sp.csr_matrix(C + blockdiag(B + np.swapaxes(B, 1, 2)))
            C.sort_indices()
        _CACHE[key] = (C, R, edges)
    return _CACHE[key]


def point(n, d, p, seed=0):
    key = ("pt", n, d, p, seed)
    if key not in _CACHE:
        _CACHE[key] = random_point(n, d, p, np.random.default_rng(77 + seed + 13 * p))
    return _CACHE[key]


# the instance, start and budget of the trustregions() count test: tests/test_blockdiag_ref_host.py shows that the restatement's
# counts on it do not move under 1e-14 perturbations of the start, tests/test_gpu_blockdiag.py holds the device to them
COUNT_CASE = dict(n=67, d=3, degree=6, sigma=1.0, p=5, maxiter=40, maxinner=30, tolgradnorm=1e-7)


def count_case():
    c = COUNT_CASE
    C, _, _ = instance(c["n"], c["d"], c["degree"], c["sigma"])
    return C, point(c["n"], c["d"], c["p"])


def counts(info):
    return (info.iters, info.hessvecs, info.accepted, info.rejected, info.stop_inner[-1] if info.stop_inner else 0)
