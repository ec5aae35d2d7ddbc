"""NumPy restatement of the pose-graph problem  min <C, X>  s.t. X PSD of order N = n (d + 1), (X_[ii])_{1..d,1..d} = I_d  on the
product of the stacked Stiefel manifold and a Euclidean space (msdp_create_posegraph_csc, Handle.posegraph; manopt's
productmanifold of stiefelstackedfactory(n, d, p) and euclideanfactory(n, p)): the manifold, cost / gradient / Hess-vec /
multiplier blocks in the project's scaling (f = <C, Y Y'> / 2), a problem object that oracle.manopt_rtr.trustregions accepts,
the solver loop of solvers.ManiSDP_posegraph, and the instances of tests/test_gpu_posegraph.py.

Block i of the (N, p) factor is the d rows Y_i with Y_i Y_i' = I_d followed by one free row tau_i; sym(M) = (M + M') / 2.
Multiplier blocks are d x d: S = C - blockdiag(Lambda_i (+) 0)."""
import math

import numpy as np
import scipy.sparse as sp


def to3(Y, d):
    """(n, d + 1, p) view of the factor."""
    return np.ascontiguousarray(Y).reshape(Y.shape[0] // (d + 1), d + 1, Y.shape[1])


def rot(Y, d):
    """The rotation rows: (n, d, p)."""
    return to3(Y, d)[:, :d, :]


def free(Y, d):
    """The free rows: (n, p)."""
    return to3(Y, d)[:, d, :]


def sym(M):
    return 0.5 * (M + np.swapaxes(M, -1, -2))


def symbdiag(A, B, d):
    """sym(A_i B_i') of the rotation rows of every block: (n, d, d)."""
    return sym(rot(A, d) @ np.swapaxes(rot(B, d), 1, 2))


def blockmul(L, Y, d):
    """blockdiag(L_i (+) 0) Y: the free rows of the product are zero."""
    out = np.zeros_like(to3(Y, d))
    out[:, :d, :] = L @ rot(Y, d)
    return out.reshape(Y.shape)


def pad(L):
    """L_i (+) 0: (n, d + 1, d + 1)."""
    n, d, _ = L.shape
    out = np.zeros((n, d + 1, d + 1))
    out[:, :d, :d] = L
    return out


def blockdiag(L):
    """blockdiag(L_i (+) 0) of order n (d + 1)."""
    return sp.block_diag(list(pad(L)), format="csr")


class StiefelEuclid:
    """productmanifold of stiefelstackedfactory(n, d, p) and euclideanfactory(n, p) on (n (d + 1), p) arrays, Frobenius metric."""

    def __init__(self, n, d, p):
        self.n, self.d, self.p = n, d, p

    def dim(self):
        return self.n * (self.p * self.d - 0.5 * self.d * (self.d + 1)) + self.n * self.p

    def inner(self, x, a, b):
        return float(np.sum(a * b))

    def norm(self, x, a):
        return float(np.linalg.norm(a))

    def typicaldist(self):
        # productmanifold.m:160-166: the root of the sum of squares of stiefelstackedfactory.m:53 and euclideanfactory.m:57
        return math.sqrt(self.dim())

    def proj(self, Y, Z):
        return Z - blockmul(symbdiag(Z, Y, self.d), Y, self.d)        # Stiefel on the rotation rows, identity on the free row

    tangent = proj

    def retr(self, Y, U):
        A = to3(Y + U, self.d).copy()                                   # the free row: tau + eta
        u, _, vt = np.linalg.svd(A[:, :self.d, :], full_matrices=False)
        A[:, :self.d, :] = u @ vt                                       # polar on the rotation rows
        return A.reshape(Y.shape)

    def zerovec(self, x):
        return np.zeros((self.n * (self.d + 1), self.p))

    def rand(self, rng):
        return random_point(self.n, self.d, self.p, rng)


def random_point(n, d, p, rng, free_scale=1.0):
    """The Q factors of randn(p, d), transposed, in the rotation rows; free_scale * randn in the free rows (the solver's start
    has zeros there: start_point)."""
    Y = np.empty((n, d + 1, p))
    for i in range(n):
        Y[i, :d] = np.linalg.qr(rng.standard_normal((p, d)))[0].T
    Y[:, d, :] = free_scale * rng.standard_normal((n, p))
    return Y.reshape(n * (d + 1), p)


def start_point(n, d, p, rng):
    """The start of solvers.ManiSDP_posegraph: the Q factors of randn(p, d) in the rotation rows, zeros in the free rows."""
    Y = np.zeros((n, d + 1, p))
    for i in range(n):
        Y[i, :d] = np.linalg.qr(rng.standard_normal((p, d)))[0].T
    return Y.reshape(n * (d + 1), p)


def planted_point(R_true, t_true):
    """The factor of width d that holds the planted poses: rotation rows R_i, free row t_i."""
    n, d, _ = R_true.shape
    Y = np.empty((n, d + 1, d))
    Y[:, :d, :] = R_true
    Y[:, d, :] = t_true
    return Y.reshape(n * (d + 1), d)


def polar_blocks(Y, d):
    """The rotation rows of every block replaced by their polar factor; the free rows as they are."""
    A = to3(Y, d).copy()
    u, _, vt = np.linalg.svd(A[:, :d, :], full_matrices=False)
    A[:, :d, :] = u @ vt
    return np.ascontiguousarray(A.reshape(Y.shape))


def tangent_direction(Y, d, rng, blocknorm=None):
    """A tangent vector at Y; with blocknorm every block (rotation and free rows together) is scaled to that Frobenius norm."""
    M = StiefelEuclid(Y.shape[0] // (d + 1), d, Y.shape[1])
    U = M.proj(Y, rng.standard_normal(Y.shape))
    if blocknorm is not None:
        U3 = to3(U, d)
        U = (U3 * (blocknorm / np.linalg.norm(U3, axis=(1, 2), keepdims=True))).reshape(Y.shape)
    return U


# ------------------------------------------------------------------ derivatives
def blockmult(C, Y, d):
    """Lambda_i = sym(G_i Y_i') with (C Y)_i = [G_i; g_i]: (n, d, d)."""
    return symbdiag(C @ Y, Y, d)


def get_z(C, Y, d):
    """The diagonals of Lambda with 0 in the free-row entries: N values, sum = the dual value."""
    L = blockmult(C, Y, d)
    z = np.zeros((L.shape[0], d + 1))
    z[:, :d] = np.diagonal(L, axis1=1, axis2=2)
    return z.ravel()


def cost(C, Y, d):
    return 0.5 * float(np.sum((C @ Y) * Y))


def dual_value(C, Y, d):
    return float(np.sum(np.trace(blockmult(C, Y, d), axis1=1, axis2=2)))


def gap(obj, dual):
    return abs(obj - dual) / (1.0 + abs(obj) + abs(dual))


def rgrad(C, Y, d):
    CY = C @ Y
    return CY - blockmul(symbdiag(CY, Y, d), Y, d)


def hessvec(C, Y, U, d, project_lambda_term=True):
    """W = C U - blockdiag(Lambda (+) 0) U; rotation rows W_i - sym(W_i Y_i') Y_i, free row of W unchanged.
    project_lambda_term=False leaves Lambda U unprojected."""
    L = blockmult(C, Y, d)
    CU = C @ U
    if project_lambda_term:
        W = CU - blockmul(L, U, d)
        return W - blockmul(symbdiag(W, Y, d), Y, d)
    return CU - blockmul(symbdiag(CU, Y, d), Y, d) - blockmul(L, U, d)


def slack(C, Y, d):
    """S = C - blockdiag(Lambda (+) 0)."""
    return sp.csr_matrix(C) - blockdiag(blockmult(C, Y, d))


def residual_cost(Y, d, edges, meas_R, meas_t, kappa=1.0, omega=1.0):
    """sum_ij kappa |Y_i - M_ij Y_j|^2 + omega |tau_j - tau_i - m_ij' Y_i|^2: the definition of problems.pose_graph, directly."""
    Yr, tau = rot(Y, d), free(Y, d)
    i, j = edges[:, 0], edges[:, 1]
    a = Yr[i] - meas_R @ Yr[j]
    b = tau[j] - tau[i] - np.einsum("ma,map->mp", meas_t, Yr[i])
    return kappa * float(np.sum(a * a)) + omega * float(np.sum(b * b))


class Problem:
    """cost / grad / hess with the per-point state (CY, Lambda) of _OnlyUnitDiagProblem(q1="correct")."""

    def __init__(self, C, n, d, p):
        self.C, self.d = C, d
        self.M = StiefelEuclid(n, d, p)
        self.CY = self.L = self._bak = None
        self.nhess = 0

    def cost(self, Y):
        self._bak = (self.CY, self.L)
        self.CY = self.C @ Y
        self.L = symbdiag(self.CY, Y, self.d)
        # <C, X> / 2 = (sum tr Lambda + sum <g_i, tau_i>) / 2
        return 0.5 * (float(np.sum(np.trace(self.L, axis1=1, axis2=2))) + float(np.sum(free(self.CY, self.d) * free(Y, self.d))))

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
    prob = Problem(C, Y0.shape[0] // (d + 1), d, Y0.shape[1])
    return manopt_rtr.trustregions(prob, np.array(Y0, dtype=np.float64), maxiter, maxinner, tolgradnorm)


# ------------------------------------------------------------------ the solver loop
DEFAULTS = dict(AL_maxiter=20, tol=1e-8, theta=1e-1, alpha=0.5, tolgradnorm=1e-8, TR_maxinner=100, TR_maxiter=40)


def solve(C, d, Y0, options=None):
    """The loop of solvers.ManiSDP_posegraph with trustregions() of the oracle and LAPACK's eigh of S.  obj = <C, Y Y'>, the
    dual value is sum tr Lambda; the loop stops when max(dinf, gap) < tol.  With dinf < tol <= gap the point is not stationary
    and trustregions() runs again on the same factor, without a cut or widening; otherwise the rank decision from Y'Y, the cut
    Y Q(:, 1:r) only for d <= r <= p - 1, widening [Y, alpha V(:, 1:nne)], the rotation rows re-orthonormalised by their polar
    factors after either step.  data["log"]: (iteration, obj, dinf, gap, p, Hess-vecs) per outer iteration.
    Returns (Y, obj, data)."""
    o = dict(DEFAULTS, delta=d)
    o.update(options or {})
    C = sp.csr_matrix(C)
    Y = np.ascontiguousarray(Y0, dtype=np.float64)
    p = Y.shape[1]
    data = {"status": 0, "widened": 0, "reruns": 0, "hessvecs": 0, "log": []}
    obj = dinf = gp = r = None
    for it in range(1, o["AL_maxiter"] + 1):
        Y, f, info = trustregions(C, Y, d, o["TR_maxiter"], o["TR_maxinner"], o["tolgradnorm"])
        data["hessvecs"] += info.hessvecs
        Y_eval = Y
        L = blockmult(C, Y, d)
        dual = float(np.sum(np.trace(L, axis1=1, axis2=2)))
        obj = 2.0 * f
        gp = gap(obj, dual)
        dS, vS = np.linalg.eigh((C - blockdiag(L)).toarray())
        dinf = max(0.0, -dS[0]) / (1.0 + dS[-1])
        w, Q = np.linalg.eigh(Y.T @ Y)
        order = np.argsort(w)[::-1]
        e = np.sqrt(np.maximum(w[order], 0.0))
        Q = Q[:, order]
        r = int(np.sum(e >= o["theta"] * e[0]))
        data["iters"] = it
        data["log"].append((it, obj, dinf, gp, p, info.hessvecs))
        if max(dinf, gp) < o["tol"]:
            break
        if dinf < o["tol"]:
            data["reruns"] += 1
            continue
        if d <= r <= p - 1:
            Y = polar_blocks(Y @ Q[:, :r], d)
            p = r
        nne = max(min(int(np.sum(dS < 0)), o["delta"]), 1)
        Y = polar_blocks(np.hstack([Y, o["alpha"] * vS[:, :nne]]), d)
        p += nne
        data["widened"] += 1
    Y = Y_eval
    data.update(dinf=dinf, gap=gp, p=Y.shape[1], rank=r, z=get_z(C, Y, d), dual=dual)
    if max(dinf, gp) >= o["tol"]:
        data["status"] = 1
    return Y, obj, data


# ------------------------------------------------------------------ instances of the device tests
_CACHE = {}

# (n, d, degree): the smallest at which chunking, partial waves and the device escape can still go wrong (N = 1372 of the last is
# above dense_eig_default)
INSTANCES = ((41, 2, 4), (67, 3, 6), (343, 3, 6))


def instance(n, d, degree, sigma_r=0.3, sigma_t=None, seed=0):
    """problems.pose_graph(n, d, degree, sigma_r, sigma_t, seed); sigma_t defaults to sigma_r."""
    sigma_t = sigma_r if sigma_t is None else sigma_t
    key = (n, d, degree, sigma_r, sigma_t, seed)
    if key not in _CACHE:
        from manisdp_matlab_amd import problems
        _CACHE[key] = problems.pose_graph(n, d, degree, sigma_r, sigma_t, seed)
    return _CACHE[key]


def point(n, d, p, seed=0):
    key = ("pt", n, d, p, seed)
    if key not in _CACHE:
        _CACHE[key] = random_point(n, d, p, np.random.default_rng(77 + seed + 13 * p))
    return _CACHE[key]


def reference_solve(n, d, degree, sigma, options=None):
    """The restatement's solve from the solver's start (p0 = d + 2, default_rng(0)), once per instance."""
    key = ("solve", n, d, degree, sigma, tuple(sorted((options or {}).items())))
    if key not in _CACHE:
        C = instance(n, d, degree, sigma)[0]
        _CACHE[key] = solve(C, d, start_point(n, d, d + 2, np.random.default_rng(0)), options)
    return _CACHE[key]


# the instance, start and budget of the trustregions() count test: tests/test_posegraph_ref_host.py shows that the restatement's
# counts on it do not move under 1e-14 perturbations of the start, tests/test_gpu_posegraph.py holds the device to them
COUNT_CASE = dict(n=67, d=3, degree=6, sigma=0.3, p=5, maxiter=15, maxinner=30, tolgradnorm=1e-5)


def count_case():
    c = COUNT_CASE
    C = instance(c["n"], c["d"], c["degree"], c["sigma"])[0]
    return C, point(c["n"], c["d"], c["p"])


def counts(info):
    return (info.iters, info.hessvecs, info.accepted, info.rejected, info.stop_inner[-1] if info.stop_inner else 0)
