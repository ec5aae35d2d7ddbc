"""NumPy restatement of the block-Jacobi preconditioned tCG of the pose-graph kind (msdp_set_option "precon",
msdp_pose_precon.hip): the blocks M_i^-1 of the cost matrix, precon(Y, R) = tangent_Y(blockdiag(M_i^-1) R), the preconditioned
branch of Manopt's truncated CG (tCG.m:117-125 and :260-287) and a trustregions() that runs oracle.manopt_rtr.trustregions with
it.  M_i = sym(C_[ii]) is the diagonal block of order B = d + 1 of pose i: fixed, unscaled, independent of the point.  The trust
region is then measured in the M-norm (e_Pe, e_Pd, d_Pd are the M-inner products of Manopt), Delta_bar and Delta0 keep the
values of the unpreconditioned solver.  Everything else (problem, manifold, instances, starts) is tests/posegraph_ref.py's."""
import math

import numpy as np
import scipy.sparse as sp

import posegraph_ref as B


def diag_blocks(C, d):
    """M_i = sym(C_[ii]): (n, B, B)."""
    Bo = d + 1
    C = sp.csr_matrix(C)
    n = C.shape[0] // Bo
    M = np.zeros((n, Bo, Bo))
    Cc = C.tocoo()
    keep = (Cc.row // Bo) == (Cc.col // Bo)
    np.add.at(M, (Cc.row[keep] // Bo, Cc.row[keep] % Bo, Cc.col[keep] % Bo), Cc.data[keep])
    return B.sym(M)


def minv_blocks(C, d):
    """M_i^-1 through the Cholesky factor of M_i, (n, B, B); ValueError naming the first block that has no factor."""
    M = diag_blocks(C, d)
    out = np.empty_like(M)
    eye = np.eye(d + 1)
    for i in range(M.shape[0]):
        try:
            L = np.linalg.cholesky(M[i])
        except np.linalg.LinAlgError:
            raise ValueError("diagonal block %d is not positive definite" % i)
        Li = np.linalg.solve(L, eye)
        out[i] = Li.T @ Li
    return out


def identity_blocks(n, d):
    return np.broadcast_to(np.eye(d + 1), (n, d + 1, d + 1)).copy()


def precon(Y, R, Minv, d):
    """tangent_Y(blockdiag(M_i^-1) R): Stiefel projection on the rotation rows, identity on the free row."""
    n = Y.shape[0] // (d + 1)
    Z = (Minv @ B.to3(R, d)).reshape(R.shape)
    return B.StiefelEuclid(n, d, Y.shape[1]).proj(Y, Z)


class Problem(B.Problem):
    """posegraph_ref.Problem with the preconditioner of the blocks Minv."""

    def __init__(self, C, n, d, p, Minv):
        super().__init__(C, n, d, p)
        self.Minv = Minv

    def precon(self, Y, R):
        return precon(Y, R, self.Minv, self.d)


def tCG(problem, x, grad, Delta, maxinner, kappa=0.1, theta=1.0, mininner=1):
    """tCG.m:95-292 with useRand = false and problem.precon: oracle.manopt_rtr.tCG with z = precon(r) where that has z = r.
    The stop test (:249) stays on norm_r = sqrt(<r, r>) and norm_r0; alpha, beta and the boundary step use <z, r> and the
    M-inner products e_Pe, e_Pd, d_Pd."""
    M = problem.M
    inner = lambda a, b: M.inner(x, a, b)
    eta = M.zerovec(x)
    Heta = M.zerovec(x)                      # tCG.m:103
    r = grad                                 # :104
    e_Pe = 0.0
    r_r = inner(r, r)                        # :114
    norm_r = math.sqrt(r_r)
    norm_r0 = norm_r
    z = problem.precon(x, r)                 # :121
    z_r = inner(z, r)                        # :126
    d_Pd = z_r
    mdelta = z                               # :130
    e_Pd = 0.0
    model_value = 0.0                        # :148
    stop_tCG = 5                             # :157
    j = 0
    for j in range(1, maxinner + 1):         # :160
        Hmdelta = problem.hess(x, mdelta)    # :163
        d_Hd = inner(mdelta, Hmdelta)        # :166
        alpha = z_r / d_Hd if d_Hd != 0.0 else math.copysign(math.inf, z_r) if z_r != 0 else math.nan
        e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd   # :173
        if d_Hd <= 0 or e_Pe_new >= Delta ** 2:                         # :183
            tau = (-e_Pd + math.sqrt(e_Pd * e_Pd + d_Pd * (Delta ** 2 - e_Pe))) / d_Pd  # :188
            eta = eta - tau * mdelta         # :192
            Heta = Heta - tau * Hmdelta      # :198
            stop_tCG = 1 if d_Hd <= 0 else 2
            break
        e_Pe = e_Pe_new                      # :214
        new_eta = eta - alpha * mdelta       # :215
        new_Heta = Heta - alpha * Hmdelta    # :220
        new_model_value = inner(new_eta, grad) + 0.5 * inner(new_eta, new_Heta)  # :227
        if new_model_value >= model_value:   # :228
            stop_tCG = 6
            break
        eta = new_eta
        Heta = new_Heta
        model_value = new_model_value        # :235
        r = r - alpha * Hmdelta              # :238
        r_r = inner(r, r)                    # :241
        norm_r = math.sqrt(r_r)
        if j >= mininner and norm_r <= norm_r0 * min(norm_r0 ** theta, kappa):  # :249
            stop_tCG = 3 if kappa < norm_r0 ** theta else 4
            break
        z = problem.precon(x, r)             # :265
        zold_rold = z_r
        z_r = inner(z, r)                    # :270
        beta = z_r / zold_rold               # :272
        mdelta = z + beta * mdelta           # :273
        mdelta = M.tangent(x, mdelta)        # :283
        e_Pd = beta * (e_Pd + alpha * d_Pd)  # :286
        d_Pd = z_r + beta * beta * d_Pd      # :287
    return eta, Heta, j, stop_tCG


def stop_margin(problem, x, grad, Delta, maxinner, kappa=0.1, theta=1.0, mininner=1):
    """The smallest relative distance from equality among the stop tests (:183 curvature and radius, :228 model, :249 residual)
    the tCG above evaluates from x: a width whose margin is below 1e-10 may end a trip apart on the device."""
    margins = []
    M = problem.M
    inner = lambda a, b: M.inner(x, a, b)
    eta, Heta, r = M.zerovec(x), M.zerovec(x), grad
    e_Pe, e_Pd, model_value = 0.0, 0.0, 0.0
    norm_r0 = math.sqrt(inner(r, r))
    z = problem.precon(x, r)
    z_r = d_Pd = inner(z, r)
    mdelta = z
    for j in range(1, maxinner + 1):
        Hm = problem.hess(x, mdelta)
        d_Hd = inner(mdelta, Hm)
        margins.append(abs(d_Hd) / max(M.norm(x, mdelta) * M.norm(x, Hm), 1e-300))
        if d_Hd <= 0:
            break
        alpha = z_r / d_Hd
        e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd
        margins.append(abs(e_Pe_new - Delta ** 2) / Delta ** 2)
        if e_Pe_new >= Delta ** 2:
            break
        e_Pe = e_Pe_new
        eta, Heta = eta - alpha * mdelta, Heta - alpha * Hm
        new_model = inner(eta, grad) + 0.5 * inner(eta, Heta)
        margins.append(abs(new_model - model_value) / max(abs(model_value), abs(new_model), 1e-300))
        if new_model >= model_value:
            break
        model_value = new_model
        r = r - alpha * Hm
        norm_r = math.sqrt(inner(r, r))
        bound = norm_r0 * min(norm_r0 ** theta, kappa)
        margins.append(abs(norm_r - bound) / bound)
        if j >= mininner and norm_r <= bound:
            break
        z = problem.precon(x, r)
        z_r_new = inner(z, r)
        beta = z_r_new / z_r
        z_r = z_r_new
        mdelta = M.tangent(x, z + beta * mdelta)
        e_Pd = beta * (e_Pd + alpha * d_Pd)
        d_Pd = z_r + beta * beta * d_Pd
    return min(margins) if margins else 1.0


def trustregions(C, Y0, d, maxiter, maxinner, tolgradnorm, Minv=None, **radii):
    """oracle.manopt_rtr.trustregions on the pose-graph problem with the tCG above in place of its own; Minv defaults to the
    blocks of C, radii (Delta_bar, Delta0) to those of the manifold.  Returns (Y, f, info)."""
    from oracle import manopt_rtr
    if Minv is None:
        Minv = minv_blocks(C, d)
    prob = Problem(C, Y0.shape[0] // (d + 1), d, Y0.shape[1], Minv)
    plain = manopt_rtr.tCG
    manopt_rtr.tCG = tCG
    try:
        return manopt_rtr.trustregions(prob, np.array(Y0, dtype=np.float64), maxiter, maxinner, tolgradnorm, **radii)
    finally:
        manopt_rtr.tCG = plain


def plain_trustregions(C, Y0, d, maxiter, maxinner, tolgradnorm, **radii):
    """posegraph_ref.trustregions (the oracle's own tCG) with the radii passed on."""
    from oracle import manopt_rtr
    prob = B.Problem(C, Y0.shape[0] // (d + 1), d, Y0.shape[1])
    return manopt_rtr.trustregions(prob, np.array(Y0, dtype=np.float64), maxiter, maxinner, tolgradnorm, **radii)


def tcg_step(C, Y, d, Delta, maxinner, Minv=None):
    """(eta, Heta, inner iterations, stop reason) of one tCG from Y at radius Delta: the preconditioned tCG above with the blocks
    Minv, the oracle's own tCG without them."""
    from oracle import manopt_rtr
    n = Y.shape[0] // (d + 1)
    prob = B.Problem(C, n, d, Y.shape[1]) if Minv is None else Problem(C, n, d, Y.shape[1], Minv)
    prob.cost(Y)
    return (manopt_rtr.tCG if Minv is None else tCG)(prob, Y, prob.grad(Y), Delta, maxinner)


def solve(C, d, Y0, options=None):
    """posegraph_ref.solve with the preconditioned trustregions()."""
    Minv = minv_blocks(C, d)
    plain = B.trustregions
    B.trustregions = lambda C_, Y, d_, a, b, c: trustregions(C_, Y, d_, a, b, c, Minv)
    try:
        return B.solve(C, d, Y0, options)
    finally:
        B.trustregions = plain


_CACHE = {}


def reference_solve(n, d, degree, sigma):
    """The preconditioned restatement's solve from the solver's start (p0 = d + 2, default_rng(0)), once per instance."""
    key = (n, d, degree, sigma)
    if key not in _CACHE:
        C = B.instance(n, d, degree, sigma)[0]
        _CACHE[key] = solve(C, d, B.start_point(n, d, d + 2, np.random.default_rng(0)))
    return _CACHE[key]


# the trustregions() count cases: instance(n, d, degree, 0.3), point(n, d, p) and a budget.  tests/test_posegraph_precon_ref_host.py
# shows that the restatement's counts on each hold under twenty 1e-14 perturbations of the start; tests/test_gpu_posegraph_precon.py
# holds the device to them.  Budgets that run to tolgradnorm = 1e-8 are not count-stable and are used for cost comparisons only.
# Case C ends at its gradient tolerance after 25 iterations: with a budget of 22 its counts held but its cost moved by up to
# 1.4e-9 relative under those perturbations (an iteration with a negative-curvature exit lies in between), above the 1e-11 of the rule.
COUNT_CASES = {
    "A": dict(n=67, d=3, degree=6, sigma=0.3, p=5, maxiter=15, maxinner=30, tolgradnorm=1e-5),
    "B": dict(n=67, d=3, degree=6, sigma=0.3, p=5, maxiter=24, maxinner=40, tolgradnorm=1e-5),
    "C": dict(n=41, d=2, degree=4, sigma=0.3, p=4, maxiter=30, maxinner=40, tolgradnorm=1e-5),
    "D": dict(n=67, d=3, degree=6, sigma=0.3, p=8, maxiter=18, maxinner=40, tolgradnorm=1e-4),
}


def count_case(name):
    c = COUNT_CASES[name]
    return B.instance(c["n"], c["d"], c["degree"], c["sigma"])[0], B.point(c["n"], c["d"], c["p"])


def count_reference(name):
    """(Y, f, info) of the restatement on a count case, once."""
    key = ("count", name)
    if key not in _CACHE:
        c = COUNT_CASES[name]
        C, Y0 = count_case(name)
        _CACHE[key] = trustregions(C, Y0, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
    return _CACHE[key]


counts = B.counts
