"""CPU tests of the multiblock dual approach: problems.bqpsos_sparse / qssos_sparse (reference
src/basicfunction/bqpsos_sparse.m, qssos_sparse.m), the NumPy restatement of src/dual/ManiDSDP_multiblock.m in
dual_multiblock_ref.py (derivatives, strong duality against the oracle's primal ManiSDP_multiblock on bqpmom_sparse /
qsmom_sparse), and the defaults of solvers.ManiDSDP_multiblock and matlab/ManiDSDP_multiblock.m (:12-28).  No GPU needed."""
import os
import re
import sys
from itertools import combinations, combinations_with_replacement

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dual_multiblock_ref as R  # noqa: E402
from oracle.manisdp_ref import BlockVec  # noqa: E402

REF_DEFAULTS = dict(min_facsize=2, ADMM_maxiter=1000, gama=2, sigma0=1e-1, sigma_min=1e-2, sigma_max=1e7, tol=1e-8, theta=1e-2,
                    delta=8, alpha=0.2, tolgradnorm=1e-8, TR_maxinner=20, TR_maxiter=4, tau1=1e1, tau2=1e1,
                    line_search=1)                                 # src/dual/ManiDSDP_multiblock.m:12-28


def _problems():
    from manisdp_matlab_amd import problems
    return problems


def _union(cliques, multilinear):
    out = set()
    for I in cliques:
        for d in range(5):
            out.update(combinations(I, d) if multilinear else combinations_with_replacement(I, d))
    return out


@pytest.mark.parametrize("t,q", [(2, 4), (3, 5), (2, 6)])
def test_bqpsos_sparse_sizes(t, q):
    P = _problems()
    cliques, n = P.chain_cliques(t, q)
    lsp = len(_union(cliques, True))
    A, b, c, K, dAAt = P.bqpsos_sparse(n, cliques, np.zeros(lsp))
    mb = [1 + q + q * (q - 1) // 2] * t
    assert K == {"f": 1, "s": mb}
    assert A.shape == (lsp, 1 + sum(v * v for v in mb)) and b.shape == (lsp,) and c.shape == (A.shape[1],)
    assert c[0] == 1 and np.count_nonzero(c) == 1
    assert A[0, 0] == 1 and A[:, 0].nnz == 1                         # the free lambda sits on the constant monomial
    Ap = sp.csr_matrix(A)[:, 1:]
    assert np.array_equal(np.asarray(Ap.multiply(Ap).sum(axis=1)).ravel(), dAAt)
    assert dAAt[0] == sum(mb)


@pytest.mark.parametrize("t,q", [(2, 3), (3, 4), (2, 5)])
def test_qssos_sparse_sizes(t, q):
    P = _problems()
    cliques, n = P.chain_cliques(t, q)
    lsp = len(_union(cliques, False))
    A, b, c, K, dAAt = P.qssos_sparse(n, cliques, np.zeros(lsp))
    mb = [(q + 1) * (q + 2) // 2] * t
    assert K == {"f": sum(mb) + 1, "s": mb}
    assert A.shape == (lsp, sum(mb) + 1 + sum(v * v for v in mb))
    Ap = sp.csr_matrix(A)[:, K["f"]:]
    assert np.array_equal(np.asarray(Ap.multiply(Ap).sum(axis=1)).ravel(), dAAt)


def test_sp_order_is_sortrows():
    """The sorted sp of the generators is MATLAB's sortrows of the exponent vectors (a_1, ..., a_n) ascending."""
    P = _problems()
    cliques, n = P.chain_cliques(3, 4)
    for ml in (True, False):
        spl = P._sos_sparse_support(cliques, ml)
        E = np.zeros((len(spl), n), dtype=int)
        for k, mo in enumerate(spl):
            for v in mo:
                E[k, v] += 1
        order = np.lexsort(E.T[::-1])
        assert np.array_equal(order, np.arange(len(spl)))


def _sos_residual(gen, t, q, pts_fn, seed):
    """b = A_psd(S) + B(w) as polynomial coefficients (sp order) against sum_k v_k(x)' S_k v_k(x) + the free terms at points."""
    P = _problems()
    cliques, n = P.chain_cliques(t, q)
    ml = gen == "bqp"
    spl = P._sos_sparse_support(cliques, ml)
    A, _, _, K, _ = (P.bqpsos_sparse if ml else P.qssos_sparse)(n, cliques, np.zeros(len(spl)))
    rng = np.random.default_rng(seed)
    mb = K["s"]
    Sb = []
    for m_ in mb:
        G = rng.standard_normal((m_, m_))
        Sb.append(G @ G.T)
    wv = rng.standard_normal(K["f"])
    vecS = np.concatenate([S.ravel(order="F") for S in Sb])
    poly = sp.csr_matrix(A) @ np.concatenate([wv, vecS])
    bases = []
    for I in cliques:
        bs = [()] + [(a,) for a in I]
        for jb in range(len(I)):
            for ia in range(jb + (0 if ml else 1)):
                bs.append((I[ia], I[jb]))
        bases.append(bs)
    worst = 0.0
    for x in pts_fn(rng, n, cliques):
        mono = lambda mo: float(np.prod([x[v] for v in mo])) if mo else 1.0   # noqa: E731
        lhs = sum(poly[k] * mono(mo) for k, mo in enumerate(spl))
        rhs = wv[0]
        for k, bs in enumerate(bases):
            v = np.array([mono(mo) for mo in bs])
            rhs += v @ Sb[k] @ v
        if not ml:                                                   # h_k(x) (|x_{I_k}|^2 - 1) vanish on the spheres
            col = 1
            for k, I in enumerate(cliques):
                for mo in bases[k]:
                    rhs += wv[col] * mono(mo) * (sum(x[a] ** 2 for a in I) - 1.0)
                    col += 1
        worst = max(worst, abs(lhs - rhs) / max(1.0, abs(rhs)))
    return worst


def test_bqpsos_sparse_sos_identity():
    pts = lambda rng, n, cl: [rng.choice([-1.0, 1.0], n) for _ in range(8)]   # noqa: E731
    assert _sos_residual("bqp", 3, 4, pts, 1) < 1e-12


def test_qssos_sparse_sos_identity():
    def pts(rng, n, cliques):                                        # off the spheres: the multiplier terms count
        return [rng.standard_normal(n) for _ in range(8)]
    assert _sos_residual("qs", 2, 3, pts, 2) < 1e-12


def _instance(nob, nf, seed=3):
    """nob = nb takes the reference's shortcut tt = bA - sigma*As (:258), the gradient only where D\\A*A' = I and x lies in
    the null space of A'(D\\A): there the constraints get pairwise disjoint supports and x is projected."""
    nset = [4, 6, 1, 5]
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum([n * n for n in nset])])
    m = 20
    rows = []
    if nob == len(nset):
        pairs = [(blk, i, j) for blk, n in enumerate(nset) for j in range(n) for i in range(j + 1)]
        order = rng.permutation(len(pairs))
    for k in range(m if nob < len(nset) else 0):
        v = np.zeros(off[-1])
        for blk in rng.choice(len(nset), size=2):
            n = nset[blk]
            Mk = np.zeros((n, n))
            for _ in range(3):
                i, j = rng.integers(0, n, 2)
                a = rng.standard_normal()
                Mk[i, j] += a; Mk[j, i] += a
            v[off[blk]:off[blk + 1]] += Mk.ravel(order="F")
        rows.append(v)
    for k in range(m if nob == len(nset) else 0):
        v = np.zeros(off[-1])
        for q in order[2 * k:2 * k + 2]:
            blk, i, j = pairs[q]
            n = nset[blk]
            a = rng.standard_normal()
            v[off[blk] + i + j * n] += a
            if i != j:
                v[off[blk] + j + i * n] += a
        rows.append(v)
    Apsd = sp.csr_matrix(np.array(rows))
    B = sp.csr_matrix(rng.standard_normal((m, nf))) if nf else None
    cp = np.concatenate([(lambda C: 0.2 * (C + C.T))(rng.standard_normal((n, n))).ravel(order="F") for n in nset])
    prob = R.DualMultiblockProblem(Apsd, B, rng.standard_normal(m), cp, rng.standard_normal(nf),
                                   np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel(), nset, nob)
    prob.sigma = 0.7
    prob.x = np.concatenate([(lambda Z: 0.15 * (Z + Z.T))(rng.standard_normal((n, n))).ravel(order="F") for n in nset])
    if nob == len(nset):
        prob.x = prob.x - prob.At @ (prob.iAt @ prob.x)
    prob.w = rng.standard_normal(nf)
    p = [3, 4, 1, 2]
    prob.set_widths(p)
    return prob, rng


@pytest.mark.parametrize("nob,nf", [(4, 0), (0, 0), (0, 2), (2, 0), (2, 2)])
def test_restatement_gradient_and_hessian_by_finite_differences(nob, nf):
    """With nob = nb the reference's closures drop the terms of A'(iA'*As) and iAB*Af (:258, :283): they are the derivatives
    only for D\\A*A' = I, x in the null space of A'(D\\A) and no free part; the instance of that case is built so."""
    prob, rng = _instance(nob, nf)
    M = prob.M
    Y = M.rand(rng)
    Z = BlockVec([rng.standard_normal(yi.shape) for yi in Y.b])
    U = M.proj(Y, Z)
    G = prob.grad(Y)
    f0 = prob.cost(Y)
    h = 1e-6
    fd = (prob.cost(M.retr(Y, U * h)) - prob.cost(M.retr(Y, U * (-h)))) / (2 * h)
    assert abs(fd - M.inner(Y, G, U)) <= 1e-6 * max(1.0, abs(fd))
    prob.grad(Y)
    H = prob.hess(Y, U)
    g1 = M.proj(Y, prob.grad(M.retr(Y, U * h)))
    g2 = M.proj(Y, prob.grad(M.retr(Y, U * (-h))))
    fdH = (g1 - g2) * (1.0 / (2 * h))
    num = np.sqrt(sum(float(np.sum((a - b) ** 2)) for a, b in zip(fdH.b, H.b)))
    den = np.sqrt(sum(float(np.sum(b ** 2)) for b in H.b))
    assert num <= 1e-5 * max(1.0, den)
    assert np.isfinite(f0)


def test_restatement_strong_duality_bqp():
    """bqpsos_sparse and bqpmom_sparse of one small chain BQP: the restatement's dual optimum equals the oracle's primal
    multiblock optimum."""
    from oracle import manisdp_ref as O
    P = _problems()
    cliques, n = P.chain_cliques(2, 4)
    coe = np.random.default_rng(1).standard_normal(len(P.bqp_sparse_monomials(cliques)))
    A, b, c, K, dAAt = P.bqpsos_sparse(n, cliques, P.bqpsos_sparse_coe(cliques, coe))
    K["nob"] = len(K["s"])
    maxb = float(np.max(np.abs(b)))
    _, obj, data = R.ManiDSDP_multiblock(A, b / maxb, c, K, {"dAAt": dAAt, "tol": 1e-8, "ADMM_maxiter": 400})
    assert data["status"] == 0
    At, bp, cp, Kp = P.bqpmom_sparse(n, cliques, coe)
    _, fp, dp = O.ManiSDP_multiblock(At, bp, cp, Kp, {"tol": 1e-8, "line_search": 1, "tau1": 1})
    assert dp["status"] == 0
    assert abs(obj * maxb - fp) <= 1e-6 * max(1.0, abs(fp))


def test_restatement_strong_duality_qsphere():
    from oracle import manisdp_ref as O
    P = _problems()
    cliques, n = P.chain_cliques(2, 3)
    coe = np.random.default_rng(1).standard_normal(len(P.quartic_sparse_monomials(cliques)))
    A, b, c, K, dAAt = P.qssos_sparse(n, cliques, P.qssos_sparse_coe(cliques, coe))
    K["nob"] = 0
    maxb = float(np.max(np.abs(b)))
    o = {"dAAt": dAAt, "tol": 1e-8, "gama": 2, "alpha": 0.01, "sigma0": 1e-2, "theta": 1e-2, "delta": 6, "line_search": 0,
         "ADMM_maxiter": 600}
    _, obj, data = R.ManiDSDP_multiblock(A, b / maxb, c, K, o)
    assert data["status"] == 0
    At, bp, cp, Kp = P.qsmom_sparse(n, cliques, coe)
    _, fp, dp = O.ManiSDP_multiblock(At, bp, cp, Kp, {"tol": 1e-8, "line_search": 1, "tau1": 1})
    assert dp["status"] == 0
    assert abs(obj * maxb - fp) <= 1e-6 * max(1.0, abs(fp))


def test_solver_defaults_are_the_references():
    from manisdp_matlab_amd import solvers
    assert solvers.DEFAULTS["dual_multiblock"] == REF_DEFAULTS
    assert solvers.DATA_FIELDS["dual_multiblock"] == ("X", "y", "S", "w", "gap", "pinf", "dinf", "gradnorm", "time", "status")
    assert R.DEFAULTS == REF_DEFAULTS


def test_matlab_driver_defaults_are_the_references():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "manisdp-matlab_amd", "matlab", "ManiDSDP_multiblock.m")).read()
    body = re.search(r"defaults\s*=\s*\{(.*?)\};", src, re.S).group(1).replace("...", " ")
    got = {name: float(val) for name, val in re.findall(r"'(\w+)'\s*,\s*([-+0-9.eE]+)", body)}
    assert got == {k: float(v) for k, v in REF_DEFAULTS.items()}
    assert "manisdp_mex('create_dual_multiblock'," in src
