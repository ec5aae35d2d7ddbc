"""Constructed constraint data for the primal affine kinds (MSDP_KIND_UNITDIAG, _UNITTRACE, _GENERIC), plain NumPy / SciPy and
seeded: every family is built so that the set-up's plans (manisdp-matlab_amd/csrc/msdp_affine_plan.h) take one particular
branch, which the shipped instances (gpp, mcp, bqp, theta) reach by accident of their structure or not at all.

A family returns ``(At, b, c, n, facts)`` in the layout of ``Handle.affine``: ``At`` is n^2 x m CSC over the column-major vec
of symmetric A_k, ``c`` the vec of a symmetric C with entries of size about 1/sqrt(n).  ``facts`` (see ``facts_of``) are computed
from ``At`` and ``c`` alone and restate in NumPy what the plans decide, so that the host test can check the construction without
a device and the GPU test can compare them with ``Handle.affine_plan()``.

Family                          pins
dense_short(n, g)               k_adjoint_gram<BW = g, PK = true>, no tail; every entry touched (no support list)
dense_short(.., normal=True)    more than 256 distinct coefficients of B: PK = false
dense_short(.., wide=(6, 6))    six constraints of 6 entries among groups of 3: BW = 4 and a tail of 36 rows
dense_short(65, 6)              every row of B wider than 4: the whole matrix goes through the one-wave-per-row tail
dense_short(.., asym=1e-13)     data not exactly symmetric: no upper view, no tiles, k_adjoint_dense
shared(97)                      four entries in 13 constraints each (> ADJ_LONG): off-diagonal tile, diagonal tile, diagonal entry
support(96)                     few touched entries, a hub row of 81 of them (second turn of k_support_spmm's q0 loop), no long constraint
support(160)                    the same with the trace row long (> 128 nonzeros)
support(160, nlong=20)          21 long constraints > MSDP_WAVES: the side job of the contraction is refused
crowded(40)                     many short constraints on a small matrix: the k_sddmm1 grid is capped at n rows in mode 2"""
import numpy as np
import scipy.sparse as sp

COEFS = np.array([1.0, -0.5, 0.25])
SDDMM_CHUNK, FIN_SHORT, ADJ_T, ADJ_LONG, MSDP_WAVES = 16, 8, 32, 8, 16      # msdp_affine_plan.h, msdp_device.h


def _assemble(n, cons, rng, trace_rows=()):
    """At (n^2 x m, CSC) from a list of constraints, each a list of (i, j, v) with i <= j: A_k gets v at (i, j) and (j, i)."""
    rows, cols, vals = [], [], []
    for k, ent in enumerate(cons):
        for i, j, v in ent:
            rows.append(i + j * n); cols.append(k); vals.append(v)
            if i != j:
                rows.append(j + i * n); cols.append(k); vals.append(v)
    At = sp.csc_matrix((vals, (rows, cols)), shape=(n * n, len(cons)))
    At.sum_duplicates()
    At.sort_indices()
    return At


def _cost(n, rng):
    G = rng.standard_normal((n, n))
    return ((G + G.T) / (2.0 * np.sqrt(n))).ravel(order="F")


def _finish(n, cons, rng, asym=0.0):
    At = _assemble(n, cons, rng)
    b = rng.standard_normal(At.shape[1])
    c = _cost(n, rng)
    if asym:
        c[3 + 7 * n] += asym                                     # C(3, 7) alone: C(7, 3) keeps its value
    return At, b, c, n, facts_of(At, c, n)


def dense_short(n, g, normal=False, wide=(0, 0), asym=0.0, seed=0):
    """The n (n + 1) / 2 upper entries, shuffled and cut into groups of ``g``: one constraint per group.  ``wide = (k, w)``:
    the first k groups hold w entries each.  ``normal``: N(0, 1) coefficients instead of {1, -0.5, 0.25}."""
    rng = np.random.default_rng([seed, n, g])
    iu, ju = np.triu_indices(n)
    perm = rng.permutation(iu.size)
    cuts, pos = [], 0
    for q in range(wide[0]):
        cuts.append((pos, pos + wide[1])); pos += wide[1]
    while pos < perm.size:
        cuts.append((pos, min(pos + g, perm.size))); pos += g
    cons = []
    for lo, hi in cuts:
        v = rng.standard_normal(hi - lo) if normal else rng.choice(COEFS, hi - lo)
        cons.append([(int(iu[e]), int(ju[e]), float(x)) for e, x in zip(perm[lo:hi], v)])
    return _finish(n, cons, rng, asym)


SHARED_ENTRIES = ((0, 1), (33, 70), (5, 5), (2, 3))             # diagonal tile; off-diagonal tile (1, 2); diagonal entry; diagonal tile


def shared(n=97, seed=0):
    """dense_short(n, 2) plus 12 constraints that each hold the four entries SHARED_ENTRIES with the coefficient 0.5 + k."""
    rng = np.random.default_rng([seed, n, 77])
    iu, ju = np.triu_indices(n)
    perm = rng.permutation(iu.size)
    cons = []
    for lo in range(0, perm.size, 2):
        e = perm[lo:lo + 2]
        cons.append([(int(iu[q]), int(ju[q]), float(x)) for q, x in zip(e, rng.choice(COEFS, e.size))])
    for k in range(12):
        cons.append([(i, j, 0.5 + k) for i, j in SHARED_ENTRIES])
    return _finish(n, cons, rng)


def _pair(rng, n):
    i, j = rng.choice(n, 2, replace=False)
    return (int(min(i, j)), int(max(i, j)), float(rng.choice(COEFS)))


def support(n, npairs=None, hub=None, nlong=0, long_first=False, seed=1):
    """``npairs`` constraints E_ij + E_ji on random pairs; a hub: ``hub`` constraints E_0j + E_j0, every third also holding
    E_jj; the trace row; ``nlong`` constraints of 70 random upper pairs with i < 24 or j < 24 (140 nonzeros: long).
    ``long_first`` puts the long constraints (trace row included where it is long) in front of the short ones."""
    npairs = {96: 150, 160: 300}[n] if npairs is None else npairs
    hub = {96: 80, 160: 100}[n] if hub is None else hub
    rng = np.random.default_rng([seed, n, 55])
    short = [[_pair(rng, n)] for _ in range(npairs)]
    for j in range(1, hub + 1):
        ent = [(0, j, float(rng.choice(COEFS)))]
        if j % 3 == 0:
            ent.append((j, j, float(rng.choice(COEFS))))
        short.append(ent)
    trace = [[(i, i, 1.0) for i in range(n)]]
    longs = []
    for _ in range(nlong):
        seen = {}
        while len(seen) < 70:
            i, j, v = _pair(rng, n)
            if i < 24 or j < 24:
                seen[(i, j)] = v
        longs.append([(i, j, v) for (i, j), v in sorted(seen.items())])
    tail = trace + longs
    return _finish(n, tail + short if long_first else short + tail, rng)


def crowded(n=40, seed=0):
    """700 constraints on random pairs, 3 constraints of 70 pairs (long), the trace row (short at n = 40)."""
    rng = np.random.default_rng([seed, n, 33])
    cons = [[_pair(rng, n)] for _ in range(700)]
    for _ in range(3):
        seen = {}
        while len(seen) < 70:
            i, j, v = _pair(rng, n)
            seen[(i, j)] = v
        cons.append([(i, j, v) for (i, j), v in sorted(seen.items())])
    cons.append([(i, i, 1.0) for i in range(n)])
    return _finish(n, cons, rng)


def dense_nS(n):
    """Padded row length of the dense operands (msdp_dense_nS: the next multiple of 16)."""
    return (n + 15) // 16 * 16


def facts_of(At, c, n):
    """What the data is, and what msdp_affine_plan.h decides from it, restated:
    touched       matrix entries (of n^2) that occur in some constraint
    max_share     largest number of constraints on one entry;  max_row: most touched entries in one matrix row
    upper_per_k   entries i <= j per constraint (array);  nnz_per_k: nonzeros per constraint
    usym          C and every A_k symmetric entry by entry
    nlong / nshort / nlit   constraints of more than FIN_SHORT items of SDDMM_CHUNK nonzeros, the others, the items of the long ones
    nsup          touched when 8 * touched <= n^2, else 0
    ntp           upper 32 x 32 tile pairs (0 unless usym);  nlong_e: upper entries in more than ADJ_LONG constraints
    bW, bnlong, packed   ELL width of B = sum_k a_k c_k' over the upper entries by the 99 % rule (rows counted once per tile
                  element, so twice in the lower half of a diagonal tile), rows wider than bW, at most 256 distinct coefficients"""
    At = sp.csc_matrix(At)
    m = At.shape[1]
    ii, jj = At.indices % n, At.indices // n
    kk = np.repeat(np.arange(m), np.diff(At.indptr))
    nnz_per_k = np.diff(At.indptr)
    share = np.bincount(ii * n + jj, minlength=n * n).reshape(n, n)          # [i, j]
    touched = int(np.count_nonzero(share))
    up = ii <= jj
    upper_per_k = np.bincount(kk[up], minlength=m)
    M = sp.csr_matrix((At.data, (ii * n + jj, kk)), shape=(n * n, m))
    Cm = np.asarray(c).reshape(n, n, order="F")
    P = sp.csr_matrix((np.ones(n * n), (np.arange(n * n), (np.arange(n * n) % n) * n + np.arange(n * n) // n)), shape=(n * n, n * n))
    usym = int(np.array_equal(Cm, Cm.T) and (M - P @ M).nnz == 0 and abs(M - P @ M).sum() == 0)
    items = (nnz_per_k + SDDMM_CHUNK - 1) // SDDMM_CHUNK
    longk = items > FIN_SHORT
    f = dict(n=n, m=m, touched=touched, max_share=int(share.max()), max_row=int(np.count_nonzero(share, axis=1).max()),
             upper_per_k=upper_per_k, nnz_per_k=nnz_per_k, usym=usym, nlong=int(longk.sum()), nshort=int((~longk).sum()),
             nlit=int(items[longk].sum()), nsup=touched if 0 < touched * 8 <= n * n else 0, ntp=0, nlong_e=0, bW=0, bnlong=0, packed=0)
    if not usym:
        return f
    nt = (dense_nS(n) + ADJ_T - 1) // ADJ_T
    f["ntp"] = nt * (nt + 1) // 2
    f["nlong_e"] = int(np.count_nonzero(np.triu(share) > ADJ_LONG))
    if not (0 < upper_per_k.max() <= 8 and At.nnz * 8 >= n * n):
        return f
    # B over the upper entries: row e = sum_k a_k[e] * (c_k with the diagonal halved)
    Ru = sp.csr_matrix((At.data[up], (ii[up] * n + jj[up], kk[up])), shape=(n * n, m))
    Uc = sp.csr_matrix((np.where(ii[up] == jj[up], 0.5, 1.0) * At.data[up], (kk[up], ii[up] * n + jj[up])), shape=(m, n * n))
    B = (Ru @ Uc).tocsr()
    width = np.diff(B.indptr).reshape(n, n)
    i, j = np.triu_indices(n)
    w_up = width[i, j]
    weight = np.where((i // ADJ_T == j // ADJ_T) & (i != j), 2, 1)           # a diagonal tile holds (i, j) and (j, i)
    nonempty = int(weight[w_up > 0].sum())
    bW, cum = 4, 0
    for w in range(1, 5):
        cum += int(weight[w_up == w].sum())
        if cum * 1000 >= nonempty * 990:
            bW = w
            break
    f["bW"] = bW
    f["bnlong"] = int(np.count_nonzero(w_up > bW))
    short_rows = np.repeat(np.diff(B.indptr) <= bW, np.diff(B.indptr))
    f["packed"] = int(np.unique(np.concatenate([[0.0], B.data[short_rows]])).size <= 256 and n * dense_nS(n) < (1 << 24))
    return f


# ------------------------------------------------------------------ the families by name, with the plan each must reach
# family -> conditions on the facts (exact value, ">0", "=0", ">16")
_TABLE = [
    ("ds33_1", lambda: dense_short(33, 1), dict(usym=1, bW=1, packed=1, bnlong="=0", nsup="=0", ntp=3)),
    ("ds33_2", lambda: dense_short(33, 2), dict(usym=1, bW=2, packed=1, bnlong="=0", nsup="=0", ntp=3)),
    ("ds33_3", lambda: dense_short(33, 3), dict(usym=1, bW=3, packed=1, bnlong="=0", nsup="=0", ntp=3)),
    ("ds33_4", lambda: dense_short(33, 4), dict(usym=1, bW=4, packed=1, bnlong="=0", nsup="=0", ntp=3)),
    ("ds65_1", lambda: dense_short(65, 1), dict(usym=1, bW=1, packed=1, bnlong="=0", nsup="=0", ntp=6)),
    ("ds65_2", lambda: dense_short(65, 2), dict(usym=1, bW=2, packed=1, bnlong="=0", nsup="=0", ntp=6)),
    ("ds65_3", lambda: dense_short(65, 3), dict(usym=1, bW=3, packed=1, bnlong="=0", nsup="=0", ntp=6)),
    ("ds65_4", lambda: dense_short(65, 4), dict(usym=1, bW=4, packed=1, bnlong="=0", nsup="=0", ntp=6)),
    ("ds65_2_normal", lambda: dense_short(65, 2, normal=True), dict(usym=1, bW=2, packed=0)),
    ("ds65_3_wide", lambda: dense_short(65, 3, wide=(6, 6)), dict(usym=1, bW=4, bnlong=36)),
    ("ds65_6", lambda: dense_short(65, 6), dict(usym=1, bW=4, bnlong=">0")),
    ("ds65_2_asym", lambda: dense_short(65, 2, asym=1e-13), dict(usym=0, ntp=0, bW=0)),
    ("shared97", lambda: shared(97), dict(usym=1, nlong_e=4, bnlong=4, bW=2)),
    ("support96", lambda: support(96), dict(usym=1, nsup=">0", nlong="=0", bW=0)),
    ("support160", lambda: support(160), dict(usym=1, nsup=">0", nlong=1, nlit=">0", bW=0)),
    ("support160_first", lambda: support(160, long_first=True), dict(usym=1, nsup=">0", nlong=1, nlit=">0", bW=0)),
    ("support160_long", lambda: support(160, nlong=20), dict(usym=1, nsup=">0", nlong=">16", nlit=">0", bW=0)),
    ("support160_long_first", lambda: support(160, nlong=20, long_first=True), dict(usym=1, nsup=">0", nlong=">16", nlit=">0", bW=0)),
    ("crowded40", lambda: crowded(40), dict(usym=1, nsup="=0", bW=0, nlong=3, nshort=701, nlit=27)),
    # dense_short(n, 2) at the edges of the 32-tile and of the padded row (the entry-wise adjoint check)
    ("ds31_2", lambda: dense_short(31, 2), dict(usym=1, bW=2, packed=1, ntp=1)),
    ("ds32_2", lambda: dense_short(32, 2), dict(usym=1, bW=2, packed=1, ntp=1)),
    ("ds63_2", lambda: dense_short(63, 2), dict(usym=1, bW=2, packed=1, ntp=3)),
    ("ds64_2", lambda: dense_short(64, 2), dict(usym=1, bW=2, packed=1, ntp=3)),
]
FAMILIES = {name: (make, cond) for name, make, cond in _TABLE}


def holds(facts, cond):
    """The conditions of TABLE on a dict of facts (the GPU test applies the same function to Handle.affine_plan())."""
    bad = []
    for key, want in cond.items():
        v = facts[key]
        ok = v > 0 if want == ">0" else v == 0 if want == "=0" else v > 16 if want == ">16" else v == want
        if not ok:
            bad.append((key, want, v))
    return bad


# ------------------------------------------------------------------ brute-force restatement of the three primal closures
def dense_constraints(At, n):
    """The A_k as an m x n x n array."""
    At = sp.csc_matrix(At)
    return np.asarray(At.todense()).T.reshape(At.shape[1], n, n).transpose(0, 2, 1)        # [k, i, j] = At[i + j n, k]


class Brute:
    """f(Y) = <C, YY'> + sigma/2 |A(YY') - b - y/sigma|^2 with dense A_k and einsum; Euclidean gradient 2 S Y with
    S = C + sigma sum_k Axb_k A_k, Euclidean Hess-vec 2 S U + 4 sigma sum_k <A_k, U Y'> A_k Y (symmetric data), and the Riemannian
    forms of the oblique manifold (rows of norm 1: ManiSDP_unitdiag.m:160-170), the sphere (|Y|_F = 1: ManiSDP_unittrace.m:161-176)
    and the flat space (ManiSDP.m:157-164)."""

    def __init__(self, kind, At, b, c, n, y, sigma):
        self.kind, self.A, self.b, self.y, self.sigma = kind, dense_constraints(At, n), b, y, sigma
        self.C = np.asarray(c).reshape(n, n, order="F")

    def parts(self, Y):
        Axb = np.einsum("kij,ip,jp->k", self.A, Y, Y) - self.b - self.y / self.sigma
        S = self.C + self.sigma * np.einsum("k,kij->ij", Axb, self.A)
        return Axb, S

    def cost(self, Y):
        Axb, _ = self.parts(Y)
        return float(np.einsum("ij,ip,jp->", self.C, Y, Y)) + 0.5 * self.sigma * float(Axb @ Axb)

    def grad(self, Y):
        _, S = self.parts(Y)
        eG = 2.0 * S @ Y
        if self.kind == "unitdiag":
            return eG - Y * np.sum(Y * eG, axis=1, keepdims=True)
        if self.kind == "unittrace":
            return eG - float(np.sum(eG * Y)) * Y
        return eG

    def hess(self, Y, U):
        _, S = self.parts(Y)
        w = np.einsum("kij,ip,jp->k", self.A, U, Y)
        eH = 2.0 * S @ U + 4.0 * self.sigma * np.einsum("k,kij,jp->ip", w, self.A, Y)
        eG = 2.0 * S @ Y
        if self.kind == "unitdiag":
            return eH - Y * np.sum(Y * eH, axis=1, keepdims=True) - U * np.sum(Y * eG, axis=1, keepdims=True)
        if self.kind == "unittrace":
            return eH - float(np.sum(eH * Y)) * Y - float(np.sum(eG * Y)) * U
        return eH


def oracle_problem(kind, At, b, c, n, p, y, sigma):
    from oracle import manisdp_ref as R
    cls = {"unitdiag": R._UnitDiagProblem, "unittrace": R._UnitTraceProblem, "generic": R._GenericProblem}[kind]
    prob = cls(At, b, c, n, p)
    prob.y, prob.sigma = np.asarray(y, dtype=np.float64), float(sigma)
    return prob


def point(kind, rng, n, p):
    Y = rng.standard_normal((n, p))
    if kind == "unitdiag":
        return Y / np.linalg.norm(Y, axis=1, keepdims=True)
    if kind == "unittrace":
        return Y / np.linalg.norm(Y)
    return Y


def tangent(kind, Y, U):
    if kind == "unitdiag":
        return U - Y * np.sum(Y * U, axis=1, keepdims=True)
    if kind == "unittrace":
        return U - float(np.sum(Y * U)) * Y
    return U


def evaluate(prob, Y, U):
    """(f, G, H) of an oracle problem at Y in the call order the closures need."""
    f = prob.cost(Y)
    G = prob.grad(Y)
    return f, G, prob.hess(Y, U)
