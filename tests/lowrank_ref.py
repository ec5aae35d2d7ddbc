"""NumPy restatement of the sparse-plus-low-rank cost kind C = Cs + V diag(s) V' (msdp_create_onlyunitdiag_csc_lowrank,
problems.SparsePlusLowRank): cost, gradient and Hessian-vector product of ManiSDP_onlyunitdiag.m:117-130 in the split form the
device uses (sparse product plus the two skinny products T = diag(s) V' U and V T), and msdp_round_hyperplane with the low-rank
term -- values x' Cs x + sum_k s_k (V_k' x)^2 and the 1-opt search with t_k = V_k' x carried per trial.  tests/round_ref.py is
imported for what does not change (signs, packing, the rows of Cs without their diagonal).

The instances of tests/test_gpu_lowrank.py are generated here from fixed integer tables (nothing is committed): every entry of
Cs, V and s is a multiple of 1/4, so that every sum of the rounding is exact in fp64 in any order."""
import numpy as np
import scipy.sparse as sp

import round_ref

N_GRID = (203, 1031)                      # neither a multiple of 64 nor of a workgroup's chunk; 203 leaves workgroups without rows
P_GRID = (1, 2, 5, 16, 17, 33, 70)        # every <LPR, NCH> instance of the row kernels up to <64, 2>, odd widths (a pad column)
P_WIDE = (130, 260)                       # rows wider than 128 columns: T read in place instead of from LDS (<64, 2>, <64, 4>)
Q_GRID = (1, 3, 8)
STORAGES = ("grid", "hub")                # four entries per row (fixed-width storage) / rows of more than 64 entries (CSR)
ROUND_T = (64, 192)
ROUND_P = (3, 17)

_W_TABLE = (1, -2, 3, -1, 2, -3, 1, 1, -1, 2, -2, 3, -3)                           # edge weights, in quarters (never 0)
_V_TABLE = (3, -5, 0, 8, -1, 2, -8, 4, 1, -3, 6, -2, 0, 7, -4, 5, -6)              # entries of V, in quarters (|.| <= 2)
_S_TABLE = {1: (-3,), 3: (2, -3, 4), 8: (1, -2, 3, -1, 4, -4, 2, -3)}                # s, in quarters; q = 3 and 8: mixed signs


def grid_cs(n):
    """A toroidal grid closed with a twist: vertex i is joined to i +- 1 and i +- a (mod n), a = 7 for n = 203 (the 29 x 7
    torus) and the like for a prime n -- four entries in every row, weights +-1/4, +-1/2, +-3/4 from the table."""
    a = 7 if n % 7 == 0 else 32
    i = np.arange(n)
    rows, cols, vals = [], [], []
    for d, k in ((1, 3), (a, 5)):
        w = np.array([_W_TABLE[(k * int(t) + d) % len(_W_TABLE)] for t in i]) / 4.0
        j = (i + d) % n
        rows += [i, j]; cols += [j, i]; vals += [w, w]
    C = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    C.sum_duplicates()
    C.sort_indices()
    assert np.all(np.diff(C.indptr) == 4) and np.all(C.data != 0)
    return C


def hub_cs(n):
    """The grid plus three hubs (vertices 0, 5 and n - 1) joined to every 3rd, 2nd and 7th vertex, and a diagonal entry on every
    11th vertex: rows of 340 / 500 / 140-odd entries at n = 1031 and of 70 / 100 / 30-odd at n = 203 -- CSR storage, and rows that
    need the second batch of 64 entries of the rounding kernels."""
    C = grid_cs(n).tolil()
    for hub, step, k in ((0, 3, 2), (5, 2, 7), (n - 1, 7, 4)):
        for j in range(1, n, step):
            if j == hub:
                continue
            w = _W_TABLE[(k * j + hub) % len(_W_TABLE)] / 4.0
            C[hub, j] = w
            C[j, hub] = w
    for i in range(0, n, 11):
        C[i, i] = _W_TABLE[i % len(_W_TABLE)] / 4.0
    C = C.tocsr()
    C.sort_indices()
    assert np.diff(C.indptr).max() > 64 and abs(C - C.T).nnz == 0
    return C


def lowrank_term(n, q):
    V = np.array([[_V_TABLE[(i * (k + 2) + 3 * k) % len(_V_TABLE)] for k in range(q)] for i in range(n)], dtype=np.float64) / 4.0
    return V, np.array(_S_TABLE[q], dtype=np.float64) / 4.0


_CACHE = {}


def instance(storage, n, q):
    """(problems.SparsePlusLowRank, its dense equivalent) of the table; built once."""
    key = (storage, n, q)
    if key not in _CACHE:
        from manisdp_matlab_amd import problems
        V, s = lowrank_term(n, q)
        C = problems.SparsePlusLowRank(grid_cs(n) if storage == "grid" else hub_cs(n), V, s)
        _CACHE[key] = (C, C.toarray())
    return _CACHE[key]


def table_point(n, p):
    return round_ref.table_point(n, p)


def table_direction(n, p):
    return np.random.default_rng(300 + p).standard_normal((n, p))


def planted_partition(n=300, p_in=0.10, p_out=0.02, seed=4):
    """Adjacency matrix of a planted two-community graph (the first n/2 vertices against the rest) and its labels."""
    rng = np.random.default_rng(seed)
    labels = np.where(np.arange(n) < n // 2, 1.0, -1.0)
    same = labels[:, None] == labels[None, :]
    U = rng.random((n, n))
    A = np.triu((U < np.where(same, p_in, p_out)).astype(np.float64), 1)
    return sp.csr_matrix(A + A.T), labels


# ------------------------------------------------------------------ derivatives, split form
def apply_c(Cs, V, s, X):
    """C X as the device forms it: the sparse product plus V T with T = diag(s) V' X."""
    return Cs @ X + V @ (s[:, None] * (V.T @ X))


def cost(Cs, V, s, Y):
    return 0.5 * float(np.sum(apply_c(Cs, V, s, Y) * Y))                     # ManiSDP_onlyunitdiag.m:118-120


def get_z(Cs, V, s, Y):
    return np.sum(apply_c(Cs, V, s, Y) * Y, axis=1)                          # :119 (eG)


def rgrad(Cs, V, s, Y):
    YC = apply_c(Cs, V, s, Y)
    return YC - Y * np.sum(YC * Y, axis=1, keepdims=True)                    # :124


def hessvec(Cs, V, s, Y, U):
    eG = np.sum(apply_c(Cs, V, s, Y) * Y, axis=1, keepdims=True)
    eH = apply_c(Cs, V, s, U)                                                # :128
    return eH - Y * np.sum(Y * eH, axis=1, keepdims=True) - U * eG           # :129


# ------------------------------------------------------------------ rounding
def values(Cs, V, s, X):
    """x' C x of every row x of X: the sparse part as round_ref.values, plus sum_k s_k (V_k' x)^2 in k order."""
    out = round_ref.values(Cs, X)
    Tm = X @ V                                                               # trials x q
    for k in range(V.shape[1]):
        out = out + s[k] * (Tm[:, k] * Tm[:, k])
    return out


def one_opt(Cs, V, s, X, sweeps):
    """round_ref.one_opt with the low-rank term: t_k = V_k' x per trial, formed at the start of every sweep;
    x_i s_i = x_i (sparse sum over j != i) + sum_k s_k V_ik (x_i t_k - V_ik); a flip takes t_k -= 2 V_ik x_i(old)."""
    T, n = X.shape
    W = T // 64
    rows = round_ref._rows_without_diagonal(Cs)
    Xt = np.array(X.T, dtype=np.float64, order="C")
    info = np.zeros((2, W), dtype=np.int32)
    active = np.ones(W, dtype=bool)
    for _ in range(int(sweeps)):
        if not active.any():
            break
        idx = np.nonzero(np.repeat(active, 64))[0]
        Xa = Xt[:, idx]
        Tm = V.T @ Xa                                                        # q x trials
        flips = np.zeros(len(idx), dtype=np.int64)
        for i in range(n):
            cols, vals = rows[i]
            xs = Xa[i] * (vals @ Xa[cols] if len(cols) else np.zeros(len(idx)))
            for k in range(V.shape[1]):
                xs = xs + (s[k] * V[i, k]) * (Xa[i] * Tm[k] - V[i, k])
            f = xs > 0
            Tm[:, f] -= 2.0 * V[i][:, None] * Xa[i, f][None, :]
            Xa[i, f] = -Xa[i, f]
            flips += f
        Xt[:, idx] = Xa
        per_word = flips.reshape(-1, 64).sum(axis=1)
        info[0, active] += 1
        info[1, active] = per_word
        active[np.nonzero(active)[0][per_word == 0]] = False
    return np.ascontiguousarray(Xt.T), info


def round_hyperplane(C, Y, R, sweeps=0):
    """What Handle.round_hyperplane(R, sweeps, masks=True) returns on a sparse-plus-low-rank handle (C: a
    problems.SparsePlusLowRank), from NumPy."""
    Cs, V, s = C.Cs, C.V, C.s
    X0, _ = round_ref.signs(Y, R)
    values0 = values(Cs, V, s, X0)
    X, info = one_opt(Cs, V, s, X0, sweeps) if sweeps else (X0, np.zeros((2, X0.shape[0] // 64), dtype=np.int32))
    vals = values(Cs, V, s, X) if sweeps else values0.copy()
    best = int(np.argmin(vals))
    return {"values0": values0, "values": vals, "info": info, "best": best, "x": X[best].astype(np.int8), "masks": round_ref.pack(X)}


def modularity_value(A, x, gamma=1.0):
    """The modularity x' (A - gamma d d'/(2m)) x / (4m) of the two-community labelling x."""
    d = np.asarray(A.sum(axis=1)).ravel()
    two_m = d.sum()
    return float(x @ (A @ x) - gamma * (d @ x) ** 2 / two_m) / (2.0 * two_m)
