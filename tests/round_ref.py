"""NumPy restatement of msdp_round_hyperplane (include/manisdp_hip.h): the signs x_t = sign(Y r_t) with sign(0) = +1, their
packing 64 trials per word, the values x' C x, and the sequential 1-opt local search -- rows in order, strict flip test, the 64
trials of a word sweeping together until a sweep of that word flips nothing.  The instances and the parameter grid of
tests/test_gpu_round.py live here too, so that tests/test_round_ref_host.py can check their precondition without a GPU."""
import numpy as np
import scipy.sparse as sp

P_GRID = (1, 2, 7, 32, 33, 40)
T_GRID = (64, 192)
P_SUBSET = (1, 7, 33)                     # G1 and G11: widths that take the register path, one LDS tile, and an odd row stride
INSTANCE_N = {"pair": 2, "torus": 65, "torus_hole": 65, "G11": 800, "G1": 800, "dense96": 96}
SPARSE = ("pair", "torus", "torus_hole", "G11", "G1")


def table():
    """Every (instance, n, p, T) of the GPU tests."""
    out = []
    for name, n in INSTANCE_N.items():
        for p in (P_SUBSET if name in ("G1", "G11") else P_GRID):
            for T in T_GRID:
                out.append((name, n, p, T))
    return out


def instance(name, golden_path=None):
    from manisdp_matlab_amd import problems
    if name == "pair":
        return sp.csr_matrix(np.array([[0.0, 0.25], [0.25, 0.0]]))
    if name in ("torus", "torus_hole"):
        C = problems.toroidal_grid_maxcut(5, 13, seed=3)
        if name == "torus_hole":                              # vertex 7 loses its row and column: an empty row
            C = C.tolil()
            C[7, :] = 0.0
            C[:, 7] = 0.0
            C = C.tocsr()
            C.eliminate_zeros()
            C.sort_indices()
        return C
    if name in ("G1", "G11"):
        return problems.maxcut_cost_matrix(golden_path(name + ".txt.gz"))
    if name == "dense96":
        return problems.dense_unitdiag_cost(96, seed=1)
    raise KeyError(name)


def table_point(n, p):
    Y = np.random.default_rng(100 + p).standard_normal((n, p))
    return np.ascontiguousarray(Y / np.sqrt(np.sum(Y * Y, axis=1, keepdims=True)))


def table_directions(T, p):
    return np.random.default_rng(200 + T).standard_normal((T, p))


def signs(Y, R):
    """X (trials x n, entries +1 / -1) and the dots they are the signs of."""
    D = R @ Y.T
    return np.where(D < 0, -1.0, 1.0), D


def pack(X):
    """M (trials/64 x n, uint64): bit t of M[w, i] is set when X[64 w + t, i] = -1."""
    T, n = X.shape
    assert T % 64 == 0
    neg = (X < 0).reshape(T // 64, 64, n).astype(np.uint64)
    return np.bitwise_or.reduce(neg << np.arange(64, dtype=np.uint64)[None, :, None], axis=1)


def unpack(M, T=None):
    W, n = M.shape
    bits = (M[:, None, :] >> np.arange(64, dtype=np.uint64)[None, :, None]) & np.uint64(1)
    X = 1.0 - 2.0 * bits.reshape(W * 64, n).astype(np.float64)
    return X if T is None else X[:T]


def values(C, X):
    """x' C x of every row x of X, the diagonal of C included."""
    return np.sum(X * (C @ X.T).T, axis=1)


def _rows_without_diagonal(C):
    n = C.shape[0]
    if sp.issparse(C):
        C = C.tocsr()
        out = []
        for i in range(n):
            cols = C.indices[C.indptr[i]:C.indptr[i + 1]]
            vals = C.data[C.indptr[i]:C.indptr[i + 1]]
            keep = cols != i
            out.append((cols[keep], vals[keep]))
        return out
    C = np.asarray(C)
    return [(np.delete(np.arange(n), i), np.delete(C[i], i)) for i in range(n)]


def one_opt(C, X, sweeps):
    """Up to `sweeps` Gauss-Seidel sweeps of 1-opt on every row of X: for i = 0 .. n-1 in order, s_i = sum_{j != i} C_ij x_j
    and x_i is flipped where x_i s_i > 0.  A word (64 consecutive trials) stops after a sweep of its own without a flip.
    Returns (X_final, info) with info[0, w] = sweeps word w ran and info[1, w] = flips of its last sweep."""
    T, n = X.shape
    W = T // 64
    rows = _rows_without_diagonal(C)
    Xt = np.array(X.T, dtype=np.float64, order="C")            # n x T: a row of it is x_i of all trials
    info = np.zeros((2, W), dtype=np.int32)
    active = np.ones(W, dtype=bool)
    for _ in range(int(sweeps)):
        if not active.any():
            break
        idx = np.nonzero(np.repeat(active, 64))[0]
        Xa = Xt[:, idx]
        flips = np.zeros(len(idx), dtype=np.int64)
        for i in range(n):
            cols, vals = rows[i]
            s = vals @ Xa[cols] if len(cols) else np.zeros(len(idx))
            f = Xa[i] * s > 0
            Xa[i, f] = -Xa[i, f]
            flips += f
        Xt[:, idx] = Xa
        per_word = flips.reshape(-1, 64).sum(axis=1)
        info[0, active] += 1
        info[1, active] = per_word
        active[np.nonzero(active)[0][per_word == 0]] = False
    return np.ascontiguousarray(Xt.T), info


def round_hyperplane(C, Y, R, sweeps=0):
    """What Handle.round_hyperplane(R, sweeps, masks=True) returns, from NumPy."""
    X0, _ = signs(Y, R)
    values0 = values(C, X0)
    X, info = one_opt(C, X0, sweeps) if sweeps else (X0, np.zeros((2, X0.shape[0] // 64), dtype=np.int32))
    vals = values(C, X) if sweeps else values0.copy()
    best = int(np.argmin(vals))                                # (the first of equal minima)
    return {"values0": values0, "values": vals, "info": info, "best": best, "x": X[best].astype(np.int8), "masks": pack(X)}


def reorder_bound(C):
    """nnz * 2^-52 * sum |C_ij|: bound on the difference of two summation orders of the nnz terms of x' C x."""
    A = np.abs(C.data) if sp.issparse(C) else np.abs(np.asarray(C)).ravel()
    return np.count_nonzero(A) * 2.0 ** -52 * float(A.sum())
