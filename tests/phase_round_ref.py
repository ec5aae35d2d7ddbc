"""NumPy restatement of msdp_round_phases (Handle.round_phases): rounding of the complex unit-diagonal factor to the unit circle
(M = 0) or to the M-th roots of unity, the values, and the Gauss-Seidel local search -- the same table, the same tie rules, the
same row order as the device, all 64 lanes of every word side by side.  Besides the results it returns the smallest decision
margins it met, so that a test can tell whether a device that sums in another order (or with fma) must take the same decisions.

Everything is kept as separate real and imaginary arrays of one dtype, so that the same code runs in numpy.longdouble."""
import math

import numpy as np
import scipy.sparse as sp


def table(M):
    """c_k = (cos, sin)(2 pi k / M) as the library builds it: the angle is ((2 * pi) * k) / M in double, through the C library's
    cos / sin (math.cos / math.sin); exactly (1, 0), (0, 1), (-1, 0), (0, -1) where 4 k is a multiple of M.  Returns (M, 2)."""
    exact = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
    t = np.zeros((M, 2))
    for k in range(M):
        if (4 * k) % M == 0:
            t[k] = exact[4 * k // M]
        else:
            a = ((2.0 * math.pi) * float(k)) / float(M)
            t[k] = (math.cos(a), math.sin(a))
    return t


def _rows(C, dtype):
    C = sp.csr_matrix(C)
    C.sort_indices()
    rp, ci = C.indptr, C.indices
    vx, vy = C.data.real.astype(dtype), C.data.imag.astype(dtype)
    return [(ci[rp[i]:rp[i + 1]], vx[rp[i]:rp[i + 1], None], vy[rp[i]:rp[i + 1], None]) for i in range(C.shape[0])]


def _row_sum(row, i, Zx, Zy, skip_diag):
    """sum_j C_ij z_j over the stored entries of row i in order (the diagonal left out when asked), for every lane."""
    cols, cx, cy = row
    if skip_diag:
        keep = cols != i
        cols, cx, cy = cols[keep], cx[keep], cy[keep]
    zx, zy = Zx[cols], Zy[cols]
    return (cx * zx - cy * zy).sum(axis=0), (cx * zy + cy * zx).sum(axis=0)


def values(rows, Zx, Zy):
    """val_t = sum_i Re(conj(z_i) sum_j C_ij z_j), diagonal included, rows added in index order."""
    acc = np.zeros(Zx.shape[1], dtype=Zx.dtype)
    for i, row in enumerate(rows):
        sx, sy = _row_sum(row, i, Zx, Zy, False)
        acc = acc + (Zx[i] * sx + Zy[i] * sy)
    return acc


def _two_best(d, largest):
    """Per lane of d (M x T): index of the best entry (the lowest index at a tie) and the gap to the second best."""
    k = np.argmax(d, axis=0) if largest else np.argmin(d, axis=0)
    s = np.sort(d, axis=0)
    gap = (s[-1] - s[-2]) if largest else (s[1] - s[0])
    return k, gap


def round_phases(C, Y, R, M=0, sweeps=0, dtype=np.float64, trace=False):
    """The restatement.  C: n x n Hermitian sparse; Y: n x p complex; R: T x p complex, T a multiple of 64.  Returns a dict:
    phases (T/64, n, 64) complex, k (T/64, n, 64) int32 or None, values0, values, info (2, T/64), best, z, kbest,
    margin_round / scale_round (M = 0: the smallest |w|; M >= 2: the smallest gap between the best and the second-best
    candidate; the scale is the largest |w|), margin_sweep / scale_sweep (the smallest non-zero |cand_k* - cur| and the smallest
    best / second-best gap met in the sweeps, inf when there was none; the scale is the largest |s_i| met), and with trace the
    values after every sweep (trace[0]: after the rounding)."""
    Y = np.asarray(Y, dtype=np.complex128)
    R = np.asarray(R, dtype=np.complex128)
    n, p = Y.shape
    T = R.shape[0]
    assert T % 64 == 0 and R.shape[1] == p
    W = T // 64
    rows = _rows(C, dtype)
    tab = table(M).astype(dtype) if M else None
    Yx, Yy, Rx, Ry = (a.astype(dtype) for a in (Y.real, Y.imag, R.real, R.imag))
    wx, wy = np.zeros((n, T), dtype=dtype), np.zeros((n, T), dtype=dtype)
    for a in range(p):                                         # w = sum_a Y_ia R_ta, ascending a, no conjugate
        wx = wx + Yx[:, a:a + 1] * Rx[None, :, a]
        wx = wx - Yy[:, a:a + 1] * Ry[None, :, a]
        wy = wy + Yx[:, a:a + 1] * Ry[None, :, a]
        wy = wy + Yy[:, a:a + 1] * Rx[None, :, a]
    mod = np.sqrt(wx * wx + wy * wy)
    scale_round = float(mod.max())
    K = None
    if M == 0:
        margin_round = float(mod.min())
        ok = mod != 0
        safe = np.where(ok, mod, 1)
        Zx, Zy = np.where(ok, wx / safe, 1).astype(dtype), np.where(ok, wy / safe, 0).astype(dtype)
    else:
        d = tab[:, 0, None, None] * wx[None] + tab[:, 1, None, None] * wy[None]
        K, gap = _two_best(d.reshape(M, -1), True)
        K = K.reshape(n, T)
        margin_round = float(gap.min())
        Zx, Zy = tab[K, 0], tab[K, 1]
    values0 = values(rows, Zx, Zy)
    tr = [values0.copy()]
    info = np.zeros((2, W), dtype=np.int32)
    margin_sweep, scale_sweep = np.inf, 0.0
    done = np.zeros(W, dtype=bool)                             # M >= 2: a word stops after a sweep of its own without a change
    for s in range(int(sweeps)):
        if M and done.all():
            break
        changes = np.zeros(T, dtype=np.int64)
        for i, row in enumerate(rows):
            sx, sy = _row_sum(row, i, Zx, Zy, True)
            m2 = sx * sx + sy * sy
            scale_sweep = max(scale_sweep, float(np.sqrt(m2.max())))
            if M == 0:
                ok = m2 != 0
                m = np.sqrt(np.where(ok, m2, 1))
                Zx[i] = np.where(ok, -sx / m, Zx[i])
                Zy[i] = np.where(ok, -sy / m, Zy[i])
                continue
            cur = Zx[i] * sx + Zy[i] * sy
            cand = tab[:, 0, None] * sx[None] + tab[:, 1, None] * sy[None]
            kb, gap = _two_best(cand, False)
            best = cand[kb, np.arange(T)]
            live = m2 != 0                                     # (s = 0: every candidate equals cur, nothing to decide)
            if live.any():
                margin_sweep = min(margin_sweep, float(gap[live].min()))
                diff = np.abs(best - cur)[live]
                if (diff != 0).any():
                    margin_sweep = min(margin_sweep, float(diff[diff != 0].min()))
            ch = best < cur
            Zx[i] = np.where(ch, tab[kb, 0], Zx[i])
            Zy[i] = np.where(ch, tab[kb, 1], Zy[i])
            K[i] = np.where(ch, kb, K[i])
            changes += ch
        if trace:
            tr.append(values(rows, Zx, Zy))
        for w in range(W):
            if M == 0 or not done[w]:
                info[0, w] += 1
                info[1, w] = 0 if M == 0 else int(changes[64 * w:64 * w + 64].sum())
                done[w] = M != 0 and info[1, w] == 0
    vals = values(rows, Zx, Zy) if sweeps > 0 else values0.copy()
    best_t = int(np.argmin(vals))                              # the lowest index wins a tie
    Z = (Zx.astype(np.float64) + 1j * Zy.astype(np.float64))
    lay = lambda A: np.ascontiguousarray(A.reshape(n, W, 64).transpose(1, 0, 2))
    out = {"phases": lay(Z), "k": lay(K).astype(np.int32) if M else None, "values0": values0, "values": vals, "info": info,
           "best": best_t, "z": Z[:, best_t].copy(), "kbest": K[:, best_t].astype(np.int32) if M else None,
           "margin_round": margin_round, "scale_round": scale_round, "margin_sweep": margin_sweep, "scale_sweep": scale_sweep}
    if trace:
        out["trace"] = tr
    return out


def host_values(C, phases):
    """The values of a (T/64, n, 64) array of phases in plain complex algebra: a (T,) array."""
    Wn, n, _ = phases.shape
    Z = phases.transpose(1, 0, 2).reshape(n, Wn * 64)
    return np.real(np.sum(np.conj(Z) * (sp.csr_matrix(C) @ Z), axis=0))


# ------------------------------------------------------------------ the inputs the GPU tests and the host test share
def inputs(n, p, T, seed):
    """A point Y (n x p complex, unit rows) and the rows R (T x p complex) of a rounding, Gaussian, from one generator."""
    g = np.random.default_rng(seed)
    Y = g.standard_normal((n, p)) + 1j * g.standard_normal((n, p))
    Y /= np.sqrt(np.sum(np.abs(Y) ** 2, axis=1, keepdims=True))
    R = g.standard_normal((T, p)) + 1j * g.standard_normal((T, p))
    return np.ascontiguousarray(Y), np.ascontiguousarray(R)


def generic_instance(C, seed=5):
    """The pattern of C with generic values: entry (i, j), i < j, multiplied by (1 + 0.2 u) exp(0.7 i v) with u, v uniform in
    (-1, 1), entry (j, i) its conjugate, the diagonal multiplied by (1 + 0.2 u).  With entries in Z/4 and the 8th roots of unity
    the candidates of the local search tie exactly (s_i lies in Z[zeta_8] / 4, and so do the bisectors c_k + c_k+1), which no
    choice of seed avoids; generic values have no such ties."""
    A = sp.coo_matrix(C)
    g = np.random.default_rng(seed)
    lo, hi = np.minimum(A.row, A.col), np.maximum(A.row, A.col)
    key = lo.astype(np.int64) * A.shape[0] + hi
    _, inv = np.unique(key, return_inverse=True)
    f = ((1.0 + 0.2 * g.uniform(-1, 1, inv.max() + 1)) * np.exp(0.7j * g.uniform(-1, 1, inv.max() + 1)))[inv]
    f = np.where(A.row < A.col, f, np.where(A.row > A.col, np.conj(f), np.abs(f)))
    G = sp.csr_matrix((A.data * f, (A.row, A.col)), shape=A.shape)
    G.sort_indices()
    assert abs(G - G.conj().T).nnz == 0 and np.all(G.diagonal().imag == 0)
    return G


# widths: 1, 2, both sides of the register threshold (4 | 5) and of the LDS tile (32 | 33), and 35
EXACT_CASES = (                 # (storage, n, T, p, M, seed): table exact, entries in Z/4 -- every sum of sweeps and values exact
    ("grid", 203, 64, 1, 2, 11), ("hub", 203, 128, 2, 4, 12), ("grid", 1031, 64, 4, 4, 13), ("hub", 1031, 128, 5, 2, 14),
    ("hub", 203, 64, 32, 4, 15), ("grid", 203, 128, 33, 2, 16), ("hub", 1031, 64, 35, 4, 17))
EXACT_SWEEPS = (0, 1, 50)
REAL_CASES = (("grid", 203, 64, 3, 21), ("hub", 1031, 128, 9, 22))          # (storage, n, T, p, seed): B = 0, real point and R, M = 2
TOL_CASES = (("grid", 203, 64, 2, 31), ("hub", 1031, 128, 5, 34), ("hub", 203, 128, 33, 33))   # (storage, n, T, p, seed): M = 0 and M = 8
CIRCLE_SWEEPS = (1, 3)
M8_SWEEPS = 50
MARGIN_REL = 1e-9


# ------------------------------------------------------------------ the solves of tests/test_gpu_phase_round.py
_SOLVES = {}


def solve_instance(name):
    """"sync": phase_synchronization(203, 8, 1.0) -- hermitian_ref.solve ends at rank 1; "mpsk": mpsk_synchronization(203, 8, 0.5,
    M = 4); "sync3": phase_synchronization(203, 8, 3.0), whose solve takes two outer iterations and ends at rank 4, so that the
    re-shaping runs.  All from default_rng(7), start point of width 2 from default_rng(1).  Returns a dict: C, z (planted), M, Y0,
    and obj / data / Y of hermitian_ref.solve."""
    if name not in _SOLVES:
        import hermitian_ref as HR
        from manisdp_matlab_amd import problems
        g = np.random.default_rng(7)
        if name == "mpsk":
            C, z = problems.mpsk_synchronization(203, 8, 0.5, 4, g)
        else:
            C, z = problems.phase_synchronization(203, 8, 1.0 if name == "sync" else 3.0, g)
        g = np.random.default_rng(1)
        Y0 = g.standard_normal((203, 2)) + 1j * g.standard_normal((203, 2))
        Y0 /= np.sqrt(np.sum(np.abs(Y0) ** 2, axis=1, keepdims=True))
        Y, obj, data = HR.solve(C, Y0)
        _SOLVES[name] = dict(C=C, z=z, M=4 if name == "mpsk" else 0, Y0=np.ascontiguousarray(Y0), Y=Y, obj=obj, data=data)
    return _SOLVES[name]
