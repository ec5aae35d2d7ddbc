"""NumPy restatement of the per-block rule of msdp_block_reshape (ManiSDP_multiblock.m:109-147, ManiDSDP_multiblock.m:146-181), the
same rule in extended precision, and planted factors whose rank decision is unambiguous.

The rule, for a block of order n with factor Y (n x p), eigenvalues w (ascending) and bottom eigenvectors V (n x k) of S_i:
n < min_facsize: untouched.  Else, p > 1: G = Y'Y, e = sqrt(max(eig(G), 0)) descending, r = #{e >= theta e_1} (strict: >), at least 1;
r < p: Y <- Y Q(:, :r).  nne = max(min(#{w < 0}, delta), 1 if oblique else 0), 0 when p + nne > n.  mode 0: Y <- [Y, alpha V(:, :nne)],
rows scaled to unit norm on oblique blocks; mode 1: Y <- [Y, 0], U = [0, V(:, :nne)].

What is compared is invariant under the rotation and the signs an eigen-solver is free to choose: the counts, U (exactly) and
X = Y_new Y_new' = D (Y Q_r Q_r' Y' + alpha^2 V V') D, D the row normalisation of the oblique blocks (identity otherwise, and no
alpha term in mode 1).

Tolerance on X.  `reshape_block` (float64: LAPACK eigh, BLAS products) was measured against `reshape_block(..., extended=True)`
(numpy.longdouble, eps 1.1e-19: products in that format, eigen-decomposition of G by a cyclic Jacobi iteration carried to
off(G)^2 <= 1e-38 |G|^2) on every planted case the GPU tests use (generator seed 81) and the host test uses (seed 71) -- the
seven-block handle (orders 1, 2, 3, 63, 64, 65, 257, widths 1, 2, 8, 9, 32, 33, 64), the branch cases and the 300 blocks of orders
1 .. 64, each as a Euclidean and as an oblique block, both modes, (theta, strict) = (1e-2, 0) and (1e-3, 1).  Largest relative deviation
|X - X_ext|_F / |X_ext|_F seen: 1.62e-15 (a block of order 44, width 12; measured 2026-10-17); X_DEVIATION is that figure rounded up.
The uncut blocks of width 57 .. 64 (`wide_uncut_blocks`, added later) stay below it: 2.7e-16.
tests/test_block_reshape_host.py re-measures a part of the set (40 of the 300 blocks, the uncut block of width 64) and fails above X_DEVIATION.  X_TOL is ten times X_DEVIATION: the margin the block-eigs tests give LAPACK.
The planted spectra keep every discarded singular value at or below 1e-6 e_1, so the comparison does not depend on them
(they enter X with weight 1e-12)."""
import numpy as np

X_DEVIATION = 1.7e-15
X_TOL = 10 * X_DEVIATION


_JACOBI_CACHE = {}


def _jacobi_eigh(G):
    """Eigen-decomposition of a symmetric matrix in its own (extended) precision: cyclic Jacobi, ascending eigenvalues."""
    key = G.tobytes()
    if key in _JACOBI_CACHE:                                         # (the same block under another mode / rule: same G)
        return _JACOBI_CACHE[key]
    A = np.array(G, copy=True)
    p = A.shape[0]
    Q = np.eye(p, dtype=A.dtype)
    for _ in range(60):
        off = np.sum(A * A) - np.sum(np.diag(A) ** 2)
        if off <= A.dtype.type(1e-38) * np.sum(A * A):
            break
        for u in range(p - 1):
            for v in range(u + 1, p):
                if A[u, v] == 0:
                    continue
                tau = (A[v, v] - A[u, u]) / (2 * A[u, v])
                t = (1 if tau >= 0 else -1) / (abs(tau) + np.hypot(A.dtype.type(1), tau))
                c = 1 / np.sqrt(1 + t * t)
                s = t * c
                for M in (A, Q):
                    cu, cv = M[:, u].copy(), M[:, v].copy()
                    M[:, u], M[:, v] = c * cu - s * cv, s * cu + c * cv
                ru, rv = A[u, :].copy(), A[v, :].copy()
                A[u, :], A[v, :] = c * ru - s * rv, s * ru + c * rv
    order = np.argsort(np.diag(A))
    _JACOBI_CACHE[key] = (np.diag(A)[order], Q[:, order])
    return _JACOBI_CACHE[key]


def reshape_block(Y, w, V, *, theta, strict, delta, alpha, min_facsize, mode, oblique, extended=False):
    """The rule on one block.  Returns dict(p_out, r, nne, X, U, e): X = Y_new Y_new' (float64), U (n x p_out; zeros in mode 0),
    e = the singular values the rank decision saw (descending; None when no decomposition is made)."""
    ft = np.longdouble if extended else np.float64
    Y = np.asarray(Y, dtype=ft)
    V = np.asarray(V, dtype=ft)
    n, p = Y.shape
    if n < min_facsize:
        return dict(p_out=p, r=p, nne=0, X=np.asarray(Y @ Y.T, dtype=np.float64), U=np.zeros((n, p)), e=None)
    r, e, Yc = p, None, Y
    if p > 1:
        lam, Q = _jacobi_eigh(Y.T @ Y) if extended else np.linalg.eigh(Y.T @ Y)
        lam, Q = np.maximum(lam[::-1], 0), Q[:, ::-1]
        e = np.sqrt(lam)
        r = int(np.sum(e > ft(theta) * e[0])) if strict else int(np.sum(e >= ft(theta) * e[0]))
        r = max(r, 1)
        if r < p:
            Yc = Y @ Q[:, :r]
    pn = min(r, p)
    nne = max(min(int(np.sum(np.asarray(w) < 0)), delta), 1 if oblique else 0)
    if pn + nne > n:
        nne = 0
    Vn = V[:, :nne]
    X = Yc @ Yc.T
    U = np.zeros((n, pn + nne))
    if mode == 0:
        X = X + ft(alpha) ** 2 * (Vn @ Vn.T)
        if oblique:
            d = np.sqrt(np.diag(X))
            d = np.where(d > 0, d, 1)
            X = X / d[:, None] / d[None, :]
    else:
        U[:, pn:] = np.asarray(Vn, dtype=np.float64)
    return dict(p_out=pn + nne, r=r, nne=nne, X=np.asarray(X, dtype=np.float64), U=U, e=e)


def decision_margin(e, theta):
    """How far the rank decision is from its threshold: the least factor between theta e_1 and a singular value, over both sides."""
    cut = theta * e[0]
    above, below = e[e >= cut], e[e < cut]
    m = float(np.min(above) / cut) if cut > 0 else np.inf
    if below.size and np.max(below) > 0:
        m = min(m, float(cut / np.max(below)))
    return m


def planted(n, p, keep, rng, scale=1.0):
    """Y = A diag(s) B' (n x p) with min(n, p) singular values: `keep` of them in [0.2, 1] * scale, the others in
    [1e-8, 1e-6] * scale -- a factor 10 and more from theta e_1 on either side for theta in [1e-3, 2e-2]."""
    q = min(n, p)
    keep = max(1, min(keep, q))
    s = np.concatenate([[1.0], rng.uniform(0.2, 1.0, keep - 1), 10.0 ** rng.uniform(-8, -6, q - keep)]) * scale
    A, _ = np.linalg.qr(rng.standard_normal((n, q)))
    B, _ = np.linalg.qr(rng.standard_normal((p, q)))
    return np.ascontiguousarray((A * s) @ B.T)


def eigen_data(n, nneg, k, rng):
    """w (ascending, `nneg` negative values, none within 0.1 of zero) and V (n x k: orthonormal columns, zeros beyond column n)."""
    w = np.sort(np.concatenate([-rng.uniform(0.1, 1.0, min(nneg, n)), rng.uniform(0.1, 1.0, n - min(nneg, n))]))
    Vq, _ = np.linalg.qr(rng.standard_normal((n, min(n, k))))
    V = np.zeros((n, k))
    V[:, :Vq.shape[1]] = Vq
    return w, V


class Case:
    """One block of a planted call: order, width, the planted factor, its eigen-data, whether the block has unit diagonal."""

    def __init__(self, n, p, keep, nneg, k, rng, scale=1.0, Y=None):
        self.n, self.p = n, p
        self.Y = planted(n, p, keep, rng, scale) if Y is None else Y
        self.w, self.V = eigen_data(n, nneg, k, rng)


def seven_blocks(rng, k=8):
    """Orders 1, 2, 3, 63, 64, 65, 257 with the unequal widths 1, 2, 8, 9, 32, 33, 64 in one handle (order 3 carries width 8: a factor
    wider than its block, five exact zero singular values).  Kept ranks and negative counts vary."""
    spec = [(1, 1, 1, 0), (2, 2, 1, 1), (3, 8, 2, 0), (63, 9, 4, 3), (64, 32, 32, 12), (65, 33, 5, 0), (257, 64, 20, 2)]
    return [Case(n, p, keep, nneg, k, rng) for n, p, keep, nneg in spec]


def many_blocks(rng, count=300, k=8):
    """`count` blocks of orders 1 .. 64 (1, 2, 63 and 64 among them), widths up to min(order, 12)."""
    orders = [1, 2, 63, 64] + [int(v) for v in rng.integers(1, 65, size=count - 4)]
    out = []
    for n in orders:
        p = int(rng.integers(1, min(n, 12) + 1))
        out.append(Case(n, p, int(rng.integers(1, p + 1)), int(rng.integers(0, 12)), k, rng))
    return out


def wide_uncut_blocks(k=8):
    """Full-rank blocks of width 57, 60 and 64 with negative eigenvalues: uncut, and widened past column 64 (to 65, 68 and 72)."""
    rng = np.random.default_rng(86)
    return [Case(100, 57, 57, 8, k, rng), Case(90, 60, 60, 9, k, rng), Case(72, 64, 64, 11, k, rng)]


def branch_blocks(rng, k=8):
    """Every branch of the rule, by name -> Case (orders 6 .. 12; 'small' has order 1 < min_facsize = 2)."""
    c = {}
    c["small"] = Case(1, 1, 1, 3, k, rng)                                    # n < min_facsize: untouched
    c["p1"] = Case(9, 1, 1, 2, k, rng)                                       # p = 1: no cut
    c["zero"] = Case(8, 3, 1, 0, k, rng, Y=np.zeros((8, 3)))                 # zero block: e = 0
    c["nneg0"] = Case(10, 4, 2, 0, k, rng)                                   # no negative eigenvalue
    c["many"] = Case(12, 3, 3, 11, k, rng)                                   # nneg > delta
    c["full"] = Case(6, 6, 6, 4, k, rng)                                     # p + nne > n: nne = 0
    c["shrink"] = Case(12, 10, 2, 1, k, rng)
    return c
