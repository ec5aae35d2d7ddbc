"""Symmetric matrices whose spectrum is known by construction, for tests of the saddle escape (msdp_escape_eigs, _matrix,
_dual) on prescribed spectra; pinned on the CPU by tests/test_escape_spectra_host.py.  Nothing here touches the GPU.

`build(n, lam, seed)` returns S = H D H' with D = diag(sort(lam)) and H = H1 H2 H3 a product of three Householder reflectors
I - 2uu' with seeded unit vectors u: O(n^2) work, no eigen-solver involved.  The reference spectrum is the prescribed `lam`
itself and the exact eigenvectors are the columns H e_i; tests/test_escape_spectra_host.py shows that LAPACK on S reproduces
`lam` to 1e-12 * scale, four digits below the tightest tolerance of the escape tests (1e-8 * scale on lambda_min).

`sparse_copies(t, base, seed)` is the block-diagonal sparse cost matrix of t disjoint copies of a small weighted graph.  With every
row of the factor equal to e_1, z = C*1 and S = C - diag(C*1) is minus the graph Laplacian of the t copies: every eigenvalue of one
copy (LAPACK on its 40 to 60 rows) appears t times or more, the kernel has dimension t.

`spectrum(name, n)` is the catalogue of named spectra."""
import numpy as np

CATALOGUE = ["posdef", "negdef", "mult5", "mult12", "cluster", "cluster_tight", "three_distinct", "scalar", "zero", "kernel_psd",
             "kernel_hidden", "shift_pos", "shift_neg", "graded", "tiny", "huge"]
# smallest order at which an entry has all its prescribed values (and, where it names a "rest", one value or more of it)
MIN_ORDER = {"posdef": 1, "negdef": 1, "scalar": 1, "zero": 1, "shift_pos": 1, "shift_neg": 1, "three_distinct": 3, "mult5": 7,
             "tiny": 7, "huge": 7, "cluster": 10, "cluster_tight": 10, "graded": 12, "kernel_psd": 12, "kernel_hidden": 13,
             "mult12": 14}
# entries whose bottom is one multiple (or numerically multiple) eigenvalue: returned vectors must lie in its eigenspace
MULTIPLE_BOTTOM = {"mult5": 5, "mult12": 12, "cluster_tight": 8, "tiny": 5, "huge": 5}


def _spread(lo, hi, r):
    """r values over [lo, hi], both ends included (the midpoint for r = 1)."""
    return np.linspace(lo, hi, r) if r > 1 else np.full(r, 0.5 * (lo + hi))


def spectrum(name, n):
    """The n prescribed eigenvalues of catalogue entry `name`, ascending."""
    if n < MIN_ORDER[name]:
        raise ValueError(f"{name} needs order >= {MIN_ORDER[name]}")
    if name == "posdef":
        lam = _spread(1.0, 2.0, n)
    elif name == "negdef":
        lam = _spread(-2.0, -1.0, n)
    elif name in ("mult5", "tiny", "huge"):
        lam = np.concatenate([np.full(5, -1.0), _spread(1.0, 2.0, n - 5)])
        lam = lam * {"mult5": 1.0, "tiny": 1e-6, "huge": 1e6}[name]
    elif name == "mult12":
        lam = np.concatenate([np.full(12, -1.0), _spread(1.0, 2.0, n - 12)])
    elif name == "cluster":
        lam = np.concatenate([-1.0 + 1e-7 * np.arange(8), _spread(0.5, 2.0, n - 8)])
    elif name == "cluster_tight":
        lam = np.concatenate([-1.0 + 1e-11 * np.arange(8), _spread(0.5, 2.0, n - 8)])
    elif name == "three_distinct":
        third = n // 3
        lam = np.concatenate([np.full(third, -1.0), np.full(third, 0.0), np.full(n - 2 * third, 3.0)])
    elif name == "scalar":
        lam = np.full(n, 2.0)
    elif name == "zero":
        lam = np.zeros(n)
    elif name == "kernel_psd":
        lam = np.concatenate([np.zeros(10), np.logspace(-3.0, 0.0, n - 10)])
    elif name == "kernel_hidden":
        lam = np.concatenate([[-1e-6], np.zeros(10), np.logspace(-3.0, 0.0, n - 11)])
    elif name == "shift_pos":
        lam = _spread(100.0, 100.1, n)
    elif name == "shift_neg":
        lam = _spread(-100.1, -100.0, n)
    elif name == "graded":
        lam = np.concatenate([-(10.0 ** -np.arange(10)), _spread(1.0, 2.0, n - 10)])
    else:
        raise KeyError(name)
    return np.sort(lam.astype(np.float64))


def reflectors(n, seed):
    """The three seeded unit vectors u of H = (I - 2 u1 u1')(I - 2 u2 u2')(I - 2 u3 u3')."""
    rng = np.random.default_rng(seed)
    us = rng.standard_normal((3, n))
    return us / np.linalg.norm(us, axis=1, keepdims=True)


def apply_h(us, X):
    """H X for the reflector product H = H1 H2 H3 (X: n x c)."""
    X = np.array(X, dtype=np.float64, copy=True)
    for u in us[::-1]:
        X -= 2.0 * np.outer(u, u @ X)
    return X


def build(n, lam, seed, ncols=None):
    """(S, lam_sorted, U): S = H diag(lam_sorted) H', exactly symmetric; U = the first `ncols` columns of H (all n when None), the
    exact eigenvectors of lam_sorted[:ncols]."""
    lam = np.sort(np.asarray(lam, dtype=np.float64))
    assert lam.shape == (n,)
    us = reflectors(n, seed)
    S = np.diag(lam)
    for u in us[::-1]:                         # S <- (I - 2uu') S (I - 2uu'), innermost reflector first
        Su = S @ u
        uSu = float(u @ Su)
        S -= 2.0 * np.outer(u, Su)
        S -= 2.0 * np.outer(Su, u)
        S += (4.0 * uSu) * np.outer(u, u)
    S = 0.5 * (S + S.T)
    nc = n if ncols is None else min(int(ncols), n)
    E = np.zeros((n, nc))
    E[np.arange(nc), np.arange(nc)] = 1.0
    return S, lam, apply_h(us, E)


def base_graph(base, seed):
    """Symmetric weighted adjacency matrix (dense, zero diagonal) of a connected base graph with seeded weights in [0.5, 1.5]:
    "cycle" = a cycle of 47 vertices, "torus" = the 6 x 8 toroidal grid (48 vertices)."""
    rng = np.random.default_rng(seed)
    if base == "cycle":
        nb = 47
        edges = [(i, (i + 1) % nb) for i in range(nb)]
    elif base == "torus":
        r, c = 6, 8
        nb = r * c
        edges = []
        for i in range(r):
            for j in range(c):
                edges.append((i * c + j, i * c + (j + 1) % c))
                edges.append((i * c + j, ((i + 1) % r) * c + j))
    else:
        raise KeyError(base)
    W = np.zeros((nb, nb))
    for (i, j) in edges:
        W[i, j] = W[j, i] = 0.5 + rng.random()
    return W


def sparse_copies(t, base, seed=0):
    """(C, w): C = the block-diagonal sparse matrix of t copies of base_graph(base, seed) (order t * nb); w = the ascending spectrum
    of S = C - diag(C*1), the eigenvalues of one copy's W - diag(W*1) (LAPACK) repeated t times."""
    import scipy.sparse as sp
    W = base_graph(base, seed)
    C = sp.block_diag([sp.csr_matrix(W)] * t, format="csr")
    wb = np.linalg.eigvalsh(W - np.diag(W.sum(axis=1)))
    return C, np.sort(np.repeat(wb, t))
