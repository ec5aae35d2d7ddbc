"""Host-only helpers of tests/test_gpu_block_eigs.py and tests/test_block_eigs_ref_host.py: the matrix families that are planted
as blocks of the dual slack, the high-precision eigenvalue reference, and the per-block assertions on what msdp_block_eigs
returns.  Nothing here touches the GPU.

References.  `mp_eigvals` is mpmath.eigsy at 40 digits on the exact binary entries of the block (or a closed form evaluated at 40
digits, or the sorted diagonal of a diagonal block, which is exact); `reference_eigvals` falls back to numpy.linalg.eigvalsh for the
cases whose order makes mpmath too slow.  tests/test_block_eigs_ref_host.py shows that LAPACK alone stays within one tenth of
the eigenvalue tolerance against mpmath on every family, so a GPU comparison against either measures the kernel.

Tolerances are those of tests/test_gpu_multiblock.py::test_block_eigs_match_lapack."""
import functools
import hashlib
from dataclasses import dataclass, field

import numpy as np

EIG_TOL = 1e-13          # |w - w_ref| <= EIG_TOL * n * scale
RES_TOL = 1e-12          # |S V - V diag(w)|_max <= RES_TOL * n * scale
ORTH_TOL = 1e-12         # |V'V - I|_max
CLUSTER_GAP = 1e-4       # the bottom set J grows while the next reference eigenvalue is within CLUSTER_GAP * scale
ORDERS = [63, 65, 127, 129, 255, 256]            # both sides of 64 and 128, and the two largest orders the solver takes
MP_DIGITS = 40


@dataclass
class Case:
    name: str
    S: np.ndarray                                # the symmetric block to plant
    family: int
    mp: bool = False                             # reference from mpmath (else LAPACK)
    closed: object = None                        # callable -> list of mpmath values (closed-form spectrum), or "diag"
    floor: bool = True                           # scale = max(1, |w|_max); False: scale = |w|_max (the scaled copies)
    nneg: int = -1                               # exact count of w < 0 (family 2), -1: not asserted
    nzero: int = 0                               # size of the zero cluster at the bottom (family 1)
    vacuous_ok: bool = False                     # the bottom set J may grow to the whole block
    parts: list = field(default_factory=list)    # direct sums: orders of the summands (mpmath runs on each summand)

    @property
    def n(self):
        return self.S.shape[0]


# ------------------------------------------------------------------------------------------------------------- generators
def _orth(n, rng):
    Q, R = np.linalg.qr(rng.standard_normal((n, n)))
    return Q * np.sign(np.diag(R))


def dense(lam, rng):
    """Q diag(lam) Q' with Q from the QR of a Gaussian matrix, symmetrised."""
    lam = np.asarray(lam, dtype=np.float64)
    Q = _orth(lam.size, rng)
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def upper_part(r, rng):
    """r eigenvalues in [0.5, 2], the largest exactly 2: an even grid with a jitter of a fifth of its step, so neighbours stay
    at least 0.6 steps (>= 3.5e-3 up to order 256) apart -- far more than CLUSTER_GAP * scale = 2e-4, which keeps the
    subspace check of families 1 to 4 from growing into this part."""
    if r <= 0:
        return np.zeros(0)
    if r == 1:
        return np.array([2.0])
    step = 1.5 / (r - 1)
    lam = np.linspace(0.5, 2.0, r) + step * rng.uniform(-0.2, 0.2, r)
    lam[0], lam[-1] = 0.5, 2.0
    return lam


def deficiencies(n):
    return sorted({d for d in (1, 3, 8, 9, n // 2, n - 1) if 1 <= d <= n - 1})


def family1(orders, rng, mp_orders=()):
    """Rank-deficient PSD: n - r exact zeros below r eigenvalues in [0.5, 2] -- the slack near an optimum."""
    out = []
    for n in orders:
        for nz in deficiencies(n):
            lam = np.concatenate([np.zeros(nz), upper_part(n - nz, rng)])
            out.append(Case(f"f1-n{n}-z{nz}", dense(lam, rng), 1, nzero=nz, mp=(n in mp_orders and nz == 8)))
    return out


def family2(orders, rng, mp_orders=()):
    """A few eigenvalues at -d and +d (d = 1e-9 and 1e-6 times the scale 2) below the part in [0.5, 2]; no exact zeros."""
    out = []
    for n in orders:
        for d in (2e-9, 2e-6):
            for nneg, npos in ((1, 2), (3, 5), (5, 7)):
                lam = np.concatenate([np.full(nneg, -d), np.full(npos, d), upper_part(n - nneg - npos, rng)])
                out.append(Case(f"f2-n{n}-d{d:g}-{nneg}neg", dense(lam, rng), 2, nneg=nneg, mp=(n in mp_orders and nneg == 3 and d == 2e-9)))
    return out


def family3(orders, rng, mp_orders=()):
    """Exactly multiple eigenvalues among the 8 (9) smallest, and equal eigenvalues across position 8 and position 9."""
    out = []
    for n in orders:
        base = -1.0 + 0.05 * np.arange(12)                        # twelve separated values below the part in [0.5, 2]
        for name, groups in (("m2", [(2, 4)]), ("m3", [(0, 3)]), ("m8", [(0, 8)]), ("m2m3", [(0, 2), (4, 7)]),
                             ("straddle8", [(7, 9)]), ("straddle9", [(8, 10)]), ("straddle89", [(6, 11)])):
            low = base.copy()
            for a, b in groups:
                low[a:b] = low[a]
            lam = np.concatenate([low, upper_part(n - low.size, rng)])
            out.append(Case(f"f3-n{n}-{name}", dense(lam, rng), 3, mp=(n in mp_orders and name == "m3")))
    return out


GAPS = (1e-14, 1e-10, 1e-6, 5e-4, 2e-3, 1e-2)


def family4(orders, rng, mp_orders=()):
    """Two of the smallest eigenvalues g * scale apart (scale = 2), g on both sides of the solver's re-orthogonalisation
    threshold of 1e-3 * scale."""
    out = []
    for n in orders:
        for g in GAPS:
            for pos in (0, 3):
                low = -1.0 + 0.05 * np.arange(12)
                low[pos + 1] = low[pos] + 2.0 * g
                lam = np.concatenate([low, upper_part(n - low.size, rng)])
                out.append(Case(f"f4-n{n}-g{g:g}-at{pos}", dense(lam, rng), 4, mp=(n in mp_orders and g == 2e-3 and pos == 3)))
    return out


def family6(orders, rng, mp_orders=()):
    """Graded spectra: logspace(-12, 0, n) and its negative."""
    out = []
    for n in orders:
        lam = np.logspace(-12.0, 0.0, n)
        out.append(Case(f"f6-n{n}-pos", dense(lam, rng), 6, vacuous_ok=True, mp=n in mp_orders))
        out.append(Case(f"f6-n{n}-neg", dense(-lam, rng), 6, vacuous_ok=True, mp=n in mp_orders))
    return out


def wilkinson(m=10):
    """W(2m+1)+: diagonal |m|, ..., 1, 0, 1, ..., |m|, off-diagonals 1."""
    d = np.abs(np.arange(-m, m + 1)).astype(np.float64)
    return np.diag(d) + np.diag(np.ones(2 * m), 1) + np.diag(np.ones(2 * m), -1)


def laplacian(n):
    return 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def _laplacian_spectrum(n):
    def f():
        import mpmath as mp
        return [2 - 2 * mp.cos(j * mp.pi / (n + 1)) for j in range(1, n + 1)]
    return f


def direct_sum(A, B):
    n, m = A.shape[0], B.shape[0]
    S = np.zeros((n + m, n + m))
    S[:n, :n] = A
    S[n:, n:] = B
    return S


def family5(rng):
    """Structured blocks, planted exactly.  Every reference here is mpmath, a closed form at 40 digits, or exact."""
    out = []
    for n in (1, 2, 3, 64, 129, 255, 256):
        out.append(Case(f"f5-zero-n{n}", np.zeros((n, n)), 5, closed="diag", vacuous_ok=True))
    for n in (1, 2, 3, 63, 128, 256):
        for a in (1.0, -3.0):
            out.append(Case(f"f5-{a:g}I-n{n}", a * np.eye(n), 5, closed="diag", vacuous_ok=True))
    for n in (2, 3, 65, 127, 255):
        vals = np.concatenate([[-2.0] * min(3, n // 2), rng.standard_normal(n)])[:n]       # repeated and distinct entries
        vals[-1] = vals[0]
        out.append(Case(f"f5-diag-n{n}", np.diag(rng.permutation(vals)), 5, closed="diag", vacuous_ok=True))
    # reducible: a direct sum inside one block (dense (+) dense, dense (+) Laplacian so that large orders keep an mpmath reference)
    spec = lambda n: np.concatenate([np.zeros(5), upper_part(n - 5, rng)])                  # noqa: E731
    out.append(Case("f5-sum-25+40", direct_sum(dense(spec(25), rng), dense(spec(40) - 0.25, rng)), 5, mp=True, parts=[25, 40], vacuous_ok=True))
    out.append(Case("f5-sum-64+65", direct_sum(dense(spec(64), rng), dense(spec(65), rng)), 5, mp=True, parts=[64, 65], vacuous_ok=True))
    for n in (255, 256):
        out.append(Case(f"f5-sum-65+lap-n{n}", direct_sum(dense(spec(65) - 1.0, rng), laplacian(n - 65)), 5, mp=True, parts=[65, n - 65],
                        closed={1: _laplacian_spectrum(n - 65)}, vacuous_ok=True))
    # tridiagonal blocks given as such
    n = 33
    T = np.diag(rng.standard_normal(n)) + np.diag(rng.standard_normal(n - 1), 1)
    out.append(Case("f5-tridiag-n33", np.triu(T) + np.triu(T, 1).T, 5, mp=True, vacuous_ok=True))
    W = wilkinson(10)
    G = direct_sum(W, W)
    G[20, 21] = G[21, 20] = 1e-8
    out.append(Case("f5-W21", W, 5, mp=True, vacuous_ok=True))
    out.append(Case("f5-W21-neg", -W, 5, mp=True, vacuous_ok=True))
    out.append(Case("f5-W21-glued", G, 5, mp=True, vacuous_ok=True))
    out.append(Case("f5-W21-glued-neg", -G, 5, mp=True, vacuous_ok=True))
    for n in (63, 65, 127, 129, 255, 256):
        out.append(Case(f"f5-laplacian-n{n}", laplacian(n), 5, closed=_laplacian_spectrum(n), vacuous_ok=True))
    # one dense block and its 1e-3- and 1e+6-scaled copies: the thresholds must follow the scale (no floor of 1 in the tolerance)
    base = dense(np.concatenate([np.zeros(4), [1e-6, 1e-6], upper_part(59, rng)]) - 0.125, rng)
    for s in (1.0, 1e-3, 1e6):
        out.append(Case(f"f5-scaled-{s:g}-n65", s * base, 5, mp=True, floor=False, vacuous_ok=True))
    return out


DENSE_FAMILIES = {1: family1, 2: family2, 3: family3, 4: family4, 6: family6}
FAMILIES = (1, 2, 3, 4, 5, 6)


def family_cases(fam, mp_orders=(33, 65), orders=None):
    """The cases of one family, always the same (seeded by the family): dense families at ORDERS plus 64, 128 and the example's 211
    and the small orders that carry the mpmath reference."""
    rng = np.random.default_rng(1000 + fam)
    if fam == 5:
        return family5(rng)
    orders = orders if orders is not None else sorted(set(ORDERS) | {64, 128, 211} | set(mp_orders))
    return DENSE_FAMILIES[fam](orders, rng, mp_orders)


# -------------------------------------------------------------------------------------------------------------- reference
@functools.lru_cache(maxsize=None)
def _mp_eigsy_cached(digest, n, raw):
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        A = np.frombuffer(raw, dtype=np.float64).reshape(n, n)
        M = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = mp.mpf(float(A[i, j]))
        E = mp.eigsy(M, eigvals_only=True)
        return tuple(sorted(E[i] for i in range(n)))


def mp_eigsy(A):
    """Eigenvalues of the symmetric float64 matrix A by mpmath.eigsy at 40 digits (kept per process: both storages plant the
    same bits)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    raw = A.tobytes()
    return list(_mp_eigsy_cached(hashlib.sha1(raw).hexdigest(), A.shape[0], raw))


def mp_eigvals(case, S):
    """The 40-digit spectrum of the block S that was read back for `case` (a list of mpmath numbers, ascending), or None when
    the case has no such reference."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        if case.closed == "diag":
            assert np.array_equal(S, np.diag(np.diag(S)))
            return sorted(mp.mpf(float(v)) for v in np.diag(S))
        if callable(case.closed):
            return sorted(case.closed())
        if not case.mp:
            return None
        if case.parts:
            vals, o = [], 0
            for q, m in enumerate(case.parts):
                assert not S[o:o + m, o + m:].any() and not S[o + m:, o:o + m].any()
                sub = case.closed.get(q) if isinstance(case.closed, dict) else None
                vals += list(sub()) if sub else mp_eigsy(S[o:o + m, o:o + m])
                o += m
            return sorted(vals)
        return mp_eigsy(S)


def reference_eigvals(case, S):
    """float64 reference spectrum of the read-back block: the rounded 40-digit one where the case has it, LAPACK's elsewhere."""
    E = mp_eigvals(case, S)
    if E is None:
        return np.linalg.eigvalsh(0.5 * (S + S.T))
    return np.array([float(e) for e in E])


def scale_of(wr, floor=True):
    m = float(np.abs(wr).max()) if len(wr) else 0.0
    return max(1.0, m) if floor else m


def lapack_error_ratio(case):
    """max |eigvalsh - mpmath| / (EIG_TOL * n * scale): the share of the eigenvalue tolerance that the LAPACK reference uses up."""
    import mpmath as mp
    E = mp_eigvals(case, case.S)
    assert E is not None, case.name
    w = np.linalg.eigvalsh(case.S)
    with mp.workdps(MP_DIGITS):
        err = max(abs(mp.mpf(float(a)) - e) for a, e in zip(w, E))
        scale = scale_of(np.array([float(e) for e in E]), case.floor)
        return float(err / (mp.mpf(EIG_TOL) * case.n * scale))


# -------------------------------------------------------------------------------------------------------------- assertions
def bottom_set(wr, kk, scale):
    """Size of J: the kk smallest reference eigenvalues, extended upward until the next one is more than CLUSTER_GAP * scale away."""
    j = kk
    while 0 < j < len(wr) and wr[j] - wr[j - 1] <= CLUSTER_GAP * scale:
        j += 1
    return j


def check_block(S, w, V, k, wr=None, *, floor=True, nneg=-1, nzero=0, vacuous_ok=True, label=""):
    """Everything a block's result must satisfy.  S: the block as read back; w: its n eigenvalues; V: n x k (ignored when k = 0);
    wr: reference eigenvalues (default LAPACK's).  Returns True when the subspace check was vacuous (J = the whole block)."""
    n = S.shape[0]
    S = 0.5 * (S + S.T)
    wl, Ql = np.linalg.eigh(S)
    wr = wl if wr is None else np.asarray(wr)
    scale = scale_of(wr, floor)
    assert w.shape == (n,), label
    assert np.all(np.isfinite(w)), label
    assert np.all(np.diff(w) >= 0), f"{label}: eigenvalues not ascending"
    err = np.abs(w - wr).max()
    assert err <= EIG_TOL * n * scale, f"{label}: eigenvalue error {err:.3e} > {EIG_TOL * n * scale:.3e}"
    if nzero:
        assert np.abs(w[:nzero]).max() <= EIG_TOL * n * scale, f"{label}: zero cluster {np.abs(w[:nzero]).max():.3e}"
    if nneg >= 0:
        assert int(np.sum(wr < 0)) == nneg, f"{label}: the planted block has {int(np.sum(wr < 0))} negative eigenvalues"
        assert int(np.sum(w < 0)) == nneg, f"{label}: {int(np.sum(w < 0))} negative eigenvalues, {nneg} planted"
    if not k:
        return True
    kk = min(k, n)
    assert V.shape == (n, k), label
    assert not np.any(V[:, kk:]), f"{label}: columns beyond the block's order are not zero"
    Vi = V[:, :kk]
    assert np.all(np.isfinite(Vi)), label
    res = np.abs(S @ Vi - Vi * w[:kk]).max()
    assert res <= RES_TOL * n * scale, f"{label}: residual {res:.3e} > {RES_TOL * n * scale:.3e}"
    orth = np.abs(Vi.T @ Vi - np.eye(kk)).max()
    assert orth <= ORTH_TOL, f"{label}: |V'V - I| = {orth:.3e}"
    j = bottom_set(wr, kk, scale)
    if j >= n:
        assert vacuous_ok, f"{label}: the bottom set grew to the whole block"
        return True
    gap = wr[j] - wr[j - 1]
    outside = np.linalg.norm(Ql[:, j:].T @ Vi, axis=0).max()             # LAPACK's basis of the complement of span(J)
    assert outside <= RES_TOL * n * scale / gap, f"{label}: {outside:.3e} outside the eigenspace of the {j} smallest (gap {gap:.3e})"
    return False
