"""GPU operator sweep of the three dual kinds (MSDP_KIND_DUAL_UNITDIAG, MSDP_KIND_DUAL, MSDP_KIND_DUAL_MULTIBLOCK) over the
widths, orders and routes that select different kernel instances, against the NumPy restatements
oracle.manisdp_ref._DualUnitDiagProblem, dual_generic_ref.DualGenericProblem (q1 = 'correct') and
dual_multiblock_ref.DualMultiblockProblem.

* Width: ld = p rounded up to even picks the lanes per row of k_rowdot_slabs / k_obl_grad_finish (1 ... 64 lanes, split at
  ld = 2, 4, 8, 16, 32, 64, 128) and k_block_contract<1|2|3|4|8> (split at ld = 16 / 32 / 48 / 64); the p x p Gram kernels
  (k_pp_gram_*, k_pp_apply, k_bpp_*) loop over ld^2 entries.
* Order: k_dual_outer, k_dmb_outer and k_dgen_rows run one wave per row with a 64-lane stride; S = YY' comes from 64 x 64
  tiles of k_gram_mfma (n = 63 / 64 / 65 / 130); k_dual_free runs 256 threads per B column; k_dgen_rows has a grid-stride
  loop beyond m = 16384.
* Route: affine_route x affine_fuse of launch_A, and dense_sym = 2 with the four k_dense_sym shapes.

Every check follows the existing operator tests: an outer step at a first point, the operators at a second point with
another penalty, the outer step again with x != 0.  The assertions are tighter than a global norm, which can hide a wrong
row range or block: 1e-11 relative on the whole operand, and 1e-10 * max(|ref part|, 1e-3 |ref|) on every block and every
range of 64 rows; entries beyond a block's own width exactly zero; two identical calls bitwise equal."""
import itertools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden_path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dual_generic_ref as DG  # noqa: E402
import dual_multiblock_ref as DMB  # noqa: E402
from oracle import manisdp_ref as R  # noqa: E402
from oracle.manisdp_ref import BlockVec  # noqa: E402
from oracle.manopt_rtr import trustregions  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 8, 15, 16, 17, 32, 33, 48, 49, 64, 65, 127, 128)
ROUTES = [(r, f, 0) for r in (0, 1, 2) for f in (0, 1)]         # affine_route x affine_fuse (dense_sym left alone)
SYM_SHAPES = [(0, 1, s) for s in (1, 2, 3, 4)]                   # dense_sym = 2 with dense_sym_rt = s
TOL, PART_TOL = 1e-11, 1e-10


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


# ------------------------------------------------------------------ assertions
def _rows64(lo, hi):
    return [(i, min(i + 64, hi)) for i in range(lo, hi, 64)]


def _vec(dev, ref, parts, what, floor=0.0):
    """|dev - ref| <= 1e-11 max(|ref|, floor) on the whole operand, <= 1e-10 max(|ref part|, 1e-3 |ref|, floor) on every
    row range of ``parts``."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    nr = float(np.linalg.norm(ref))
    err = float(np.linalg.norm(dev - ref))
    assert err <= TOL * max(nr, floor), (what, err, nr)
    for a, b in parts:
        rp = float(np.linalg.norm(ref[a:b]))
        ep = float(np.linalg.norm(dev[a:b] - ref[a:b]))
        assert ep <= PART_TOL * max(rp, 1e-3 * nr, floor), (what, "rows", a, b, ep, rp, nr)


def _scal(dev, ref, what, scale=1.0):
    assert abs(dev - ref) <= TOL * max(scale, abs(ref)), (what, dev, ref)


def _set_route(h, route, fuse, sym):
    h.set_option("affine_route", route)
    h.set_option("affine_fuse", fuse)
    h.set_option("dense_sym", 2 if sym else 1)
    h.set_option("dense_sym_rt", sym)


# ------------------------------------------------------------------ instances
def _sym_rows(rng, sizes, m, nent, blocks_per_row=1):
    """m random constraints, each a symmetric matrix with ``nent`` random (i, j) + (j, i) pairs on ``blocks_per_row``
    random blocks of the direct sum (column-major vec of every block, blocks one after the other)."""
    off = np.concatenate([[0], np.cumsum([k * k for k in sizes])]).astype(np.int64)
    rows, cols, vals = [], [], []
    for r in range(m):
        for blk in rng.choice(len(sizes), size=blocks_per_row):
            k = sizes[blk]
            for _ in range(nent):
                i, j = rng.integers(0, k, 2)
                v = rng.standard_normal()
                rows += [r, r]; cols += [off[blk] + i + j * k, off[blk] + j + i * k]; vals += [v, v]
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, int(off[-1])))


def _sym_cost(rng, sizes):
    return np.concatenate([(lambda C: 0.2 * (C + C.T))(rng.standard_normal((k, k))).ravel(order="F") for k in sizes])


def _single_data(Apsd, B, rng, n, dAAt=None):
    """(A, b, c, K, dAAt) in the layout of the solvers: [B, A_psd], [c_f, vec(C)]."""
    m, nf = Apsd.shape[0], B.shape[1]
    A = sp.hstack([B, Apsd]).tocsr()
    c = np.concatenate([rng.standard_normal(nf), _sym_cost(rng, [n])])
    if dAAt is None:
        dAAt = np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel()
    return A, rng.standard_normal(m), c, {"f": nf, "s": n}, dAAt


def _random_single(n, m, nf, seed):
    rng = np.random.default_rng(seed)
    Apsd = _sym_rows(rng, [n], m, 4)
    B = sp.csr_matrix(rng.standard_normal((m, nf)) * (rng.random((m, nf)) < 0.5))
    return _single_data(Apsd, B, rng, n)


def _bqp_unit(d, seed):
    from manisdp_matlab_amd import problems
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((d, d)); Q = (Q + Q.T) / 2
    A, b, c, K, dAAt, _ = problems.bqpsos_dual_problem(Q, rng.standard_normal(d), d)
    return A, b, c, K, dAAt


def _qssos(d):
    from manisdp_matlab_amd import problems
    if d == 10:
        coe = np.loadtxt(golden_path("qs_c_10_1.txt.gz"), delimiter=",").ravel()
    else:
        coe = np.random.default_rng(5).standard_normal(problems.get_basis(d, 4).shape[1])
    A, b, c, K, dAAt = problems.qssos(d, coe)
    return A, b / float(np.max(np.abs(b))), c, K, dAAt


def _random_multi(nset, nob, nf, m, seed):
    rng = np.random.default_rng(seed)
    Apsd = _sym_rows(rng, nset, m, 3, blocks_per_row=2)
    B = sp.csr_matrix(rng.standard_normal((m, nf)) * (rng.random((m, nf)) < 0.6)) if nf else None
    dAAt = np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel()
    return Apsd, B, rng.standard_normal(m), _sym_cost(rng, nset), rng.standard_normal(nf), dAAt


# ------------------------------------------------------------------ the kinds behind one interface
class _Single:
    """Dual unit-diagonal (``unit``: oblique rows, z) or generic (Euclidean) kind: one (n, p) factor."""

    def __init__(self, lib, kind, A, b, c, K, dAAt, pcap=128):
        nf, n = K["f"], K["s"]
        Ac = sp.csc_matrix(A)
        c = np.asarray(c, dtype=np.float64).ravel()
        self.Apsd, self.B = sp.csr_matrix(Ac[:, nf:]), Ac[:, :nf]
        self.cp, self.cf = c[nf:], c[:nf]
        self.b, self.n, self.nf, self.unit = np.asarray(b, dtype=np.float64), n, nf, kind == "unit"
        if self.unit:
            self.ref = R._DualUnitDiagProblem(self.Apsd, self.B, self.b, self.cp, self.cf, dAAt, n, 1)
            make = lib.Handle.dual_unitdiag
        else:
            self.ref = DG.DualGenericProblem(self.Apsd, self.B, self.b, self.cp, self.cf, dAAt, n, 1, q1="correct")
            make = lib.Handle.dual
        self.h = make(self.Apsd, self.b, self.cp, dAAt, self.B if nf else None, self.cf if nf else None, pcap=pcap)
        self.parts = _rows64(0, n)
        self.pad = None                                  # the API returns the p columns only

    def set_width(self, p):
        if self.unit:
            self.ref.M = R.ObliqueNT(p, self.n, inner_all=False)
        else:
            self.ref.set_width(p)

    def _norm(self, Y):
        return Y / np.linalg.norm(Y, axis=1, keepdims=True) if self.unit else Y

    def point(self, rng, p):
        return self._norm(rng.standard_normal((self.n, p)))

    def direction(self, rng, p):
        return rng.standard_normal((self.n, p))

    def pack(self, Y):
        return Y

    def proj(self, Y, Z):
        return Z - Y * np.sum(Y * Z, axis=1, keepdims=True) if self.unit else Z.copy()

    def retr(self, Y, U):
        return self._norm(Y + U)

    def trial(self, Y, V, alpha):
        return self._norm(Y + alpha * V)

    def penalty(self, sigma, w):
        self.ref.sigma, self.ref.w = sigma, np.array(w, dtype=np.float64)
        self.h.dual_set_penalty(sigma, w if self.nf else None)

    def cost(self, Y):
        return self.ref.cost(Y)

    def grad(self, Y):
        self.ref.cost(Y)
        return self.ref.grad(Y)

    def hess(self, Y, U):
        return self.ref.hess(Y, U)

    def co(self, Y):
        return self.ref.cost(Y) if self.unit else self.ref.co(Y)

    def outer(self, Y):
        """Outer step at the resident point Y on the device and in the restatement (updated before any assertion, so the two
        stay in step)."""
        by, cex, as2, Af, z = self.h.dual_outer_step()
        slack, ydev = self.h.get_dual_slack(), self.h.dual_get_y()
        ref, n, sigma = self.ref, self.n, self.ref.sigma
        S = Y @ Y.T
        sc = S.ravel(order="F") - self.cp
        y = ref.iAt @ sc
        As = ref.At @ y - sc
        Af_r = ref.B.T @ y - self.cf
        if self.unit:
            ref.x = ref.x - sigma * As                                               # ManiDSDP_unitdiag.m:77
            eX = (ref.x + ref.bA).reshape((n, n), order="F")
            z_r = np.sum(S * eX, axis=0)
            X_r = eX - np.diag(z_r)                                                  # :81
        else:
            ref.x = ref.x + sigma * (ref.iAB @ (Af_r - ref.w / sigma) + ref.At @ (ref.iAt @ (As - ref.x / sigma)) - As)   # ManiDSDP.m:73
            ref.w = ref.w - sigma * Af_r                                             # :74
            eX = (ref.x + ref.bA).reshape((n, n), order="F")
            X_r = eX
        _scal(by, float(self.b @ y), "b'y")
        _scal(as2, float(As @ As), "|As|^2")
        _scal(cex, float(self.cp @ eX.ravel(order="F")), "<C,eX>", float(np.abs(eX).sum()))
        if self.nf:
            # unit diagonal: B'y - cf is 0 up to rounding on the BQP instances (y_1 = tr(S)/n = 1)
            _vec(Af, Af_r, [], "Af", floor=(1.0 + float(np.linalg.norm(y))) if self.unit else 0.0)
        if self.unit:
            _vec(z, z_r, self.parts, "z")
        _vec(slack, X_r, self.parts, "dual slack")
        _vec(ydev, y, _rows64(0, y.size), "y")


class _Multi:
    """Multiblock dual kind: blocks of orders ``nset``, the first ``nob`` oblique; per-block widths packed into (N, pmax)."""

    def __init__(self, lib, Apsd, B, b, cp, cf, dAAt, nset, nob, pcap=128):
        self.nset, self.nob = list(nset), int(nob)
        self.nf = 0 if B is None else B.shape[1]
        self.r0 = np.concatenate([[0], np.cumsum(self.nset)]).astype(int)
        self.ref = DMB.DualMultiblockProblem(Apsd, B, b, cp, cf, dAAt, self.nset, self.nob)
        self.h = lib.Handle.dual_multiblock(Apsd, b, cp, dAAt, self.nset, self.nob, B, cf if self.nf else None, pcap=pcap)
        # every block, and every 64 rows inside a longer block
        self.parts = [(int(a), int(e)) for a, e in zip(self.r0[:-1], self.r0[1:])]
        self.parts += [q for a, e in zip(self.r0[:-1], self.r0[1:]) if e - a > 64 for q in _rows64(int(a), int(e))]
        self.zrows = int(self.r0[self.nob])

    def set_width(self, widths):
        self.pw = list(widths)
        self.ref.set_widths(self.pw)
        self.pad = self.pack(BlockVec([np.ones((n, w)) for n, w in zip(self.nset, self.pw)])) == 0

    def _norm(self, blocks):
        return BlockVec([Y / np.linalg.norm(Y, axis=1, keepdims=True) if i < self.nob else Y for i, Y in enumerate(blocks)])

    def point(self, rng, widths):
        return self._norm([rng.standard_normal((n, w)) for n, w in zip(self.nset, widths)])

    def direction(self, rng, widths):
        return BlockVec([rng.standard_normal((n, w)) for n, w in zip(self.nset, widths)])

    def pack(self, Y):
        out = np.zeros((self.r0[-1], max(self.pw)))
        for i, Yi in enumerate(Y.b):
            out[self.r0[i]:self.r0[i + 1], :Yi.shape[1]] = Yi
        return out

    def proj(self, Y, Z):
        return self.ref.M.proj(Y, Z)

    def retr(self, Y, U):
        return self.ref.M.retr(Y, U)

    def trial(self, Y, V, alpha):
        return self._norm([y + alpha * v for y, v in zip(Y.b, V.b)])

    def penalty(self, sigma, w):
        self.ref.sigma, self.ref.w = sigma, np.array(w, dtype=np.float64)
        self.h.dual_set_penalty(sigma, w if self.nf else None)

    def cost(self, Y):
        return self.ref.cost(Y)

    def grad(self, Y):
        return self.ref.grad(Y)

    def hess(self, Y, U):
        return self.ref.hess(Y, U)

    def co(self, Y):
        return self.ref.co(Y)

    def outer(self, Y):
        by, cex, as2, Af, z = self.h.dual_outer_step()
        slack = [self.h.get_dual_slack_block(int(self.r0[i]), n) for i, n in enumerate(self.nset)]
        ydev = self.h.dual_get_y()
        by_r, cex_r, as2_r, Af_r, z_r, X_r, y_r = self.ref.outer(Y)
        _scal(by, by_r, "b'y")
        _scal(cex, cex_r, "<C,X>")
        _scal(as2, as2_r, "|As|^2")
        if self.nf:
            _vec(Af, Af_r, [], "Af")
        assert z.shape == z_r.shape
        if z.size:
            _vec(z, z_r, [q for q in self.parts if q[1] <= self.zrows], "z")
        for i, (Xd, Xr) in enumerate(zip(slack, X_r)):
            _vec(Xd, Xr, _rows64(0, Xr.shape[0]), "dual slack block %d" % i)
        _vec(ydev, y_r, _rows64(0, y_r.size), "y")


def _padzero(a, M, what):
    if a.pad is not None:
        assert np.all(M[a.pad] == 0.0), what + ": nonzero beyond a block's own width"


def _protocol(a, widths, rng):
    """Outer step at a first point (x = 0 on a fresh handle), the operators at a second point with another penalty (each
    called twice: bitwise equal), then the outer step again at that point (x != 0)."""
    a.set_width(widths)
    a.penalty(0.37, rng.standard_normal(a.nf))
    Y0 = a.point(rng, widths)
    a.h.set_point(a.pack(Y0))
    a.outer(Y0)
    a.penalty(2.3, rng.standard_normal(a.nf))
    Y = a.point(rng, widths)
    a.h.set_point(a.pack(Y))
    fd = a.h.cost()
    _scal(fd, a.cost(Y), "cost")
    Gd = a.h.rgrad()
    _vec(Gd, a.pack(a.grad(Y)), a.parts, "rgrad")
    _padzero(a, Gd, "rgrad")
    assert np.array_equal(Gd, a.h.rgrad()) and a.h.cost() == fd
    Z = a.direction(rng, widths)
    Pd = a.h.proj(a.pack(Z))
    U = a.proj(Y, Z)
    _vec(Pd, a.pack(U), a.parts, "proj")
    _padzero(a, Pd, "proj")
    Hd = a.h.hessvec(a.pack(U))
    _vec(Hd, a.pack(a.hess(Y, U)), a.parts, "hessvec")
    _padzero(a, Hd, "hessvec")
    assert np.array_equal(Hd, a.h.hessvec(a.pack(U)))
    Rd = a.h.retr(a.pack(U))
    _vec(Rd, a.pack(a.retr(Y, U)), a.parts, "retr")
    _padzero(a, Rd, "retr")
    V = a.direction(rng, widths)
    ft = a.co(a.trial(Y, V, 0.3))
    lc = a.h.linesearch_cost(a.pack(V), 0.3)
    _scal(lc, ft, "line-search cost")
    assert lc == a.h.linesearch_cost(a.pack(V), 0.3)
    a.h.set_point(a.pack(Y))
    a.outer(Y)


# ------------------------------------------------------------------ width x route on one mid-size instance per kind
MB_MID = [1, 9, 130, 40]            # block 0 below min_facsize; block 2 carries pmax = p


def _mid_widths(kind, p):
    return [1, min(p, 9), p, min(p, 40)] if kind == "multi" else p


@pytest.fixture(scope="module")
def mid(lib):
    data = {}

    def make(kind):
        """A fresh handle (pcap = 128) and restatement on the mid-size instance of the kind, x = 0."""
        if kind not in data:
            if kind == "unit":
                data[kind] = _bqp_unit(12, seed=12)                                          # n = 79
            elif kind == "generic":
                data[kind] = _qssos(10)                                                      # n = 66, m = 1001
            else:
                data[kind] = _random_multi(MB_MID, 2, 3, 160, seed=21)
        if kind == "multi":
            return _Multi(lib, *data[kind], MB_MID, 2)
        return _Single(lib, kind, *data[kind])
    return make


@pytest.mark.parametrize("kind", ["unit", "generic", "multi"])
@pytest.mark.parametrize("p", WIDTHS)
def test_width_route_sweep(lib, mid, kind, p):
    """Every width under every launch_A route and, for the two kinds with one factor and symmetric data (p <= 32), every
    k_dense_sym shape; each variant on the same points against the restatement.  Every variant starts from x = 0 on a fresh
    handle: at random points the generic outer step x <- x + sigma*(A'(D\\A(As - x/sigma)) - As) grows x geometrically
    where A'D\\A is no projector, and the device forms |As|^2 as (As - x/sigma) + x/sigma, so a long chain of outer steps
    on one handle measures that cancellation, not the kernels."""
    variants = list(ROUTES)
    if kind != "multi" and p <= 32:
        variants += SYM_SHAPES
    for route, fuse, sym in variants:
        a = mid(kind)
        _set_route(a.h, route, fuse, sym)
        try:
            _protocol(a, _mid_widths(kind, p), np.random.default_rng(1000 + p))
        except AssertionError as e:
            raise AssertionError("affine_route %d, affine_fuse %d, dense_sym_rt %d: %s" % (route, fuse, sym, e)) from e
        finally:
            a.h.close()


# ------------------------------------------------------------------ orders x a few widths
@pytest.mark.parametrize("inst", [("bqp", 10), ("bqp", 12), ("bqp", 20), ("rand", 63), ("rand", 64), ("rand", 65),
                                  ("rand", 130)])
def test_unitdiag_orders(lib, inst):
    """bqpsos at d = 10 / 12 / 20 (n = 56 / 79 / 211) and random symmetric constraints at the 64-row tile edges."""
    src, v = inst
    data = _bqp_unit(v, seed=v) if src == "bqp" else _random_single(v, 3 * v, 2, seed=v)
    a = _Single(lib, "unit", *data)
    rng = np.random.default_rng(v)
    for p in (3, 33, 128):
        _protocol(a, p, rng)
    if src == "rand":                   # the Gram route: A(YY') over the same k_gram_mfma tiles as S
        _set_route(a.h, 2, 0, 0)
        _protocol(a, 17, rng)
    a.h.close()


@pytest.mark.parametrize("d", [10, 16, 24])
def test_generic_orders(lib, d):
    """qssos at d = 10 / 16 / 24: n = 66 / 153 / 325, m = 1001 / 4845 / 20475 (d = 24: beyond the 16384 rows of one grid of
    k_dgen_rows).  The setup proves G = D\\A A' = I on these instances."""
    A, b, c, K, dAAt = _qssos(d)
    a = _Single(lib, "generic", A, b, c, K, dAAt)
    assert a.h.dual_g_identity()
    rng = np.random.default_rng(d)
    for p in ((3, 33, 128) if d < 24 else (5, 128)):
        _protocol(a, p, rng)
    a.h.close()


def test_generic_long_rows_and_free_columns(lib):
    """An A row with 200 entries (> 64 lanes of k_dgen_rows) and a B column with 300 entries (> 256 threads of k_dual_free),
    nf = 3."""
    rng = np.random.default_rng(31)
    n, m, nf = 40, 300, 3
    Apsd = _sym_rows(rng, [n], m, 3).tolil()
    pairs = [q for q in itertools.combinations(range(n), 2)]
    for t in rng.choice(len(pairs), size=100, replace=False):
        i, j = pairs[t]
        v = rng.standard_normal()
        Apsd[0, i + j * n] += v; Apsd[0, j + i * n] += v
    Apsd = Apsd.tocsr()
    B = rng.standard_normal((m, nf)) * (rng.random((m, nf)) < 0.3)
    B[:, 0] = rng.standard_normal(m)
    B = sp.csr_matrix(B)
    assert np.diff(Apsd.indptr).max() > 64 and np.diff(sp.csc_matrix(B).indptr).max() > 256
    a = _Single(lib, "generic", *_single_data(Apsd, B, rng, n))
    assert not a.h.dual_g_identity()
    for p in (5, 65):
        _protocol(a, p, rng)
    a.h.close()


def test_generic_disjoint_supports_without_identity(lib):
    """Disjoint supports but dAAt = 2 x the squared row norms: G = D\\A A' = I/2, so the setup must not take the G = I
    shortcut, and the Hess-vec keeps its G terms."""
    rng = np.random.default_rng(41)
    n, m, nf = 30, 200, 2
    pairs = [q for q in itertools.combinations(range(n), 2)]
    rows, cols, vals = [], [], []
    for k, t in enumerate(rng.choice(len(pairs), size=m, replace=False)):
        i, j = pairs[t]
        v = rng.standard_normal()
        rows += [k, k]; cols += [i + j * n, j + i * n]; vals += [v, v]
    Apsd = sp.csr_matrix((vals, (rows, cols)), shape=(m, n * n))
    B = sp.csr_matrix(rng.standard_normal((m, nf)) * (rng.random((m, nf)) < 0.5))
    dAAt = 2.0 * np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel()
    a = _Single(lib, "generic", *_single_data(Apsd, B, rng, n, dAAt=dAAt))
    assert not a.h.dual_g_identity()
    for p in (4, 33):
        _protocol(a, p, rng)
    a.h.close()


MB_ORDERS = [1, 63, 64, 65, 130, 7]


@pytest.mark.parametrize("nob,nf", [(6, 0), (0, 3), (3, 3), (6, 3)])
def test_multiblock_orders(lib, nob, nf):
    """Blocks of order 1 (below min_facsize), 63, 64, 65, 130 and 7; per-block widths that differ, pmax = 128 and 64."""
    Apsd, B, b, cp, cf, dAAt = _random_multi(MB_ORDERS, nob, nf, 300, seed=50 + 10 * nob + nf)
    a = _Multi(lib, Apsd, B, b, cp, cf, dAAt, MB_ORDERS, nob)
    rng = np.random.default_rng(nob + nf)
    for widths in ([1, 40, 64, 17, 128, 3], [1, 64, 33, 64, 50, 2]):
        _protocol(a, widths, rng)
    a.h.close()


def test_multiblock_many_blocks(lib):
    """104 blocks of mixed orders 1 ... 13, the first 52 oblique, nf = 3, per-block widths 1 ... 12."""
    nset = [(1, 2, 3, 5, 8, 13, 4, 7, 11, 6)[i % 10] for i in range(104)]
    widths = [1 if k == 1 else min(k, 1 + (7 * i) % 12) for i, k in enumerate(nset)]
    Apsd, B, b, cp, cf, dAAt = _random_multi(nset, 52, 3, 400, seed=60)
    a = _Multi(lib, Apsd, B, b, cp, cf, dAAt, nset, 52)
    _protocol(a, widths, np.random.default_rng(60))
    a.h.close()


# ------------------------------------------------------------------ width changes and the width limit on one handle
def _small(lib, kind, pcap=32):
    if kind == "unit":
        return _Single(lib, "unit", *_bqp_unit(8, seed=8), pcap=pcap)                       # n = 37
    if kind == "generic":
        return _Single(lib, "generic", *_qssos(6), pcap=pcap)                                # n = 28
    Apsd, B, b, cp, cf, dAAt = _random_multi(MB_MID, 2, 3, 160, seed=22)
    return _Multi(lib, Apsd, B, b, cp, cf, dAAt, MB_MID, 2, pcap=pcap)


def _hess_at(a, widths, rng, sigma=0.5):
    """Cost and Hess-vec at a fresh point of the given width against the restatement; returns the point."""
    a.set_width(widths)
    a.penalty(sigma, 0.1 * rng.standard_normal(a.nf))
    Y = a.point(rng, widths)
    a.h.set_point(a.pack(Y))
    _scal(a.h.cost(), a.cost(Y), "cost")
    a.grad(Y)
    U = a.proj(Y, a.direction(rng, widths))
    Hd = a.h.hessvec(a.pack(U))
    _vec(Hd, a.pack(a.hess(Y, U)), a.parts, "hessvec")
    _padzero(a, Hd, "hessvec")
    return Y


@pytest.mark.parametrize("kind", ["unit", "generic", "multi"])
def test_width_changes_on_one_handle(lib, kind):
    """p = 2 -> 65 -> 3 -> 128 -> 8 -> 127 on one handle that starts at pcap = 32, as the AL loop widens and cuts the factor:
    the Hess-vec against the restatement and a short trustregions() call against the oracle's at every width (G2[slot],
    M1 and pp_part must not carry the previous width)."""
    a = _small(lib, kind)
    rng = np.random.default_rng(7)
    for p in (2, 65, 3, 128, 8, 127):
        widths = _mid_widths(kind, p)
        Y = _hess_at(a, widths, rng)
        kw = {"Delta_bar": a.ref.M.typicaldist()} if kind == "multi" else {}
        st = a.h.rtr(lib.default_opts(maxiter=2, maxinner=4, tolgradnorm=1e-8, **kw))
        Yr, fr, info = trustregions(a.ref, Y.copy(), 2, 4, 1e-8)
        assert st.hessvecs == info.hessvecs and st.hessvecs > 0, (p, st.hessvecs, info.hessvecs)
        assert abs(st.cost - fr) <= 1e-10 * max(1.0, abs(fr)), (p, st.cost, fr)
    a.h.close()


@pytest.mark.parametrize("kind", ["unit", "generic", "multi"])
def test_width_limit_boundary(lib, kind):
    """p = 127 and 128 (ld = 128) are served; p = 129 (ld = 130) is refused with the message; the handle stays usable.
    Multiblock: the limit applies to pmax."""
    a = _small(lib, kind, pcap=128)
    rng = np.random.default_rng(9)
    for p in (127, 128):
        _hess_at(a, _mid_widths(kind, p), rng)
    wide = _mid_widths(kind, 129)
    a.set_width(wide)
    a.penalty(0.5, np.zeros(a.nf))
    a.h.set_point(a.pack(a.point(rng, wide)))
    with pytest.raises(lib.MsdpError, match="exceeds the supported maximum"):
        a.h.cost()
    _hess_at(a, _mid_widths(kind, 128), rng)
    a.h.close()
