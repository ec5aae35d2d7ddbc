"""NumPy restatement of the complex unit-diagonal problem  min <C, X>  s.t. X Hermitian PSD, X_ii = 1  with a sparse Hermitian
cost C = A + iB (msdp_create_onlyunitdiag_csc_hermitian, Handle.onlyunitdiag_hermitian): the instances of
tests/test_gpu_hermitian.py, the order-2n real embedding, an operator that lets the CPU oracle run the complex problem on the
real view of the factor, and cost / gradient / Hess-vec / z / the whole AL loop in plain complex algebra.

On its real view (n x 2p doubles, (re, im) interleaved) the complex oblique manifold {Y in C^{n x p}: |y_i| = 1} is
ObliqueNT(2p, n): Re<u, v> on C^p is the real inner product of the views, so the oracle's manifold, tCG and trustregions apply
unchanged once C @ Y means the complex product (class Op)."""
import numpy as np
import scipy.sparse as sp

import lowrank_ref
from lowrank_ref import _W_TABLE

N_GRID = (203, 1031)
P_GRID = (1, 2, 3, 5, 8, 9, 17, 35)       # complex widths: real width 2p = 2 .. 70, every <LPR, 1> instance and <8, 2> / <16, 2> / <64, 2>
P_WIDE = (65, 130)                        # real width 130 / 260: the <64, 2> and <64, 4> instances
STORAGES = ("grid", "hub")                # four entries per row (fixed-width storage) / rows of more than 64 entries (CSR)

_CACHE = {}


def instance(storage, n):
    """C = A + iB (CSR, complex128): A the real table instance, B antisymmetric on the same off-diagonal pattern -- for i < j
    B_ij = _W_TABLE[(5 i + 3 j) % 13] / 4 and B_ji = -B_ij, zero on the diagonal and never zero off it."""
    key = (storage, n)
    if key not in _CACHE:
        A = (lowrank_ref.grid_cs(n) if storage == "grid" else lowrank_ref.hub_cs(n)).tocoo()
        lo, hi = np.minimum(A.row, A.col), np.maximum(A.row, A.col)
        b = np.array([_W_TABLE[(5 * int(i) + 3 * int(j)) % len(_W_TABLE)] for i, j in zip(lo, hi)], dtype=np.float64) / 4.0
        b = np.where(A.row < A.col, b, np.where(A.row > A.col, -b, 0.0))
        C = sp.csr_matrix((A.data + 1j * b, (A.row, A.col)), shape=A.shape)
        C.sort_indices()
        assert abs(C - C.conj().T).nnz == 0 and np.all(C.diagonal().imag == 0)
        off = C.tocoo()
        assert np.all(off.data.imag[off.row != off.col] != 0)
        _CACHE[key] = C
    return _CACHE[key]


def embed(C):
    """The real symmetric matrix of order 2n that acts on [Re v; Im v] as C acts on v."""
    A, B = sp.csr_matrix(C.real), sp.csr_matrix(C.imag)
    return sp.bmat([[A, -B], [B, A]], format="csr")


def embed_point(Y):
    """The 2n x 2p real factor of the embedded problem whose Gram matrix is the embedding of Y Y^H; its cost is twice the complex one."""
    return np.ascontiguousarray(np.block([[Y.real, -Y.imag], [Y.imag, Y.real]]))


def table_point(n, p):
    """Unit-modulus-sum rows: the real table point of width 2p viewed as complex."""
    return np.ascontiguousarray(lowrank_ref.table_point(n, 2 * p)).view(np.complex128)


def table_direction(n, p):
    g = np.random.default_rng(400 + p)
    return g.standard_normal((n, p)) + 1j * g.standard_normal((n, p))


def real_view(Y):
    Y = np.ascontiguousarray(Y, dtype=np.complex128)
    return Y.view(np.float64).reshape(Y.shape[0], -1)


def complex_view(Yr):
    return np.ascontiguousarray(Yr, dtype=np.float64).view(np.complex128)


class Op:
    """C acting on real-interleaved arrays: Op(C) @ Yreal = real view of C @ (complex view of Yreal)."""

    def __init__(self, C):
        self.C = sp.csr_matrix(C)
        self.shape = self.C.shape

    def __matmul__(self, Yr):
        return real_view(self.C @ complex_view(Yr))


# ------------------------------------------------------------------ derivatives, complex algebra
def get_z(C, Y):
    return np.real(np.sum((C @ Y) * np.conj(Y), axis=1))


def cost(C, Y):
    return 0.5 * float(np.sum(get_z(C, Y)))


def rgrad(C, Y):
    CY = C @ Y
    return CY - Y * np.real(np.sum(CY * np.conj(Y), axis=1, keepdims=True))


def hessvec(C, Y, U):
    eG = np.real(np.sum((C @ Y) * np.conj(Y), axis=1, keepdims=True))
    eH = C @ U
    return eH - Y * np.real(np.sum(eH * np.conj(Y), axis=1, keepdims=True)) - U * eG


def solve(C, Y0, options=None):
    """The AL loop of ManiSDP_onlyunitdiag.m in complex algebra: trustregions() of the oracle on the real view, eigh of the
    complex S, the rank decision from Y^H Y, the cut Y Q(:, 1:r), widening [Y, alpha v] with the rows renormalised.  Returns
    (Y, obj, data)."""
    from oracle import manisdp_ref as R, manopt_rtr
    o = dict(p0=2, AL_maxiter=20, tol=1e-8, theta=1e-1, delta=8, alpha=0.5, tolgradnorm=1e-8, TR_maxinner=100, TR_maxiter=40)
    o.update(options or {})
    C = sp.csr_matrix(C)
    n = C.shape[0]
    Y = np.ascontiguousarray(Y0, dtype=np.complex128)
    p = Y.shape[1]
    op = Op(C)
    data = {"status": 0}
    obj = dinf = None
    for it in range(1, o["AL_maxiter"] + 1):
        prob = R._OnlyUnitDiagProblem(op, n, 2 * p, q1="correct")
        Yr, _, info = manopt_rtr.trustregions(prob, real_view(Y).copy(), o["TR_maxiter"], o["TR_maxinner"], o["tolgradnorm"])
        Y = complex_view(Yr)
        Y_eval = Y
        z = get_z(C, Y)
        obj = float(np.sum(z))
        dS, vS = np.linalg.eigh((C - sp.diags(z)).toarray())
        dinf = max(0.0, -dS[0]) / (1.0 + dS[-1])
        w, Q = np.linalg.eigh(Y.conj().T @ Y)
        order = np.argsort(w)[::-1]
        e = np.sqrt(np.maximum(w[order], 0.0))
        Q = Q[:, order]
        r = int(np.sum(e >= o["theta"] * e[0]))
        data["iters"] = it
        if dinf < o["tol"]:
            break
        if r <= p - 1:
            Y = Y @ Q[:, :r]
            p = r
        nne = max(min(int(np.sum(dS < 0)), o["delta"]), 1)
        Y = np.hstack([Y, o["alpha"] * vS[:, :nne]])
        Y = np.ascontiguousarray(Y / np.sqrt(np.sum(np.abs(Y) ** 2, axis=1, keepdims=True)))
        p += nne
    Y = Y_eval
    data.update(dinf=dinf, z=z, p=Y.shape[1], rank=r)
    if dinf > o["tol"]:
        data["status"] = 1
    return Y, obj, data
