"""GPU tests: finite-difference checks of cost, Riemannian gradient and Hess-vec of every kind THROUGH THE C ABI
(msdp_cost / msdp_rgrad / msdp_hessvec / msdp_proj / msdp_retr), the procedure of manopt/tools/checkgradient.m and
checkhessian.m: on the manifold f(R_Y(tU)) = f + t<G,U> + t^2/2 <U, Hess U> + O(t^3), so halving t divides the residual of
the second-order model by ~8.  Independent of the oracle: the device closures are checked against the device cost alone
(the oracle passes the same check on the CPU, tests/test_oracle_derivatives.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _fd_check(h, Y, Uraw):
    h.set_point(Y)
    f0 = h.cost()
    G = h.rgrad()
    U = h.proj(Uraw)
    U *= np.linalg.norm(Y) / np.linalg.norm(U)             # a step t*U moves every point by ~t times its own size
    H = h.hessvec(U)
    g1 = float(np.sum(G * U))
    g2 = float(np.sum(U * H))
    # the gradient is tangent, the Hess-vec too (ManiSDP_onlyunitdiag.m:129 projects; spherefactory.m:229)
    assert np.linalg.norm(h.proj(G) - G) <= 1e-12 * max(1.0, np.linalg.norm(G))
    assert np.linalg.norm(h.proj(H) - H) <= 1e-11 * max(1.0, np.linalg.norm(H))
    errs, first = [], []
    for t in (2e-2, 1e-2, 5e-3):
        Z = h.retr(t * U)                                  # retraction from the resident point, which stays put
        h.set_point(Z)
        ft = h.cost()
        h.set_point(Y)
        h.cost()                                           # per-point state back at Y for the next retraction
        errs.append(abs(ft - (f0 + t * g1 + 0.5 * t * t * g2)))
        first.append(abs(ft - (f0 + t * g1)))
    # first-order model: error O(t^2) (ratio ~4); second-order model: O(t^3) (ratio ~8)
    assert 3.0 < first[0] / first[1] < 5.5 and 3.0 < first[1] / first[2] < 5.5, first
    assert errs[0] / max(errs[1], 1e-300) > 5.5 and errs[1] / max(errs[2], 1e-300) > 5.5, errs
    # symmetry of the Hessian on the tangent space: <V, Hess U> = <U, Hess V>
    V = h.proj(np.random.default_rng(99).standard_normal(U.shape))
    HV = h.hessvec(V)
    a, b = float(np.sum(V * H)), float(np.sum(U * HV))
    assert abs(a - b) <= 1e-10 * max(1.0, abs(a), abs(b))


@pytest.mark.parametrize("p", [3, 20, 70])
def test_fd_onlyunitdiag_sparse_and_dense(lib, p):
    from manisdp_matlab_amd import problems
    C = problems.toroidal_grid_maxcut(30, 40, seed=2)
    n = C.shape[0]
    rng = np.random.default_rng(p)
    Y = rng.standard_normal((n, p)); Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    U = rng.standard_normal((n, p))
    for Cm in (C, C.toarray()):
        h = lib.Handle.onlyunitdiag(Cm, pcap=p)
        _fd_check(h, Y, U)
        h.close()


def _affine(lib, kind, name, p, sigma, seed):
    from manisdp_matlab_amd import problems
    At, b, c, K = problems.from_sdpa(golden_path(name + ".dat-s.gz"))
    c = np.asarray(c.todense()).ravel(); b = np.asarray(b, float)
    n = K["s"]
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((n, p))
    if kind == lib.KIND_UNITDIAG:
        Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    elif kind == lib.KIND_UNITTRACE:
        Y /= np.linalg.norm(Y)
    h = lib.Handle.affine(kind, At, b, c, n, pcap=p)
    h.set_multipliers(0.1 * rng.standard_normal(b.size), sigma)
    return h, Y, rng.standard_normal((n, p))


@pytest.mark.parametrize("route", [1, 2])
def test_fd_unitdiag(lib, route):
    h, Y, U = _affine(lib, lib.KIND_UNITDIAG, "gpp100", 4, 0.5, 1)
    h.set_option("affine_route", route)                    # SDDMM and Gram route of A(Ya Yb')
    _fd_check(h, Y, U)
    h.close()


@pytest.mark.parametrize("name,p", [("theta1", 3), ("theta2", 12)])
def test_fd_unittrace(lib, name, p):
    h, Y, U = _affine(lib, lib.KIND_UNITTRACE, name, p, 3.0, 2)
    _fd_check(h, Y, U)
    h.close()


def test_fd_generic(lib):
    h, Y, U = _affine(lib, lib.KIND_GENERIC, "mcp100", 5, 0.7, 3)
    _fd_check(h, 0.3 * Y, U)
    h.close()


# ---- the dual kinds.  The penalty (sigma, w) is set first, and one outer step at another point moves the device-resident
# multiplier x away from 0, so every term of the cost is live; the outer step spends the penalty, so it is set again.
def _dual_penalised(h, Y0, sigma, w):
    h.dual_set_penalty(sigma, w)
    h.set_point(Y0)
    h.dual_outer_step()
    h.dual_set_penalty(sigma, w)


def _split(A, c, nf):
    Ac = sp.csc_matrix(A)
    return sp.csr_matrix(Ac[:, nf:]), Ac[:, :nf], c[nf:], c[:nf]


@pytest.mark.parametrize("p", [7, 70])
def test_fd_dual_unitdiag(lib, p):
    from manisdp_matlab_amd import problems
    rng = np.random.default_rng(p)
    d = 8
    Q = rng.standard_normal((d, d)); Q = (Q + Q.T) / 2
    A, b, c, K, dAAt, _ = problems.bqpsos_dual_problem(Q, rng.standard_normal(d), d)
    n, nf = K["s"], K["f"]
    Apsd, B, cp, cf = _split(A, c, nf)
    h = lib.Handle.dual_unitdiag(Apsd, b, cp, dAAt, B, cf, pcap=p)
    def point():
        Y = rng.standard_normal((n, p)); return Y / np.linalg.norm(Y, axis=1, keepdims=True)
    _dual_penalised(h, point(), 0.6, 0.2 * rng.standard_normal(nf))
    _fd_check(h, point(), rng.standard_normal((n, p)))
    h.close()


@pytest.mark.parametrize("p", [5, 70])
def test_fd_dual_generic(lib, p):
    from manisdp_matlab_amd import problems
    d = 6
    rng = np.random.default_rng(p)
    A, b, c, K, dAAt = problems.qssos(d, rng.standard_normal(problems.get_basis(d, 4).shape[1]))
    b = b / np.max(np.abs(b))
    n, nf = K["s"], K["f"]
    Apsd, B, cp, cf = _split(A, c, nf)
    h = lib.Handle.dual(Apsd, b, cp, dAAt, B, cf, pcap=p)
    _dual_penalised(h, rng.standard_normal((n, p)) / np.sqrt(p), 0.4, 0.1 * rng.standard_normal(nf))
    _fd_check(h, rng.standard_normal((n, p)) / np.sqrt(p), rng.standard_normal((n, p)))
    h.close()


@pytest.mark.parametrize("widths", [[9, 5, 1, 2], [70, 3, 1, 2]])
def test_fd_dual_multiblock(lib, widths):
    """Blocks of order 70 / 6 / 1 / 5, the first two oblique (the generic closures, nob < nb); zero beyond each block's width."""
    nset, nob, nf, m = [70, 6, 1, 5], 2, 2, 40
    rng = np.random.default_rng(sum(widths))
    off = np.concatenate([[0], np.cumsum([k * k for k in nset])])
    rows = []
    for _ in range(m):
        v = np.zeros(off[-1])
        for blk in rng.choice(len(nset), size=2):
            k = nset[blk]
            Mk = np.zeros((k, k))
            for _ in range(3):
                i, j = rng.integers(0, k, 2)
                a = rng.standard_normal()
                Mk[i, j] += a; Mk[j, i] += a
            v[off[blk]:off[blk + 1]] += Mk.ravel(order="F")
        rows.append(v)
    Apsd = sp.csr_matrix(np.array(rows))
    B = sp.csr_matrix(rng.standard_normal((m, nf)) * (rng.random((m, nf)) < 0.6))
    cp = np.concatenate([(lambda C: 0.2 * (C + C.T))(rng.standard_normal((k, k))).ravel(order="F") for k in nset])
    dAAt = np.asarray(Apsd.multiply(Apsd).sum(axis=1)).ravel()
    h = lib.Handle.dual_multiblock(Apsd, rng.standard_normal(m), cp, dAAt, nset, nob, B, rng.standard_normal(nf),
                                   pcap=max(widths))
    r0 = np.concatenate([[0], np.cumsum(nset)])
    def packed(unit):
        Y = np.zeros((r0[-1], max(widths)))
        for i, (k, w) in enumerate(zip(nset, widths)):
            Yi = rng.standard_normal((k, w))
            Y[r0[i]:r0[i + 1], :w] = Yi / np.linalg.norm(Yi, axis=1, keepdims=True) if (unit and i < nob) else Yi
        return Y
    _dual_penalised(h, packed(True), 0.5, 0.2 * rng.standard_normal(nf))
    _fd_check(h, packed(True), packed(False))
    h.close()
