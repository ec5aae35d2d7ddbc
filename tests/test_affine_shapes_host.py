"""CPU tests of the constructed instance families of tests/affine_shapes_ref.py and of the reference the GPU sweep
(tests/test_gpu_affine_shapes.py) compares against: the families are deterministic, symmetric and have the structure each is
built for (computed from At in Python; on the device the same conditions are read back through Handle.affine_plan()); the
oracle closures agree with a brute-force restatement over dense A_k, and with central differences of their own cost and gradient."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_shapes_ref as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("unitdiag", "unittrace", "generic")

TABLE = [(name, make, cond) for name, (make, cond) in F.FAMILIES.items()]
holds = F.holds


@pytest.mark.parametrize("name,make,cond", TABLE, ids=[t[0] for t in TABLE])
def test_family_is_deterministic_symmetric_and_has_its_structure(name, make, cond):
    At, b, c, n, f = make()
    At2, b2, c2, _, _ = make()
    assert (At != At2).nnz == 0 and np.array_equal(At.data, At2.data) and np.array_equal(b, b2) and np.array_equal(c, c2)
    assert At.shape == (n * n, b.size) and c.shape == (n * n,)
    A = F.dense_constraints(At, n)
    assert np.array_equal(A, A.transpose(0, 2, 1))                         # every A_k symmetric, bit for bit
    Cm = c.reshape(n, n, order="F")
    if cond["usym"]:
        assert np.array_equal(Cm, Cm.T)
    else:
        assert np.count_nonzero(Cm != Cm.T) == 2 and np.abs(Cm - Cm.T).max() < 2e-13
    assert 0.3 < np.sqrt(n) * np.abs(Cm).mean() < 1.0                      # entries of size about 1/sqrt(n)
    assert not holds(f, cond), holds(f, cond)
    # the facts against plain loops over the nonzeros
    share = {}
    for k in range(At.shape[1]):
        for r in At.indices[At.indptr[k]:At.indptr[k + 1]]:
            share.setdefault((r % n, r // n), []).append(k)
    assert f["touched"] == len(share) and f["max_share"] == max(len(v) for v in share.values())
    assert f["max_row"] == max(sum(1 for (i, _) in share if i == r) for r in range(n))
    assert f["nlong_e"] == sum(1 for (i, j), v in share.items() if i <= j and len(v) > 8) * f["usym"]
    assert f["nlong"] == sum(1 for k in range(At.shape[1]) if At.indptr[k + 1] - At.indptr[k] > 128)


def test_what_the_families_are_built_for():
    f = F.support(96)[4]
    assert f["max_row"] > 64 and f["max_row"] % 4 != 0                    # k_support_spmm: second turn of the q0 loop, ragged SPB group
    f = F.support(160, nlong=20)[4]
    assert f["max_row"] > 64 and f["nlong"] > F.MSDP_WAVES
    a, b = F.support(160, nlong=20), F.support(160, nlong=20, long_first=True)
    assert a[4]["nnz_per_k"][0] == 2 and b[4]["nnz_per_k"][0] == 160       # the same constraints in another order
    assert sorted(a[4]["nnz_per_k"]) == sorted(b[4]["nnz_per_k"]) and a[4]["touched"] == b[4]["touched"]
    f = F.crowded(40)[4]
    assert f["nshort"] + f["nlit"] > 16 * 40                               # more k_sddmm1 workgroups of 16 units than rows: the mode-2 grid is capped
    f = F.shared(97)[4]
    assert f["max_share"] == 13
    for g in (1, 2, 3, 4, 6):
        assert F.dense_short(65, g)[4]["upper_per_k"].max() == g


CASES = [("support96", lambda: F.support(96)), ("ds33_3", lambda: F.dense_short(33, 3))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,make", CASES, ids=[t[0] for t in CASES])
def test_oracle_agrees_with_brute_force(name, make, kind):
    At, b, c, n, _ = make()
    p, sigma = 3, 2.3
    rng = np.random.default_rng(11)
    y = 0.1 * rng.standard_normal(b.size)
    Y = F.point(kind, rng, n, p)
    U = F.tangent(kind, Y, rng.standard_normal((n, p)))
    f, G, H = F.evaluate(F.oracle_problem(kind, At, b, c, n, p, y, sigma), Y, U)
    br = F.Brute(kind, At, b, c, n, y, sigma)
    assert abs(f - br.cost(Y)) <= 1e-13 * max(1.0, abs(f))
    assert np.linalg.norm(G - br.grad(Y)) <= 1e-13 * np.linalg.norm(G)
    assert np.linalg.norm(H - br.hess(Y, U)) <= 1e-13 * np.linalg.norm(H)


# Central differences with step FD_STEP along a unit tangent direction.  The cost is a quartic in Y: the truncation error of the
# difference quotients is O(h^2), the rounding error O(eps / h).  Measured with h = 1e-4 over the six cases below (relative to
# |<G, V>| and |H|): gradient at most 1.13e-8 (support96, unittrace), Hess-vec at most 9.59e-9 (support96, unitdiag); the bounds are ten times the largest.
FD_STEP = 1e-4
FD_GRAD_TOL = 1.13e-7
FD_HESS_TOL = 9.59e-8


def _retract(kind, Y):
    if kind == "unitdiag":
        return Y / np.linalg.norm(Y, axis=1, keepdims=True)
    if kind == "unittrace":
        return Y / np.linalg.norm(Y)
    return Y


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,make", CASES, ids=[t[0] for t in CASES])
def test_oracle_derivatives_agree_with_central_differences(name, make, kind):
    At, b, c, n, _ = make()
    p, sigma = 3, 2.3
    rng = np.random.default_rng(12)
    y = 0.1 * rng.standard_normal(b.size)
    Y = F.point(kind, rng, n, p)
    V = F.tangent(kind, Y, rng.standard_normal((n, p)))
    V /= np.linalg.norm(V)
    new = lambda: F.oracle_problem(kind, At, b, c, n, p, y, sigma)
    _, G, H = F.evaluate(new(), Y, V)
    # <grad f, V> = d/dt f(R(Y + t V)) at 0 (R: the retraction, first order)
    h = FD_STEP
    d1 = (new().cost(_retract(kind, Y + h * V)) - new().cost(_retract(kind, Y - h * V))) / (2 * h)
    gv = float(np.sum(G * V))
    eg = abs(d1 - gv) / abs(gv)
    # Hess f [V] = P_Y (D grad[V]): the closures' gradient formulas are smooth in the ambient space around the manifold

    def grad_at(Z):
        prob = new()
        prob.cost(Z)
        return prob.grad(Z)
    d2 = F.tangent(kind, Y, (grad_at(Y + h * V) - grad_at(Y - h * V)) / (2 * h))
    eh = np.linalg.norm(d2 - H) / np.linalg.norm(H)
    print(f"{name} {kind}: central differences, gradient {eg:.2e}, Hess-vec {eh:.2e}")
    assert eg <= FD_GRAD_TOL and eh <= FD_HESS_TOL, (eg, eh)


def test_the_plan_query_is_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "manisdp_hip.h")).read()
    assert re.search(r"\bint\s+msdp_debug_affine_plan\s*\(\s*msdp_handle\s+h\s*,\s*int32_t\s*\*\s*out\s*\)\s*;", txt)
    for field in ("usym", "ntp", "nlong_e", "bW", "packed", "bnlong", "nsup", "nlong", "nshort", "nlit", "nS",
                  "last_hess_path", "last_A_route"):
        assert re.search(r"\b%s\b" % field, txt), field
    from manisdp_matlab_amd import _lib
    assert "msdp_debug_affine_plan" in _lib.SIGNATURES and hasattr(_lib.Handle, "affine_plan")
    assert _lib.AFFINE_PLAN_FIELDS[:4] == ("usym", "ntp", "nlong_e", "bW") and len(_lib.AFFINE_PLAN_FIELDS) == 14
