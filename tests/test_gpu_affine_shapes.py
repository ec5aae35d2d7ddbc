"""GPU sweep of the primal affine operators (MSDP_KIND_UNITDIAG, _UNITTRACE, _GENERIC) over constructed constraint plans: the
instance families of tests/affine_shapes_ref.py, each built to reach one branch of msdp_affine_hess / msdp_affine_costgrad /
msdp_affine_launch_A / msdp_affine_launch_adjoint, at the widths that select the kernel instances (ld = p rounded up to even).
The reference is the oracle (oracle.manisdp_ref._UnitDiagProblem, _UnitTraceProblem, _GenericProblem), which
tests/test_affine_shapes_host.py checks against a brute-force restatement.

Every case asserts, besides the numbers, that the handle planned what the family is built for and took the route the case is
meant to take (Handle.affine_plan()): a case that silently ran another kernel fails.

* Whole operand 1e-11 relative; every range of 32 rows of G and H 1e-10 max(|ref part|, 1e-3 |ref|); cost 1e-11 max(1, |f|); two
  identical Hess-vec calls bitwise equal (the arrival counter of k_sddmm1 is back at zero).  The tolerances are those of the
  existing affine and dual operator tests.
* w = A(YY') per constraint: |w_k - ref_k| <= 1e-11 max(|ref_k|, |A_k|_F |Y|_F^2).
* The full adjoint sweep entry by entry (al_dual + get_dual_slack), see test_adjoint_entry_by_entry.

The multipliers are y = 0.1 N(0, 1), sigma = 0.37 (unitdiag), 2.3 (unittrace), 12.5 (generic).  The direction is projected to the
tangent space, except for unitdiag at p = 1, where the tangent space is {0}: there the raw direction is used (the closures'
formula is defined for any U, ManiSDP_unitdiag.m:167-170)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_shapes_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, PART_TOL = 1e-11, 1e-10
SIGMA = {"unitdiag": 0.37, "unittrace": 2.3, "generic": 12.5}
KINDS = ("unitdiag", "unittrace", "generic")
WORST = {}                                    # sweep -> largest relative error seen (printed at the end of the module)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    yield _lib
    for sweep, v in sorted(WORST.items()):
        print(f"\n[affine shapes] {sweep}: largest relative error {v:.2e}")


# ------------------------------------------------------------------ data and reference, computed once
@functools.lru_cache(maxsize=None)
def _family(name):
    make, cond = F.FAMILIES[name]
    At, b, c, n, facts = make()
    At.data.setflags(write=False); b.setflags(write=False); c.setflags(write=False)
    normA = np.sqrt(np.asarray(At.multiply(At).sum(axis=0)).ravel())
    return At, b, c, n, facts, cond, normA


def _asym_visible():
    """dense_short(65, 2) with C(3, 7) moved by 0.1."""
    At, b, c, n, _ = F.dense_short(65, 2, asym=0.1)
    return At, b, c, n


@functools.lru_cache(maxsize=None)
def _reference(name, kind, p):
    At, b, c, n = _family(name)[:4]
    rng = np.random.default_rng([p, KINDS.index(kind), len(name)])
    y = 0.1 * rng.standard_normal(b.size)
    Y = F.point(kind, rng, n, p)
    U = rng.standard_normal((n, p))
    if not (kind == "unitdiag" and p == 1):
        U = F.tangent(kind, Y, U)
    prob = F.oracle_problem(kind, At, b, c, n, p, y, SIGMA[kind])
    f, G, H = F.evaluate(prob, Y, U)
    w = At.T @ (Y @ Y.T).ravel(order="F")
    # unitdiag at p = 1: G = eG - Y (Y . eG) is zero in exact arithmetic, what remains is the rounding of eG: compared on that scale
    floor = float(np.linalg.norm(2.0 * (prob.eS.T @ Y))) if (kind == "unitdiag" and p == 1) else 0.0
    out = (y, Y, U, f, G, H, w, floor)
    for a in out[:3] + out[4:7]:
        a.setflags(write=False)
    return out


def _open(lib, name, kind, pcap):
    At, b, c, n = _family(name)[:4]
    k = {"unitdiag": lib.KIND_UNITDIAG, "unittrace": lib.KIND_UNITTRACE, "generic": lib.KIND_GENERIC}[kind]
    return lib.Handle.affine(k, At, b, c, n, pcap=pcap)


# ------------------------------------------------------------------ assertions
def _note(sweep, err, ref):
    if ref > 0:
        WORST[sweep] = max(WORST.get(sweep, 0.0), err / ref)


def _vec(dev, ref, what, sweep, floor=0.0):
    """|dev - ref| <= 1e-11 |ref| on the whole operand, <= 1e-10 max(|ref part|, 1e-3 |ref|) on every range of 32 rows
    (``floor``: the scale of an operand that is zero in exact arithmetic, in the place of |ref|)."""
    assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
    nr, err = max(float(np.linalg.norm(ref)), floor), float(np.linalg.norm(dev - ref))
    _note(sweep, err, nr)
    assert err <= TOL * nr, (what, err, nr)
    for a in range(0, ref.shape[0], 32):
        rp = float(np.linalg.norm(ref[a:a + 32]))
        ep = float(np.linalg.norm(dev[a:a + 32] - ref[a:a + 32]))
        assert ep <= PART_TOL * max(rp, 1e-3 * nr), (what, "rows", a, a + 32, ep, rp, nr)


def _set(h, **opts):
    for k, v in opts.items():
        h.set_option("affine_" + k, v)


def _plan_is(h, name, what, **want):
    plan = h.affine_plan()
    cond = _family(name)[5]
    assert not F.holds(plan, cond), (what, F.holds(plan, cond), plan)
    facts = _family(name)[4]
    for key in ("usym", "ntp", "nlong_e", "bW", "packed", "bnlong", "nsup", "nlong", "nshort", "nlit", "n"):
        assert plan[key] == facts[key], (what, key, plan[key], facts[key])            # the NumPy restatement of the plans
    for key, v in want.items():
        assert plan[key] == v, (what, key, "expected", v, plan)
    return plan


def _operators(h, name, kind, p, what, sweep, path, aroute, primal_route=None):
    """Cost, gradient, Hess-vec (twice) and w at the reference point of (name, kind, p), with the routes the case expects."""
    At, b, c, n, facts, cond, normA = _family(name)
    y, Y, U, f, G, H, w, floor = _reference(name, kind, p)
    h.set_multipliers(y, SIGMA[kind])
    h.set_point(Y)
    fd, Gd = h.cost(), h.rgrad()
    Hd = h.hessvec(U)
    _plan_is(h, name, what, last_hess_path=path, last_A_route=aroute)
    Hd2 = h.hessvec(U)
    _note(sweep, abs(fd - f), max(1.0, abs(f)))
    assert abs(fd - f) <= TOL * max(1.0, abs(f)), (what, fd, f)
    _vec(Gd, G, what + " G", sweep, floor)
    _vec(Hd, H, what + " H", sweep)
    assert np.array_equal(Hd, Hd2), (what, "two identical Hess-vec calls differ", float(np.abs(Hd - Hd2).max()))
    obj, wd = h.al_primal(b.size)
    _plan_is(h, name, what + " al_primal", last_A_route=aroute if primal_route is None else primal_route)
    bound = TOL * np.maximum(np.abs(w), normA * float(np.sum(Y * Y)))
    bad = np.flatnonzero(~(np.abs(wd - w) <= bound))
    assert bad.size == 0, (what, "constraints", bad[:8], (wd - w)[bad[:8]], bound[bad[:8]])
    _note(sweep, float(np.abs(wd - w).max()), float(np.abs(w).max()))
    return Gd, Hd


def _ld(p):
    return p + (p & 1)


# ------------------------------------------------------------------ 1. B route
B_FAMILIES = ["ds33_1", "ds33_2", "ds33_3", "ds33_4", "ds65_1", "ds65_2", "ds65_3", "ds65_4", "ds65_2_normal", "ds65_3_wide",
              "ds65_6", "shared97"]
B_WIDTHS = (1, 2, 3, 8, 17, 32, 33, 64, 65, 130)


@pytest.mark.parametrize("p", B_WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", B_FAMILIES)
def test_b_route(lib, name, kind, p):
    """k_adjoint_gram<BW, PK> with its tail on the Gram route (affine_route = 2) for the oblique, sphere and Euclidean factor:
    path 2; with affine_broute = 0 the two-pass form (k_gram_apply, k_adjoint_tiled, two-matrix contraction): path 6.  Both
    compute the same A'(A(.)), so they agree to 1e-12."""
    h = _open(lib, name, kind, p)
    try:
        _set(h, route=2, broute=1)
        G1, H1 = _operators(h, name, kind, p, f"{name} {kind} p={p} broute=1", "B route", path=2, aroute=3)
        _set(h, route=2, broute=0)
        G0, H0 = _operators(h, name, kind, p, f"{name} {kind} p={p} broute=0", "B route", path=6, aroute=3)
        assert np.linalg.norm(H1 - H0) <= 1e-12 * np.linalg.norm(H0), (name, kind, p, np.linalg.norm(H1 - H0), np.linalg.norm(H0))
        assert np.array_equal(G1, G0)
    finally:
        h.close()


# ------------------------------------------------------------------ 2. support route
S_NARROW = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)
S_WIDE = (127, 128, 129, 256, 257, 384, 385, 511, 512, 513, 600)
S_CASES = ([(nm, p) for nm in ("support96", "support160", "support160_first", "support160_long", "support160_long_first") for p in S_NARROW]
           + [(nm, p) for nm in ("support96", "support160_long_first") for p in S_WIDE])       # the wide widths thinned to two families


def _gram_by_bytes(facts, At, ld):
    """The rule of use_gram_route (msdp_affine.hip) for affine_route = 0."""
    n, nS, nnz = facts["n"], F.dense_nS(facts["n"]), At.nnz
    return nnz * ld * 16.0 > 4.0 * (2.0 * n * nS * 8.0 + nnz * 20.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,p", S_CASES)
def test_support_route(lib, name, kind, p):
    """At touches at most 1/8 of the matrix: restricted adjoint (k_adjoint_support), k_support_spmm<NCH> (ld <= 512), and for the
    sphere / Euclidean factor the fused Hess-vec k_sph_hess_fused<LPR, NCH> behind k_sddmm1 in mode 2 or behind the side job of the
    contraction.  affine_route = 1 keeps the SDDMM at every width (by bytes the library would change to the Gram matrix at
    ld > 73 on support96, and the fused kernels would never see NCH > 1); the last variant leaves the choice to the library.
    The side job takes ld <= 32 and at most MSDP_WAVES long constraints.  ld > 512: the two-pass form with the restricted
    adjoint and the dense contraction."""
    At, facts = _family(name)[0], _family(name)[4]
    ld = _ld(p)
    h = _open(lib, name, kind, p)
    try:
        variants = [(1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 1, 1)] if kind != "unitdiag" else [(1, 1, 1), (1, 0, 0), (0, 1, 1)]
        for route, fuse, side in variants:
            gram = route == 0 and _gram_by_bytes(facts, At, ld)
            if ld > 512:
                path = 6
            elif kind == "unitdiag" or not fuse or gram:
                path = 5
            elif side and facts["nlong"] <= F.MSDP_WAVES and ld <= 32:
                path = 3
            else:
                path = 4
            aroute = 3 if gram else 2 if fuse else 1
            _set(h, route=route, fuse=fuse, side=side)
            _operators(h, name, kind, p, f"{name} {kind} p={p} route={route} fuse={fuse} side={side}", "support route", path, aroute)
    finally:
        h.close()


# ------------------------------------------------------------------ 3. SDDMM grids
@pytest.mark.parametrize("p", (1, 2, 4, 8, 16, 32, 64, 128, 130))
@pytest.mark.parametrize("kind", ("unittrace", "generic"))
@pytest.mark.parametrize("name", ("crowded40", "support160_long", "support160_long_first"))
def test_sddmm_grids(lib, name, kind, p):
    """k_sddmm1 with long constraints whose items start in different workgroups (per_block = 16 * 64 / LPR changes with the
    width; the two orders of support160_long move the items from the end of the unit list to its start): mode 1 (cost, the
    full grid), mode 2 (Hess-vec; on crowded40 the grid is capped at n = 40 rows and the unit loop wraps), mode 0 (al_primal);
    and with affine_fuse = 0 k_sddmm + k_sddmm_finish."""
    facts = _family(name)[4]
    h = _open(lib, name, kind, p)
    try:
        _set(h, route=1, fuse=1)
        _operators(h, name, kind, p, f"{name} {kind} p={p} fuse=1", "SDDMM grids", path=4, aroute=2)
        _set(h, route=1, fuse=0)
        _operators(h, name, kind, p, f"{name} {kind} p={p} fuse=0", "SDDMM grids", path=5 if facts["nsup"] else 6, aroute=1)
    finally:
        h.close()


# ------------------------------------------------------------------ 4. two streams
@pytest.mark.parametrize("p", (6, 40))
@pytest.mark.parametrize("name,kind", [("support96", "unittrace"), ("ds65_2", "unitdiag")])
def test_two_streams(lib, name, kind, p):
    """affine_overlap = 1: 2 eS U on a second stream beside the A(.) / A'(.) chain (path 1), against the oracle and at 1e-12
    against the same handle with the option off.  affine_route is left at 0: the A route is the library's choice by bytes
    (the rule, restated in _gram_by_bytes: SDDMM on support96, and on ds65_2 at p = 6; Gram matrix on ds65_2 at p = 40)."""
    At, facts = _family(name)[0], _family(name)[4]
    aroute = 3 if _gram_by_bytes(facts, At, _ld(p)) else 2
    assert aroute == (3 if (name, p) == ("ds65_2", 40) else 2)
    h = _open(lib, name, kind, p)
    try:
        _set(h, overlap=1)
        _, H1 = _operators(h, name, kind, p, f"{name} {kind} p={p} overlap=1", "two streams", path=1, aroute=aroute)
        _set(h, overlap=0)
        y, Y, U = _reference(name, kind, p)[:3]
        h.set_point(Y)
        h.cost(); h.rgrad()
        H0 = h.hessvec(U)
        assert h.affine_plan()["last_hess_path"] in (2, 3, 4, 5, 6)
        assert np.linalg.norm(H1 - H0) <= 1e-12 * np.linalg.norm(H0), (name, kind, p, np.linalg.norm(H1 - H0), np.linalg.norm(H0))
    finally:
        h.close()


# ------------------------------------------------------------------ 5. asymmetric data
@pytest.mark.parametrize("p", (3, 33))
@pytest.mark.parametrize("kind", ("unitdiag", "generic"))
def test_slightly_asymmetric_data(lib, kind, p):
    """One entry of C moved by 1e-13: no upper view, no tiles, no B route (usym = 0); k_adjoint_dense and the full Gram matrix on
    every A route, path 6 whatever affine_fuse says (the fused sphere Hess-vec needs symmetric data).  The asymmetry is far
    below the tolerances."""
    name = "ds65_2_asym"
    h = _open(lib, name, kind, p)
    try:
        for route in (1, 2):
            for fuse in (0, 1):
                _set(h, route=route, fuse=fuse)
                _operators(h, name, kind, p, f"{name} {kind} p={p} route={route} fuse={fuse}", "asymmetric data", path=6,
                           aroute=3 if route == 2 else 2 if fuse else 1)
    finally:
        h.close()


@pytest.mark.parametrize("kind", ("unitdiag", "generic"))
def test_visibly_asymmetric_cost_matrix(lib, kind):
    """C(3, 7) moved by 0.1, every A_k symmetric.  The oracle does not symmetrise: it applies reshape(c, n, n) as the MATLAB
    closures do.  The device keeps the bytes of c as its row-major dense operand (msdp_affine_setup: the set-up documents c as
    symmetric), which is the TRANSPOSE of MATLAB's column-major reshape(c, n, n), and multiplies it from the left onto the n x p
    factor.  For the unit-diagonal kind that is what the reference does (ManiSDP_unitdiag.m:161, eG = 2*Y*eS with Y p x n, i.e.
    eS' applied to the rows): device and oracle agree on the asymmetric data.  For the generic kind the reference applies S
    itself (ManiSDP.m:158, eG = 2*S*Y with Y n x p), so the device is expected to agree with the oracle on the data with C
    transposed -- and not on the data as given, which this test also pins so that a change of either convention is noticed.
    (A(.) and the cost do not depend on the orientation of C: <C, YY'> = <C', YY'>.)"""
    At, b, c, n = _asym_visible()
    p = 5
    rng = np.random.default_rng(31)
    y = 0.1 * rng.standard_normal(b.size)
    Y = F.point(kind, rng, n, p)
    U = F.tangent(kind, Y, rng.standard_normal((n, p)))
    cT = c.reshape(n, n).ravel(order="F")                                      # vec of C'
    f, G, H = F.evaluate(F.oracle_problem(kind, At, b, c if kind == "unitdiag" else cT, n, p, y, SIGMA[kind]), Y, U)
    k = lib.KIND_UNITDIAG if kind == "unitdiag" else lib.KIND_GENERIC
    h = lib.Handle.affine(k, At, b, c, n, pcap=p)
    try:
        h.set_multipliers(y, SIGMA[kind])
        h.set_point(Y)
        fd, Gd, Hd = h.cost(), h.rgrad(), h.hessvec(U)
        plan = h.affine_plan()
        assert plan["usym"] == 0 and plan["ntp"] == 0 and plan["bW"] == 0 and plan["last_hess_path"] == 6, plan
        assert abs(fd - f) <= TOL * max(1.0, abs(f))
        _vec(Gd, G, f"visible asymmetry {kind} G", "asymmetric data")
        _vec(Hd, H, f"visible asymmetry {kind} H", "asymmetric data")
        if kind == "generic":
            _, G_given, _ = F.evaluate(F.oracle_problem(kind, At, b, c, n, p, y, SIGMA[kind]), Y, U)
            Cm = c.reshape(n, n, order="F")
            D = 2.0 * (Cm.T - Cm) @ Y                                          # rows 3 and 7 only: 0.2 |Y_7|, 0.2 |Y_3|
            assert np.linalg.norm(D) > 1e4 * TOL * np.linalg.norm(G_given)
            assert np.linalg.norm(Gd - G_given - D) <= TOL * np.linalg.norm(G_given)
    finally:
        h.close()


# ------------------------------------------------------------------ 6. state across calls on one handle
def _eval(h, kind, y, sigma, Y, U):
    h.set_multipliers(y, sigma)
    h.set_point(Y)
    return h.cost(), h.rgrad(), h.hessvec(U)


@pytest.mark.parametrize("kind", ("unitdiag", "unittrace"))
def test_state_across_calls_on_one_handle(lib, kind):
    """support160: a point at p = 9, other multipliers and penalty at the same point, a point at p = 40 -- on one handle and on
    three fresh ones, bitwise.  The restricted adjoint writes the touched entries of eS and AyU only and relies on the others
    keeping C and 0 across calls: a stale or overwritten entry shows here.  Then affine_route 1 -> 2 -> 1: the Gram route uses
    scratch of its own (a.W), so the first result comes back bit for bit."""
    name = "support160"
    At, b, c, n = _family(name)[:4]
    rng = np.random.default_rng(77)
    steps = []
    for p, sigma in ((9, 0.37), (9, 2.3), (40, 12.5)):
        if not steps or p != steps[-1][3].shape[1]:
            Y = F.point(kind, rng, n, p)
            U = F.tangent(kind, Y, rng.standard_normal((n, p)))
        steps.append((0.1 * rng.standard_normal(b.size), sigma, p, Y, U))
    h = _open(lib, name, kind, 40)
    try:
        one = [_eval(h, kind, y, s, Y, U) for y, s, p, Y, U in steps]
        assert h.affine_plan()["nsup"] > 0
    finally:
        h.close()
    for (y, s, p, Y, U), got in zip(steps, one):
        g = _open(lib, name, kind, 40)
        try:
            fresh = _eval(g, kind, y, s, Y, U)
        finally:
            g.close()
        assert got[0] == fresh[0] and np.array_equal(got[1], fresh[1]) and np.array_equal(got[2], fresh[2]), (kind, p, s)
        f, G, H = F.evaluate(F.oracle_problem(kind, At, b, c, n, p, y, s), Y, U)
        _vec(got[1], G, f"state {kind} p={p} G", "state")
        _vec(got[2], H, f"state {kind} p={p} H", "state")
    y, s, p, Y, U = steps[2]
    h = _open(lib, name, kind, 40)
    try:
        res = []
        for route in (1, 2, 1):
            _set(h, route=route)
            res.append(_eval(h, kind, y, s, Y, U))
            assert h.affine_plan()["last_A_route"] == (3 if route == 2 else 2)
        assert res[0][0] == res[2][0] and np.array_equal(res[0][1], res[2][1]) and np.array_equal(res[0][2], res[2][2])
        assert np.linalg.norm(res[1][2] - res[0][2]) <= 1e-12 * np.linalg.norm(res[0][2])
    finally:
        h.close()


# ------------------------------------------------------------------ the full adjoint sweep, entry by entry
ADJ_FAMILIES = ["shared97", "ds65_2", "ds65_2_asym", "support160_long", "ds31_2", "ds32_2", "ds33_2", "ds63_2", "ds64_2"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ADJ_FAMILIES)
def test_adjoint_entry_by_entry(lib, name, kind):
    """al_dual runs the FULL adjoint sweep (k_adjoint_tiled with its long-entry waves, or k_adjoint_dense) into S = C - sum_k y_k
    A_k [- diag(z) | - z I]; get_dual_slack returns it.  Every entry against the dense sum, the diagonal shift taken from the
    returned z.  Bound per entry: 1e-13 (|C_ij| + sum_k |y_k A_k,ij| + |z|) -- at most 14 terms are summed in fp64, in any order:
    14 * 2^-53 = 1.6e-15 of the sum of magnitudes, the rest is margin; entries no constraint touches: 1e-13 |C|_max (they are
    copies of C).  Symmetric data: S == S' bitwise (the tiled kernel stores both halves from one sum).  ds65_2_asym: the device
    keeps the bytes of c row-major (see test_visibly_asymmetric_cost_matrix), so its S is compared with C' - sum_k y_k A_k."""
    At, b, c, n, facts = _family(name)[:5]
    p = 4
    rng = np.random.default_rng([5, len(name), KINDS.index(kind)])
    y = 0.1 * rng.standard_normal(b.size)
    Y = F.point(kind, rng, n, p)
    h = _open(lib, name, kind, p)
    try:
        h.set_multipliers(np.zeros(b.size), 1.0)
        h.set_point(Y)
        z = h.al_dual(y)
        S = h.get_dual_slack()
        _plan_is(h, name, f"{name} {kind} al_dual")
    finally:
        h.close()
    Cm = c.reshape(n, n, order="F")
    if not facts["usym"]:
        Cm = Cm.T
    A = F.dense_constraints(At, n)
    ref = Cm - np.einsum("k,kij->ij", y, A)
    mag = np.abs(Cm) + np.einsum("k,kij->ij", np.abs(y), np.abs(A))
    if kind == "unitdiag":
        ref = ref - np.diag(z); mag = mag + np.diag(np.abs(z))
        X = Y @ Y.T
        z_ref = np.sum(X * (Cm - np.einsum("k,kij->ij", y, A)), axis=1)
        assert np.linalg.norm(z - z_ref) <= TOL * np.linalg.norm(z_ref)
    elif kind == "unittrace":
        ref = ref - z * np.eye(n); mag = mag + abs(z) * np.eye(n)
        z_ref = float(np.sum((Y @ Y.T) * (Cm - np.einsum("k,kij->ij", y, A))))
        assert abs(z - z_ref) <= TOL * max(1.0, abs(z_ref))
    else:
        assert z is None
    touched = np.abs(A).sum(axis=0) > 0
    err = np.abs(S - ref)
    bad = np.argwhere(err > 1e-13 * mag)
    assert bad.size == 0, (name, kind, "entries", bad[:6].tolist(), [float(err[i, j]) for i, j in bad[:6]])
    cmax = float(np.abs(Cm).max())
    off = ~touched & ~np.eye(n, dtype=bool)
    assert float(err[off].max(initial=0.0)) <= 1e-13 * cmax
    if facts["usym"]:
        assert np.array_equal(S, S.T), (name, kind, np.argwhere(S != S.T)[:6].tolist())
    _note("adjoint entries (relative to |C|_max)", float(err.max()), cmax)


def test_the_query_refuses_other_handles(lib):
    """MSDP_ESTATE on a handle without affine state, on a dual handle and on a multiblock handle with per-block storage."""
    import scipy.sparse as sp
    from manisdp_matlab_amd import problems
    At, b, c, n = _family("ds33_2")[:4]
    A = sp.csr_matrix(At.T)
    nb = 16                                                                    # 16 blocks: per-block storage by default
    rows = np.array([[4 * k + 1, 4 * k + 2] for k in range(nb)]).ravel()
    Atb = sp.csc_matrix((np.ones(2 * nb), (rows, np.repeat(np.arange(nb), 2))), shape=(4 * nb, nb))
    cb = np.tile(np.array([0.5, 0.25, 0.25, -0.5]), nb)
    makers = [lambda: lib.Handle.onlyunitdiag(problems.toroidal_grid_maxcut(4, 4)),
              lambda: lib.Handle.dual_unitdiag(A, b, c, np.asarray(A.multiply(A).sum(axis=1)).ravel()),
              lambda: lib.Handle.multiblock(Atb, np.zeros(nb), cb, [2] * nb, nb)]
    for make in makers:
        h = make()
        try:
            with pytest.raises(lib.MsdpError) as e:
                h.affine_plan()
            assert e.value.code == -4
        finally:
            h.close()
