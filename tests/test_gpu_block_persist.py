"""The persistent single-launch tCG of the block kinds (option "block_persist", msdp_blockpersist.hip) against the generic
per-iteration path of the same handle and the NumPy restatements (tests/blockdiag_ref.py, tests/posegraph_ref.py): counts,
points and tCG invariants over every lanes-per-block instance and both row-slot counts, the pose rows, ineligible handles,
the fall-back after a time-out, whole solves and the benchmark hook.  tests/test_block_persist_cases_host.py shows on the CPU
that the counts of every case used here do not move under 1e-14 perturbations of the start.  Every run that is meant to be
persistent asserts the kernel instance the plan selects (K.plan_of, the ledger of tests/block_persist_cases.py) before and
tcg_path() == 1 after it: a launch that timed out and was repeated on the chunked path would leave 0 there.

The yardstick of a rounding-level figure is the EXISTING path: with e_gen and e_per the errors of the generic and of the
persistent path against the restatement, e_per <= max(10 e_gen, 1e-12) -- the factor for another summation order of two
rounding-level results, the floor the project's operator tolerance."""
import numpy as np
import pytest
import scipy.sparse as sp

import block_persist_cases as K
import blockdiag_ref as BD
import posegraph_ref as PG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _rule(e_per, e_gen):
    return e_per <= max(10.0 * e_gen, 1e-12)


def _handle(lib, kind, C, d, pcap=32):
    return lib.Handle.onlyunitblockdiag(C, d, pcap=pcap) if kind == "stiefel" else lib.Handle.posegraph(C, d, pcap=pcap)


def _rot3(kind, Y, d):
    return BD.to3(Y, d) if kind == "stiefel" else PG.rot(Y, d)


def _dev_counts(st):
    return (st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner)


def _select(h, on, grid=0):
    h.set_option("block_persist", 1 if on else 0)
    h.set_option("block_persist_grid", grid)


def _rtr(lib, h, Y0, maxiter, maxinner=K.MAXINNER, tol=K.TOLGRADNORM, **more):
    h.set_point(Y0)
    st = h.rtr(lib.default_opts(maxiter=maxiter, maxinner=maxinner, tolgradnorm=tol, **more))
    return st, h.get_point()


def _planned(h, kind, n, d, p, grid, wide=0):
    """The handle is on the persistent path with exactly the plan of the ledger: lanes per block, row slots and grid."""
    assert h.tcg_path() == 1 and h.persist_form() == 0, (kind, n, d, p, grid)
    plan, want = h.block_persist_plan(), K.plan_of(kind, n, d, p, grid, wide=wide)
    assert want is not None and plan["eligible"] == 1, (kind, n, d, p, grid, plan)
    assert {k: plan[k] for k in ("lpr", "slots", "grid", "lds")} == {k: want[k] for k in ("lpr", "slots", "grid", "lds")}, (kind, n, d, p, grid, plan, want)
    return plan


# ------------------------------------------------------------------ 1. counts
@pytest.mark.parametrize("kind", ["stiefel", "pose"])
def test_count_case_on_the_persistent_path(lib, kind):
    R = K.ref(kind)
    c = R.COUNT_CASE
    C, Y0 = R.count_case()
    _, f_ref, info = R.trustregions(C, Y0, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
    h = _handle(lib, kind, C, c["d"], pcap=c["p"])
    try:
        h.set_option("block_persist", 1)
        h.set_point(Y0)
        assert h.tcg_path() == 1 and h.persist_form() == 0
        st = h.rtr(lib.default_opts(maxiter=c["maxiter"], maxinner=c["maxinner"], tolgradnorm=c["tolgradnorm"]))
        print("rtr (%s): device" % kind, _dev_counts(st), st.cost, "restatement", R.counts(info), f_ref)
        assert _dev_counts(st) == R.counts(info)
        assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
        assert abs(h.cost() - st.cost) <= 1e-11 * abs(st.cost)
        Y3 = _rot3(kind, h.get_point(), c["d"])
        assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(c["d"]))) < 1e-13
        assert h.tcg_path() == 1
    finally:
        h.close()


# ------------------------------------------------------------------ 2. shape sweep
def _sweep(lib, kind, n, d, ps):
    """Three iterations from K.start at every width of ps on the generic path, the planned grid and the grid capped at 8:
    counts against the restatement, cost, point and the tCG invariants by the rule."""
    C = K.matrix(kind, n, d)
    h = _handle(lib, kind, C, d)
    try:
        for p in ps:
            Y0 = K.start(kind, n, d, p)
            Y_ref, f_ref, info = K.restatement(kind, n, d, p)
            _select(h, False)
            h.set_point(Y0)
            assert h.tcg_path() == 0
            st_g, Y_g = _rtr(lib, h, Y0, K.MAXITER)
            e_gen = _relerr(Y_g, Y_ref)
            # the tCG invariants of one iteration on the generic path
            _rtr(lib, h, Y0, 1)
            eta, heta = h.debug_get_tcg_step()
            h.set_point(Y0)
            inv_g = _relerr(heta, h.hessvec(eta))
            tan_g = _relerr(h.proj(eta), eta)
            assert _dev_counts(st_g) == K.counts(info), (p, _dev_counts(st_g), K.counts(info))
            for grid in (0, 8):
                _select(h, True, grid)
                h.set_point(Y0)
                plan = _planned(h, kind, n, d, p, grid)
                assert plan["grid"] % 8 == 0 and plan["slots"] in (1, 2)
                if grid == 8:
                    assert plan["grid"] == 8
                    if n == 343 and p >= 17:
                        assert plan["slots"] == 2 and plan["lpr"] == 16      # 343 blocks on 8 workgroups of 32 per slot
                st_p, Y_p = _rtr(lib, h, Y0, K.MAXITER)
                assert h.tcg_path() == 1, (p, grid)
                e_per = _relerr(Y_p, Y_ref)
                _rtr(lib, h, Y0, 1)
                assert h.tcg_path() == 1, (p, grid)
                eta, heta = h.debug_get_tcg_step()
                _select(h, False)
                h.set_point(Y0)
                inv_p = _relerr(heta, h.hessvec(eta))
                tan_p = _relerr(h.proj(eta), eta)
                print("%s n %d d %d p %2d grid %d (G %d, %d slots): counts %s  point %.1e (generic %.1e)  Heta %.1e (%.1e)  tangent %.1e (%.1e)"
                      % (kind, n, d, p, grid, plan["grid"], plan["slots"], _dev_counts(st_p), e_per, e_gen, inv_p, inv_g, tan_p, tan_g))
                assert _dev_counts(st_p) == _dev_counts(st_g) == K.counts(info), (p, grid)
                assert abs(st_p.cost - f_ref) <= 1e-11 * abs(f_ref)
                assert _rule(e_per, e_gen), (p, grid, e_per, e_gen)
                assert _rule(inv_p, inv_g), (p, grid, inv_p, inv_g)
                assert _rule(tan_p, tan_g), (p, grid, tan_p, tan_g)
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["stiefel", "pose"])
@pytest.mark.parametrize("n,d", K.SHAPES)
def test_sweep_against_the_generic_path_and_the_restatement(lib, kind, n, d):
    _sweep(lib, kind, n, d, K.widths(d))


@pytest.mark.parametrize("case", K.LONG_CASES)
def test_long_cases_counts_and_cost(lib, case):
    """Budgets whose tCG runs up to 20 trips per launch and ends on the kappa / theta test (stop 3) or, rejected iterations
    included, on the boundary: counts of both paths equal the restatement's, the cost to the 1e-11 of the count tests."""
    kind, n, d, p, maxiter = case
    C, Y0 = K.matrix(kind, n, d), K.start(kind, n, d, p)
    _, f_ref, info = K.restatement(*case)
    h = _handle(lib, kind, C, d)
    try:
        _select(h, False)
        st_g, _ = _rtr(lib, h, Y0, maxiter)
        assert _dev_counts(st_g) == K.counts(info)
        for grid, wide in ((0, 0), (8, 0), (0, 1)):                         # planned, capped, and the widest grid (A/B switch)
            _select(h, True, grid)
            h.set_option("block_persist_wide", wide)
            h.set_point(Y0)
            plan = _planned(h, kind, n, d, p, grid, wide)
            if wide:
                assert plan["grid"] >= 64                                    # more workgroups than blocks per slot need: empty chunks too
            st_p, Y_p = _rtr(lib, h, Y0, maxiter)
            assert h.tcg_path() == 1, (grid, wide)
            print(case, "grid", grid, "wide", wide, "device", _dev_counts(st_p), st_p.cost, "restatement", K.counts(info), f_ref)
            assert _dev_counts(st_p) == K.counts(info)
            assert abs(st_p.cost - f_ref) <= 1e-11 * abs(f_ref)
            Y3 = _rot3(kind, Y_p, d)
            assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(d))) < 1e-13
    finally:
        h.close()


# ------------------------------------------------------------------ 3. pose rows
@pytest.mark.parametrize("n,d,degree", [(67, 3, 6), (343, 3, 6)])
def test_zero_free_rows_equal_the_persistent_stiefel_kind(lib, n, d, degree):
    C = sp.csr_matrix(PG.instance(n, d, degree, 0.3)[0])
    keep = np.ones(n * (d + 1), dtype=bool)
    keep[d::d + 1] = False
    Cr = sp.csr_matrix(C[keep][:, keep])                                     # the rotation submatrix, order n d
    Dk = sp.diags(keep.astype(np.float64))
    Cz = sp.csr_matrix(Dk @ C @ Dk)                                          # the pose matrix with zero free rows and columns
    Cz.eliminate_zeros()
    p = 9
    Y = PG.point(n, d, p)
    Yr = np.ascontiguousarray(Y[keep])
    # one trust region for both kinds: the default radius follows the manifold's dimension, which counts the free rows
    radius = dict(Delta_bar=float(np.sqrt(n * (p * d - d * (d + 1) / 2))))
    radius["Delta0"] = radius["Delta_bar"] / 8.0
    h = _handle(lib, "pose", Cz, d)
    hs = _handle(lib, "stiefel", Cr, d)
    try:
        diff = {}
        for on in (False, True):
            for hh in (h, hs):
                _select(hh, on, 8 if on else 0)
            if on:
                h.set_point(Y); hs.set_point(Yr)
                _planned(h, "pose", n, d, p, 8); _planned(hs, "stiefel", n, d, p, 8)
            st, Yp = _rtr(lib, h, Y, K.MAXITER, **radius)
            eta, heta = h.debug_get_tcg_step()
            sts, Ys = _rtr(lib, hs, Yr, K.MAXITER, **radius)
            etas, hetas = hs.debug_get_tcg_step()
            assert h.tcg_path() == hs.tcg_path() == (1 if on else 0)
            assert _dev_counts(st) == _dev_counts(sts)
            diff[on] = (_relerr(Yp[keep], Ys), _relerr(eta[keep], etas), _relerr(heta[keep], hetas))
            assert np.all(eta[~keep] == 0.0) and np.all(heta[~keep] == 0.0)  # exactly zero free rows
        print("pose rows n %d d %d (point, eta, Heta): persistent %s generic %s"
              % (n, d, " ".join("%.1e" % v for v in diff[True]), " ".join("%.1e" % v for v in diff[False])))
        for e_per, e_gen in zip(diff[True], diff[False]):
            assert e_gen < 1e-10, diff                                       # the two problems are the same one on either path
            assert _rule(e_per, e_gen), diff
    finally:
        h.close(); hs.close()


# ------------------------------------------------------------------ 4. ineligible stays right
@pytest.mark.parametrize("kind", ["stiefel", "pose"])
def test_ineligible_handles_take_the_generic_path_bit_for_bit(lib, kind):
    n, d = 67, 3
    C = K.matrix(kind, n, d)
    h = _handle(lib, kind, C, d, pcap=256)
    h0 = _handle(lib, kind, C, d, pcap=256)
    try:
        h.set_option("block_persist", 1)
        for p in (33, 256):                                                  # 33: the first width without a plan
            Y0 = K.ref(kind).point(n, d, p)
            h.set_point(Y0)
            assert h.tcg_path() == 0 and h.persist_form() == -1 and h.block_persist_plan()["eligible"] == 0
            st, Y = _rtr(lib, h, Y0, K.MAXITER)
            st0, Yd = _rtr(lib, h0, Y0, K.MAXITER)
            assert _dev_counts(st) == _dev_counts(st0) and st.cost == st0.cost
            assert np.array_equal(Y, Yd)
        Y0 = K.ref(kind).point(n, d, 8)
        h.set_point(Y0)
        assert h.tcg_path() == 1
        h.set_option("persist", 0)                                           # option on with the persistent kernels off
        assert h.tcg_path() == 0
        st, Y = _rtr(lib, h, Y0, K.MAXITER)
        st0, Yd = _rtr(lib, h0, Y0, K.MAXITER)
        assert _dev_counts(st) == _dev_counts(st0) and np.array_equal(Y, Yd)
        h.set_option("persist", 1)
        assert h.tcg_path() == 1
    finally:
        h.close(); h0.close()


# ------------------------------------------------------------------ 5. fall-back
@pytest.mark.parametrize("kind", ["stiefel", "pose"])
def test_fall_back_after_a_reported_time_out(lib, kind):
    R = K.ref(kind)
    c = R.COUNT_CASE
    C, Y0 = R.count_case()
    _, f_ref, info = R.trustregions(C, Y0, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
    h = _handle(lib, kind, C, c["d"], pcap=c["p"])
    try:
        h.set_option("block_persist", 1)
        h.set_point(Y0)
        assert h.tcg_path() == 1
        h.set_option("debug_fail_persist", 1)
        st = h.rtr(lib.default_opts(maxiter=c["maxiter"], maxinner=c["maxinner"], tolgradnorm=c["tolgradnorm"]))
        assert h.tcg_path() == 0                                             # the handle stays on the chunked path
        assert _dev_counts(st) == R.counts(info)
        assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
    finally:
        h.close()


# ------------------------------------------------------------------ 6. solves
def test_unit_block_diagonal_solve_with_the_option(lib):
    from manisdp_matlab_amd import solvers
    n, d, sigma = 67, 3, 2.0
    C, _, _ = BD.instance(n, d, 6, sigma)
    Y0 = BD.random_point(n, d, d, np.random.default_rng(1))
    Y, obj, data = solvers.ManiSDP_onlyunitblockdiag(C, d, {"Y0": Y0, "block_persist": True}, verbose=False)
    print("unit-block-diagonal solve, persistent tCG: %.10f, %d iterations, p %d, dinf %.1e" % (obj, data["iters"], data["p"], data["dinf"]))
    assert data["status"] == 0 and data["dinf"] < 1e-8
    assert abs(obj - (-794.4145229643)) <= 1e-6 * 794.4145229643


def test_pose_graph_solve_with_the_option(lib):
    from manisdp_matlab_amd import solvers
    n, d = 67, 3
    C = PG.instance(n, d, 6, 0.3)[0]
    Y, obj, data = solvers.ManiSDP_posegraph(C, d, {"block_persist": True}, verbose=False)
    print("pose-graph solve, persistent tCG: %.10f, %d iterations, p %d, dinf %.1e, gap %.1e" % (obj, data["iters"], data["p"], data["dinf"], data["gap"]))
    assert data["status"] == 0 and data["dinf"] < 1e-8 and data["gap"] < 1e-8
    assert abs(obj - 76.1126274793) <= 1e-6 * 76.1126274793


# ------------------------------------------------------------------ 7. benchmark hook
@pytest.mark.parametrize("kind", ["stiefel", "pose"])
def test_bench_hook_leaves_the_handle_usable(lib, kind):
    n, d, p = 101, 2, 9
    C, Y0 = K.matrix(kind, n, d), K.start(kind, n, d, p)
    _, _, info = K.restatement(kind, n, d, p)
    h = _handle(lib, kind, C, d)
    try:
        for on in (False, True):
            _select(h, on)
            h.set_point(Y0)
            assert h.tcg_path() == (1 if on else 0)
            if on:
                _planned(h, kind, n, d, p, 0)
            t = h.bench_tcg_trip(64)
            assert h.tcg_path() == (1 if on else 0)
            print("%s trip, block_persist %d: %.2f us" % (kind, on, t * 1e3))
            assert t > 0
            st, _ = _rtr(lib, h, Y0, K.MAXITER)
            assert h.tcg_path() == (1 if on else 0)
            assert _dev_counts(st) == K.counts(info)
    finally:
        h.close()
