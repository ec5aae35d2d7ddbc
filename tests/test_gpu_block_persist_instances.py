"""Every instance of the block kinds' persistent tCG kernel k_tcg_persist_blk<D, EF, LPR, R> (msdp_blockpersist.hip) that a
handle can select, and the branches of the kernel and of its host side beside the plain trip: the two-slot kernels at every
lanes-per-block count (another gather depth, Heta kept as r - grad for blocks of four rows), two slots on sixteen workgroups, the
step itself against the restatement's tCG, the trust-region options kappa / theta / mininner, a finished solve, fewer blocks than
workgroups, a grid cap that leaves no plan, and block rows without an entry.

The cases, and the CPU conditions on them, are those of tests/block_persist_cases.py and
tests/test_block_persist_cases_host.py; the helpers, the yardstick and the tolerances those of tests/test_gpu_block_persist.py:
counts exact, cost to 1e-11, blocks orthonormal to 1e-13, rounding-level figures e_per <= max(10 e_gen, 1e-12) with e_gen the
generic path's error against the NumPy restatement of the same case.  The reference is always the restatement.  Every
persistent run asserts the planned instance before and tcg_path() == 1 after it."""
import numpy as np
import pytest

import block_persist_cases as K
from test_gpu_block_persist import _dev_counts, _handle, _planned, _relerr, _rot3, _rtr, _rule, _select, _sweep, lib  # noqa: F401

pytestmark = pytest.mark.gpu


def _stats(st):
    return _dev_counts(st) + (st.cost, st.gradnorm, st.Delta, st.cost_evals)


# ------------------------------------------------------------------ 1. two row slots at every LPR, D and EF
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,d", sorted(K.TWO_SLOT_SHAPES))
def test_two_slot_sweep_against_the_generic_path_and_the_restatement(lib, kind, n, d):
    """The sweep of test_gpu_block_persist.py on shapes that take two row slots under the grid cap 8 (and one at the planned
    grid): _planned() holds every run to the instance of the ledger."""
    for p in K.TWO_SLOT_SHAPES[(n, d)]:
        assert K.instance_of(kind, n, d, p, 8)[3] == 2
    _sweep(lib, kind, n, d, K.TWO_SLOT_SHAPES[(n, d)])


@pytest.mark.parametrize("case", K.LONG_TWO_SLOT_CASES)
def test_long_two_slot_cases_counts_and_cost(lib, case):
    """Budgets of 30 to 150 Hess-vecs on two row slots, tCGs of up to 20 trips, rejected iterations, stops 1, 2, 3 and 5; the
    last two cases on sixteen workgroups: counts of both paths equal the restatement's, the cost to 1e-11."""
    kind, n, d, p, maxiter, grid = case
    C, Y0 = K.matrix(kind, n, d), K.start(kind, n, d, p)
    _, f_ref, info = K.restatement(kind, n, d, p, maxiter)
    h = _handle(lib, kind, C, d)
    try:
        _select(h, False)
        st_g, _ = _rtr(lib, h, Y0, maxiter)
        assert h.tcg_path() == 0 and _dev_counts(st_g) == K.counts(info)
        _select(h, True, grid)
        h.set_option("block_persist_wide", 0)
        h.set_point(Y0)
        plan = _planned(h, kind, n, d, p, grid)
        assert plan["slots"] == 2 and plan["grid"] == grid
        st_p, Y_p = _rtr(lib, h, Y0, maxiter)
        assert h.tcg_path() == 1
        print(case, "G", plan["grid"], "lpr", plan["lpr"], "device", _dev_counts(st_p), st_p.cost, "restatement", K.counts(info), f_ref)
        assert _dev_counts(st_p) == K.counts(info)
        assert abs(st_p.cost - f_ref) <= 1e-11 * abs(f_ref)
        Y3 = _rot3(kind, Y_p, d)
        assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(d))) < 1e-13
    finally:
        h.close()


# ------------------------------------------------------------------ 2. the step itself
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,d,p", K.STEP_SHAPES)
def test_step_and_product_equal_the_restatements_tcg(lib, kind, n, d, p):
    """eta and Heta of the first tCG of a call against oracle/manopt_rtr.tCG at the same point, gradient and radius, from the
    random start (a trip or a few) and from the warm start (five trips or more): one slot and two, by the rule."""
    h = _handle(lib, kind, K.matrix(kind, n, d), d)
    try:
        for warm in (False, True):
            Y0 = K.warm_start(kind, n, d, p) if warm else K.start(kind, n, d, p)
            eta_ref, heta_ref, trips, stop = K.first_step(kind, n, d, p, warm)
            _select(h, False)
            st, _ = _rtr(lib, h, Y0, 1)
            assert h.tcg_path() == 0 and (st.hessvecs, st.last_stop_inner) == (trips, stop), (warm, st.hessvecs, st.last_stop_inner, trips, stop)
            eta, heta = h.debug_get_tcg_step()
            e_gen, he_gen = _relerr(eta, eta_ref), _relerr(heta, heta_ref)
            for grid in (0, 8):
                _select(h, True, grid)
                h.set_point(Y0)
                plan = _planned(h, kind, n, d, p, grid)
                assert plan["slots"] == (2 if grid else 1)
                st, _ = _rtr(lib, h, Y0, 1)
                assert h.tcg_path() == 1
                assert (st.hessvecs, st.last_stop_inner) == (trips, stop), (warm, grid, st.hessvecs, st.last_stop_inner, trips, stop)
                eta, heta = h.debug_get_tcg_step()
                e_per, he_per = _relerr(eta, eta_ref), _relerr(heta, heta_ref)
                print("%s n %d d %d p %2d warm %d grid %d (lpr %d, %d slots): %2d trips, stop %d  eta %.1e (generic %.1e)  Heta %.1e (%.1e)"
                      % (kind, n, d, p, warm, grid, plan["lpr"], plan["slots"], trips, stop, e_per, e_gen, he_per, he_gen))
                assert _rule(e_per, e_gen), (warm, grid, e_per, e_gen)
                assert _rule(he_per, he_gen), (warm, grid, he_per, he_gen)
    finally:
        h.close()


# ------------------------------------------------------------------ 3. trust-region options
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,d,p", K.OPTION_SHAPES)
def test_kappa_theta_and_mininner_on_both_paths(lib, kind, n, d, p):
    """kappa, theta and mininner through default_opts(...) against trustregions(...) of the oracle with the same values: stop 4
    behind mininner, norm_r0^theta through pow (theta != 1), stop 3 at the length mininner."""
    maxiter = K.OPTION_MAXITER[kind]
    h = _handle(lib, kind, K.matrix(kind, n, d), d)
    try:
        Y0 = K.start(kind, n, d, p)
        for o in K.OPTION_SETS:
            Y_ref, f_ref, info = K.restatement(kind, n, d, p, maxiter, **o)
            _select(h, False)
            st_g, Y_g = _rtr(lib, h, Y0, maxiter, **o)
            assert h.tcg_path() == 0 and _dev_counts(st_g) == K.counts(info), (o, _dev_counts(st_g), K.counts(info))
            e_gen = _relerr(Y_g, Y_ref)
            for grid in (0, 8):
                _select(h, True, grid)
                h.set_point(Y0)
                plan = _planned(h, kind, n, d, p, grid)
                st_p, Y_p = _rtr(lib, h, Y0, maxiter, **o)
                assert h.tcg_path() == 1
                e_per = _relerr(Y_p, Y_ref)
                print("%s n %d d %d p %2d %s grid %d (%d slots): counts %s  stops %s  point %.1e (generic %.1e)"
                      % (kind, n, d, p, o, grid, plan["slots"], _dev_counts(st_p), sorted(set(info.stop_inner)), e_per, e_gen))
                assert _dev_counts(st_p) == K.counts(info), (o, grid)
                assert abs(st_p.cost - f_ref) <= 1e-11 * abs(f_ref)
                assert _rule(e_per, e_gen), (o, grid, e_per, e_gen)
    finally:
        h.close()


# ------------------------------------------------------------------ 4. edges
@pytest.mark.parametrize("case", K.FINISHED_CASES)
def test_a_finished_solve_is_left_alone(lib, case):
    """A budget that converges, then rtr() again: no iteration, the point bit for bit where it was, the statistics of the
    generic path at the same point, and the handle still on the persistent path."""
    kind, n, d, p, maxiter, tol = case
    _, f_ref, info = K.restatement(kind, n, d, p, maxiter, tol)
    h = _handle(lib, kind, K.matrix(kind, n, d), d)
    try:
        Y0 = K.start(kind, n, d, p)
        _select(h, True)
        h.set_point(Y0)
        _planned(h, kind, n, d, p, 0)
        opts = lib.default_opts(maxiter=maxiter, maxinner=K.MAXINNER, tolgradnorm=tol)
        st = h.rtr(opts)
        assert h.tcg_path() == 1
        assert _dev_counts(st) == K.counts(info) and st.gradnorm < tol and st.iters < maxiter
        assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
        Y1 = h.get_point()
        st2 = h.rtr(opts)                                                    # on the resident point, as a caller would
        assert h.tcg_path() == 1
        assert (st2.iters, st2.hessvecs, st2.accepted, st2.rejected) == (0, 0, 0, 0)
        assert np.array_equal(h.get_point(), Y1)
        st3, Y3 = _rtr(lib, h, Y1, maxiter, tol=tol)                         # and on the same point set anew
        assert h.tcg_path() == 1 and np.array_equal(Y3, Y1)
        _select(h, False)
        st_g, Y_g = _rtr(lib, h, Y1, maxiter, tol=tol)
        assert h.tcg_path() == 0 and np.array_equal(Y_g, Y1)
        print(case, "first call", _dev_counts(st), "again", _stats(st2), "generic", _stats(st_g))
        assert _stats(st2) == _stats(st3) == _stats(st_g)
    finally:
        h.close()


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", K.FEW_BLOCKS)
def test_fewer_blocks_than_workgroups_at_the_planned_grid(lib, kind, n, d):
    """1, 5 and 9 blocks on the eight workgroups of the planned grid (no block_persist_wide): chunks of one block or none, at
    the narrowest and the widest factor."""
    h = _handle(lib, kind, K.matrix(kind, n, d), d)
    try:
        for p in (d, 32):
            Y0 = K.start(kind, n, d, p)
            Y_ref, f_ref, info = K.restatement(kind, n, d, p)
            _select(h, False)
            st_g, Y_g = _rtr(lib, h, Y0, K.MAXITER)
            assert h.tcg_path() == 0 and _dev_counts(st_g) == K.counts(info), (p, _dev_counts(st_g), K.counts(info))
            e_gen = _relerr(Y_g, Y_ref)
            _select(h, True)
            h.set_option("block_persist_wide", 0)
            h.set_point(Y0)
            plan = _planned(h, kind, n, d, p, 0)
            assert plan["grid"] == 8 and plan["slots"] == 1
            st_p, Y_p = _rtr(lib, h, Y0, K.MAXITER)
            assert h.tcg_path() == 1
            e_per = _relerr(Y_p, Y_ref)
            print("%s n %d d %d p %2d: counts %s  cost %.6e  point %.1e (generic %.1e)" % (kind, n, d, p, _dev_counts(st_p), st_p.cost, e_per, e_gen))
            assert _dev_counts(st_p) == K.counts(info), p
            assert abs(st_p.cost - f_ref) <= 1e-11 * abs(f_ref)
            assert _rule(e_per, e_gen), (p, e_per, e_gen)
    finally:
        h.close()


@pytest.mark.parametrize("kind", K.KINDS)
def test_a_grid_cap_without_a_plan_and_the_plan_back(lib, kind):
    """521 blocks of lpr 16 do not fit two slots of eight workgroups: the capped handle is ineligible and equals a handle with the
    option off bit for bit; with the cap taken away the same handle is eligible again (the cached occupancy answer belongs to
    another plan) and matches the restatement."""
    n, d, p = K.CAP_TOO_SMALL
    C, Y0 = K.matrix(kind, n, d), K.start(kind, n, d, p)
    Y_ref, f_ref, info = K.restatement(kind, n, d, p)
    h = _handle(lib, kind, C, d)
    h0 = _handle(lib, kind, C, d)
    try:
        st0, Yd = _rtr(lib, h0, Y0, K.MAXITER)
        assert h0.tcg_path() == 0 and _dev_counts(st0) == K.counts(info)
        e_gen = _relerr(Yd, Y_ref)
        for cap in (8, 0, 8, 0):
            _select(h, True, cap)
            h.set_point(Y0)
            if cap:
                assert K.plan_of(kind, n, d, p, cap) is None
                assert h.block_persist_plan()["eligible"] == 0 and h.tcg_path() == 0 and h.persist_form() == -1
                st, Y = _rtr(lib, h, Y0, K.MAXITER)
                assert h.tcg_path() == 0
                assert _dev_counts(st) == _dev_counts(st0) and st.cost == st0.cost and np.array_equal(Y, Yd)
            else:
                plan = _planned(h, kind, n, d, p, 0)
                assert plan["slots"] == 1 and plan["grid"] == 24
                st, Y = _rtr(lib, h, Y0, K.MAXITER)
                assert h.tcg_path() == 1
                e_per = _relerr(Y, Y_ref)
                print("%s n %d d %d p %d, the cap taken away: counts %s  point %.1e (generic %.1e)" % (kind, n, d, p, _dev_counts(st), e_per, e_gen))
                assert _dev_counts(st) == K.counts(info)
                assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
                assert _rule(e_per, e_gen), (e_per, e_gen)
    finally:
        h.close(); h0.close()


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n,d,p", K.MASKED_SHAPES)
def test_block_rows_without_an_entry(lib, kind, n, d, p):
    """About a quarter of the blocks removed from the cost matrix, rows and columns: their block rows are empty (k0 == k1 in the
    gather), those of their neighbours short.  Counts against the restatement, the point by the rule, on one slot and two; where
    the gradient of a removed block is zero (the Stiefel kind) its rows of eta and Heta are exactly zero."""
    C = K.masked_matrix(kind, n, d)
    gone = np.repeat(~K.block_mask(n), K.blk(kind, d))
    Y0 = K.start(kind, n, d, p)
    Y_ref, f_ref, info = K.restatement(kind, n, d, p, masked=True)
    h = _handle(lib, kind, C, d)
    try:
        _select(h, False)
        st_g, Y_g = _rtr(lib, h, Y0, K.MAXITER)
        assert h.tcg_path() == 0 and _dev_counts(st_g) == K.counts(info), (_dev_counts(st_g), K.counts(info))
        e_gen = _relerr(Y_g, Y_ref)
        for grid in (0, 8):
            _select(h, True, grid)
            h.set_point(Y0)
            plan = _planned(h, kind, n, d, p, grid)
            assert plan["slots"] == (2 if grid else 1)
            st_p, Y_p = _rtr(lib, h, Y0, K.MAXITER)
            assert h.tcg_path() == 1
            e_per = _relerr(Y_p, Y_ref)
            _rtr(lib, h, Y0, 1)
            assert h.tcg_path() == 1
            eta, heta = h.debug_get_tcg_step()
            print("%s n %d d %d p %d, %d blocks removed, grid %d (%d slots): counts %s  point %.1e (generic %.1e)  removed rows of eta, Heta %.1e %.1e"
                  % (kind, n, d, p, gone.sum() // K.blk(kind, d), grid, plan["slots"], _dev_counts(st_p), e_per, e_gen,
                     np.max(np.abs(eta[gone])), np.max(np.abs(heta[gone]))))
            assert _dev_counts(st_p) == K.counts(info), grid
            assert abs(st_p.cost - f_ref) <= 1e-11 * abs(f_ref)
            assert _rule(e_per, e_gen), (grid, e_per, e_gen)
            assert np.linalg.norm(eta) > 0
            if kind == "stiefel":
                assert np.all(eta[gone] == 0.0) and np.all(heta[gone] == 0.0)
    finally:
        h.close()
