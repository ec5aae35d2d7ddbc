"""The one-reduction persistent tCG (msdp_pipe.h) forms its gather addresses from byte offsets laid down at set-up and masks idle
lanes under one workgroup-uniform branch.  Whole rtr() calls against the oracle on the smallest shapes at which that addressing can
go wrong: several workgroups (the grid has eight at least, so a few hundred rows leave each with 25 to 38), both lane widths
(16 lanes per row at p = 17..32, 8 at p <= 16), lane groups with idle lanes (p = 17: ld = 18 of 32 columns, p = 8: 8 of 16), a
capacity wider than the point (pcap = 32 > p), row slots that are partly or wholly empty, waves without any row, rows of fewer than
five entries (empty ELL slots), refresh trips (regions 2 and 3 of the exchange buffer), the fused launch (regions 4..6) and
per-iteration launches -- and the largest n x ld the <16, 5, 3> instance accepts, where the offsets in the last region are largest.

Tolerances.  Counts, stop codes and accept / reject decisions are exact.  Cost and gradient norm: those of
tests/test_gpu_onlyunitdiag.py for a tCG against the oracle's (1e-11 and 1e-8, relative to max(1, .)).  The point: the step of a
tCG of up to 12 trips carries the recurrences' drift of C tangent(r) and C md, 4e-11 relative after 50 trips at the default refresh
(msdp_pipe.h, tools/pipe_drift_probe.py), and three TR iterations add up: 1e-9 relative to |Y| = sqrt(n)."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _point(n, p, seed):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((n, p))
    return Y / np.linalg.norm(Y, axis=1, keepdims=True)


def _ring(n, seed):
    """Symmetric C of three entries per row (a ring + the diagonal): two of the five ELL slots of every row are empty."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    j = (i + 1) % n
    w = rng.standard_normal(n)
    return sp.csr_matrix((np.concatenate([w, w, rng.standard_normal(n)]), (np.concatenate([i, j, i]), np.concatenate([j, i, i]))), shape=(n, n))


def _cost_matrix(kind):
    from manisdp_matlab_amd import problems
    if kind == "grid300":       # 37 / 38 rows per workgroup: the second row slot of 32 (16 lanes per row) has waves without rows, the third is empty
        return problems.toroidal_grid_maxcut(15, 20, seed=3)
    if kind == "grid200":       # 25 rows per workgroup: less than one row slot -- wave 6 holds one row, wave 7 none at all
        return problems.toroidal_grid_maxcut(10, 20, seed=5)
    if kind == "ring301":       # odd row count (chunks of 38 and 37), three entries per row
        return _ring(301, seed=4)
    raise ValueError(kind)


_REFS = {}
_STARTS = {}


def _start(kind, C, p, warm):
    """The starting point: a random point moved `warm` TR iterations towards the optimum by the oracle -- from a random point the
    first tCGs end at the trust-region boundary after one or two trips, from here they run to the inner cap (refresh trips included)."""
    from oracle import manisdp_ref as R, manopt_rtr
    key = (kind, p)
    if key not in _STARTS:
        prob = R._OnlyUnitDiagProblem(C, C.shape[0], p, q1="correct")
        x, _, _ = manopt_rtr.trustregions(prob, _point(C.shape[0], p, seed=11), warm, 20, 1e-8)
        _STARTS[key] = np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True))
    return _STARTS[key]


def _oracle(kind, C, Y, p, maxiter, maxinner):
    from oracle import manisdp_ref as R, manopt_rtr
    key = (kind, p, maxiter, maxinner)
    if key not in _REFS:
        prob = R._OnlyUnitDiagProblem(C, C.shape[0], p, q1="correct")
        _REFS[key] = manopt_rtr.trustregions(prob, Y.copy(), maxiter, maxinner, 1e-8)
    return _REFS[key]


def _solve_and_compare(lib, kind, C, p, fused, refresh, maxiter, maxinner, warm, min_trips, check_point=True):
    Y = _start(kind, C, p, warm)
    h = lib.Handle.onlyunitdiag(C, pcap=32)
    try:
        h.set_option("persist_pipe", 1)
        h.set_option("fused_rtr", fused)
        if refresh is not None:
            h.set_option("pipe_refresh", refresh)
        h.set_point(Y)
        assert h.tcg_path() == 1, "persistent kernel not selected"
        assert h.persist_form() == 2, "one-reduction trip not selected"
        st = h.rtr(lib.default_opts(maxiter=maxiter, maxinner=maxinner, tolgradnorm=1e-8))
        x_ref, f_ref, info = _oracle(kind, C, Y, p, maxiter, maxinner)
        X = h.get_point()
        print(f"{kind} p={p} fused={fused} refresh={refresh}: iters {st.iters}/{info.iters} hessvecs {st.hessvecs}/{info.hessvecs} "
              f"acc {st.accepted}/{info.accepted} rej {st.rejected}/{info.rejected} stop {st.last_stop_inner}/{info.stop_inner[-1]} "
              f"cost err {abs(st.cost - f_ref) / max(1.0, abs(f_ref)):.2e} gradnorm err {abs(st.gradnorm - info.gradnorm) / max(1.0, info.gradnorm):.2e} "
              f"point err {np.linalg.norm(X - x_ref) / np.linalg.norm(x_ref):.2e}")
        assert info.hessvecs >= min_trips, "the case does not reach the trips it is meant to cover"
        assert (st.iters, st.hessvecs, st.accepted, st.rejected) == (info.iters, info.hessvecs, info.accepted, info.rejected)
        assert st.last_stop_inner == info.stop_inner[-1]
        assert abs(st.cost - f_ref) < 1e-11 * max(1.0, abs(f_ref))
        assert abs(st.gradnorm - info.gradnorm) < 1e-8 * max(1.0, info.gradnorm)
        assert np.allclose(np.linalg.norm(X, axis=1), 1.0, atol=1e-14)
        if check_point:
            assert np.linalg.norm(X - x_ref) < 1e-9 * np.linalg.norm(x_ref)
    finally:
        h.close()


# (kind, p, fused launch, pipe_refresh or None for the default)
@pytest.mark.parametrize("kind,p,fused,refresh", [
    ("grid300", 32, 1, 4),          # every lane has columns; refresh trips: regions 2 and 3 are gathered
    ("grid300", 17, 1, None),       # ld = 18: seven of sixteen lanes idle
    ("grid300", 16, 1, None),       # eight lanes per row, none idle
    ("grid300", 8, 1, 4),           # eight lanes per row, four idle
    ("grid300", 32, 0, None),       # per-iteration launches
    ("grid300", 17, 0, 4),
    ("grid300", 8, 0, None),
    ("grid200", 32, 1, None),       # a wave without rows
    ("grid200", 17, 0, None),
    ("grid200", 16, 0, 4),
    ("ring301", 17, 1, 4),          # empty ELL slots
    ("ring301", 8, 0, None),
    ("ring301", 32, 0, 4),
])
def test_rtr_matches_oracle_on_small_grids(lib, kind, p, fused, refresh):
    """Three TR iterations of up to 12 trips each: counts and decisions exact, cost, gradient norm and point to rounding."""
    _solve_and_compare(lib, kind, _cost_matrix(kind), p, fused, refresh, maxiter=3, maxinner=12, warm=8, min_trips=15)


@pytest.mark.parametrize("fused", [1, 0])
def test_largest_rows_times_width_of_the_three_slot_instance(lib, fused):
    """n = 24 576 = 256 workgroups x 96 row slots at ld = 32: the largest exchange buffer the <16, 5, 3> instances admit (6.3 MB per
    region, seven regions in the fused launch).  Two TR iterations of up to three trips (the second trip publishes the refresh rows, the third gathers them); cost and gradient norm against the oracle."""
    from manisdp_matlab_amd import problems
    C = problems.toroidal_grid_maxcut(128, 192, seed=7)
    _solve_and_compare(lib, "grid24576", C, 32, fused, 2, maxiter=2, maxinner=3, warm=4, min_trips=5, check_point=False)
