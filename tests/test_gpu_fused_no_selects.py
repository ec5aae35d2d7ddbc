"""The one-reduction tCG trip (msdp_pipe.h) without the selects of round 8: the rows of H md carry no select in any instance (the
mask of lanes without columns sits under one workgroup-uniform branch), the refresh rows are published in one block behind the row
loop on a countdown that restarts with every tCG, and the TR tail of the fused launches relies on the invariants of set-up -- exact
zeros in a lane without a row or without columns -- instead of selects on the proposal's rows, its gradient's rows and the slot's eG.
What can go wrong: a lane without columns inside a live row, or a row slot past the workgroup's last row (x = 0 and a row norm of 0: 0 / 0
in the tail), feeds something that is not an exact zero -- or a NaN -- into LDS, a group sum or the iteration's reduction; the countdown
publishes on other trips than `(j + 1) % pipe_refresh == 0` did, or does not restart with the next tCG of a fused launch.

Shapes (tests/test_gpu_fused_row_bounds.py documents them; the persistent kernel chooses its own grid):

    (33, 37)  p = 17, 20   <16, 5, 3>, 16 workgroups: lanes without columns inside live rows, a third row slot with 12 or 13 rows
    (7, 11)   p = 32       <16, 5, 3>, 8 workgroups of 9 or 10 rows: whole waves and whole row slots without rows (the 0 / 0 of the tail)
    (20, 30)  p = 3, 10    <8, 5, 2>, 8 workgroups, two row slots of 64, the second with 11 rows; 2 or 5 of 8 lanes with columns: the
                           instances at 8 lanes per row take all three pieces too (fused: guarded stores, not the descriptor's)

pipe_refresh = 2, 3 (odd) and 4 publish several times inside the tCGs that start at the oracle's point after six TR iterations (7 trips to
the cap, 9 to 13 to the boundary); 64 is more than any tCG here runs: the countdown never fires.  The bounds are those of
tests/test_gpu_fused_row_bounds.py: counts and stop codes exact, cost to 1e-11 and gradient norm to 1e-8 relative."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (shape, p, pipe_refresh)
CASES = [((33, 37), 17, 2), ((33, 37), 17, 3), ((33, 37), 20, 4), ((33, 37), 20, 64),
         ((7, 11), 32, 2), ((7, 11), 32, 3), ((20, 30), 3, 3), ((20, 30), 10, 2), ((20, 30), 10, 4)]


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


@functools.lru_cache(maxsize=None)
def _reference(shape, p):
    """The problem, the two start points and the oracle's single tCGs from them -- computed once per (shape, p), never written to."""
    from manisdp_matlab_amd import problems
    from oracle import manisdp_ref as R, manopt_rtr
    C = problems.toroidal_grid_maxcut(shape[0], shape[1], seed=3)
    n = C.shape[0]
    rng = np.random.default_rng(11)
    Y = rng.standard_normal((n, p))
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    prob = R._OnlyUnitDiagProblem(C, n, p, q1="correct")
    Y1 = manopt_rtr.trustregions(prob, Y.copy(), 6, 40, 1e-8)[0]
    starts = (Y, Y1)
    caps = ((1, 2, 7), (7, 20))
    refs = {}
    for s in range(2):
        for m in caps[s]:
            _, f_ref, info = manopt_rtr.trustregions(prob, starts[s].copy(), 1, m, 1e-8)
            refs[(s, m)] = (f_ref, info.gradnorm, info.hessvecs, info.stop_inner[-1])
    for a in starts:
        a.setflags(write=False)
    return C, starts, refs


def _handle(lib, C, p, refresh, fused):
    h = lib.Handle.onlyunitdiag(C, pcap=p)
    h.set_option("persist_pipe", 1)
    h.set_option("pipe_refresh", refresh)
    h.set_option("fused_rtr", fused)
    return h


def _check_point(h, what):
    Yg = h.get_point()
    assert np.all(np.isfinite(Yg)), what
    assert np.abs(np.linalg.norm(Yg, axis=1) - 1.0).max() <= 1e-14, what


@pytest.mark.parametrize("shape,p,refresh", CASES)
def test_single_tcg_matches_oracle(lib, shape, p, refresh):
    """ONE tCG (maxiter = 1) for every inner-iteration cap, fused and as per-iteration launches, against the oracle's tCG."""
    C, starts, refs = _reference(shape, p)
    for fused in (1, 0):
        h = _handle(lib, C, p, refresh, fused)
        h.set_point(starts[0])
        assert h.tcg_path() == 1 and h.persist_form() == 2, "one-reduction persistent trip not selected"
        for (s, maxinner), (f_ref, g_ref, hv_ref, stop_ref) in refs.items():
            h.set_point(starts[s])
            st = h.rtr(lib.default_opts(maxiter=1, maxinner=maxinner, tolgradnorm=1e-8))
            dc = abs(st.cost - f_ref) / max(1.0, abs(f_ref))
            dg = abs(st.gradnorm - g_ref) / max(1.0, g_ref)
            what = f"{shape} p={p} refresh={refresh} fused={fused} start={s} maxinner={maxinner}"
            print(f"{what}: hessvecs {st.hessvecs} / {hv_ref}, stop {st.last_stop_inner} / {stop_ref}, cost {dc:.2e}, gradnorm {dg:.2e}")
            assert np.isfinite(st.cost) and np.isfinite(st.gradnorm), what
            assert st.hessvecs == hv_ref, what
            assert st.last_stop_inner == stop_ref, what
            assert dc < 1e-11, what
            assert dg < 1e-8, what
            _check_point(h, what)
        h.close()


@pytest.mark.parametrize("shape,p,refresh", CASES)
def test_fused_matches_per_iteration_over_six_iterations(lib, shape, p, refresh):
    """Six TR iterations in one launch and as one launch per iteration, from the random point (short first tCGs, rejected steps) and
    from the oracle's point after six iterations (tCGs that cross several refresh trips each: the countdown restarts six times inside
    the fused launch, and every per-iteration launch starts its own): the same counts."""
    C, starts, _ = _reference(shape, p)
    for s in range(2):
        out = []
        for fused in (0, 1):
            h = _handle(lib, C, p, refresh, fused)
            h.set_point(starts[s])
            assert h.tcg_path() == 1 and h.persist_form() == 2
            st = h.rtr(lib.default_opts(maxiter=6, maxinner=40, tolgradnorm=1e-9))
            what = f"{shape} p={p} refresh={refresh} start={s} fused={fused}"
            assert np.isfinite(st.cost) and np.isfinite(st.gradnorm), what
            _check_point(h, what)
            out.append((st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner, st.cost, st.gradnorm, h.cost()))
            h.close()
        a, b = out
        print(f"{shape} p={p} refresh={refresh} start={s}: per-iteration {a[:5]}, fused {b[:5]}, cost {abs(a[5] - b[5]):.2e}, "
              f"gradnorm {abs(a[6] - b[6]):.2e}")
        assert a[:5] == b[:5]
        assert abs(a[5] - b[5]) < 1e-11 * max(1.0, abs(a[5])) and abs(a[6] - b[6]) < 1e-8 * max(1.0, a[6])
        assert abs(b[7] - b[5]) < 1e-10 * max(1.0, abs(b[5]))       # the resident point IS the accepted one


@pytest.mark.parametrize("shape,p,refresh", CASES)
def test_fused_call_repeats_bit_for_bit(lib, shape, p, refresh):
    """The same fused call twice on ONE handle: nothing of the first call -- the refresh regions, the proposal's rows, a countdown --
    reaches the second; the points are equal bit for bit."""
    C, starts, _ = _reference(shape, p)
    h = _handle(lib, C, p, refresh, 1)
    got = []
    for _ in range(2):
        h.set_point(starts[1])
        st = h.rtr(lib.default_opts(maxiter=6, maxinner=40, tolgradnorm=1e-9))
        got.append(((st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner, st.cost, st.gradnorm), h.get_point()))
    h.close()
    assert got[0][0] == got[1][0]
    assert np.all(np.isfinite(got[0][1]))
    assert np.array_equal(got[0][1], got[1][1])
