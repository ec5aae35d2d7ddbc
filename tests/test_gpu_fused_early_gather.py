"""The fused one-reduction tCG trip at 16 lanes per row (msdp_pipe.h, `k_tcg_pipe_obl<16, 5, 3, ..., FUSE>`) requests the NEXT trip's
gather inside the reduction, as soon as every workgroup has posted, and keeps its two product recurrences (C md, C tangent(r)) in LDS
between trips instead of in registers.  What can go wrong:

  - a request that runs in front of a refresh trip, or is not skipped exactly there, hands the next trip rows of the wrong region;
  - a way out of the trip loop with loads in flight (the inner cap, the boundary / negative curvature, the model test, convergence)
    leaves `have_x` set, and the next tCG of the launch folds rows of the last one;
  - a tCG that restarts at the SAME point (a rejected step) finds the parked vectors of the tCG before it;
  - a request that runs ahead of a neighbour's store of the rows it asks for: a difference between two runs of the same call.

Shapes (tests/test_gpu_fused_row_bounds.py documents them; the persistent kernel chooses its own grid), the smallest that reach the
instance:

    (7, 11)   p = 32       8 workgroups of 9 or 10 rows: whole waves and whole row slots without rows
    (33, 37)  p = 17, 20   16 workgroups, lanes without columns, a third row slot with 12 or 13 rows

Bounds against the oracle's tCG, those of tests/test_gpu_fused_row_bounds.py: counts and stop codes exact, cost to 1e-11 relative,
gradient norm to 1e-8 relative.  Every run asserts the path taken (tcg_path() == 1, persist_form() == 2): a silent fall-back fails."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [((7, 11), 32), ((33, 37), 17), ((33, 37), 20)]
REFRESH = [2, 3, 4, 64]          # prefetched trips and refresh trips alternating (2), mixed (3, 4), no refresh trip ever (64)
CAPS = (1, 2, 3, 7, 20)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


@functools.lru_cache(maxsize=None)
def _reference(shape, p):
    """The problem, the two start points (cold; the oracle's point after six TR iterations), the oracle's single tCGs from them for
    every inner cap, and its six TR iterations from a start radius of Delta_bar -- computed once per (shape, p), never written to."""
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
    single = {}
    for s in range(2):
        for m in CAPS:
            _, f_ref, info = manopt_rtr.trustregions(prob, starts[s].copy(), 1, m, 1e-8)
            single[(s, m)] = (f_ref, info.gradnorm, info.hessvecs, info.stop_inner[-1])
    # six TR iterations from the largest start radius: the oracle over-reaches and rejects (asserted by the test that relies on it)
    delta_bar = prob.M.typicaldist()
    six = []
    for s in range(2):
        _, f_ref, info = manopt_rtr.trustregions(prob, starts[s].copy(), 6, 40, 1e-9, Delta0=delta_bar)
        six.append((info.iters, info.hessvecs, info.accepted, info.rejected, info.stop_inner[-1], f_ref, info.gradnorm,
                    tuple(info.stop_inner)))
    for a in starts:
        a.setflags(write=False)
    return C, starts, single, delta_bar, tuple(six)


def _handle(lib, C, p, refresh, fused):
    h = lib.Handle.onlyunitdiag(C, pcap=p)
    h.set_option("persist_pipe", 1)
    h.set_option("pipe_refresh", refresh)
    h.set_option("fused_rtr", fused)
    return h


def _on_path(h):
    assert h.tcg_path() == 1 and h.persist_form() == 2, "one-reduction persistent trip not selected"


def test_tcgs_leave_the_trip_loop_every_way():
    """Precondition of the tests below, on the CPU: the ways out of the trip loop that the oracle's tCGs take on these shapes.  The
    single tCGs end at their cap (stop 5), at the boundary (2) and at negative curvature (1); the tCGs of the six-iteration runs also
    end by convergence (4, theta = 1: the linear criterion).  The cap, convergence and the model test leave behind the model test, with
    two or three batches of the next gather requested; the boundary and negative curvature in front of it, with one.  The model test
    (6) and the superlinear criterion (3, needs theta > 1) fire on none of these instances in the oracle either: they leave through
    the same `break` statements as 5 and 4, with the same batches requested."""
    stops = set()
    for shape, p in SHAPES:
        _, _, single, _, six = _reference(shape, p)
        stops |= {v[3] for v in single.values()}
        for ref in six:
            stops |= set(ref[7])
    assert {1, 2, 4, 5} <= stops, stops


@pytest.mark.parametrize("refresh", REFRESH)
@pytest.mark.parametrize("shape,p", SHAPES)
def test_single_tcg_matches_oracle_for_every_inner_cap(lib, shape, p, refresh):
    """ONE tCG (maxiter = 1) for the inner caps 1, 2, 3, 7 and 20, from the cold start and from the oracle's point after six TR
    iterations, fused and as per-iteration launches, against the oracle's tCG."""
    C, starts, single, _, _ = _reference(shape, p)
    for fused in (1, 0):
        h = _handle(lib, C, p, refresh, fused)
        h.set_point(starts[0])
        _on_path(h)
        for (s, maxinner), (f_ref, g_ref, hv_ref, stop_ref) in single.items():
            h.set_point(starts[s])
            st = h.rtr(lib.default_opts(maxiter=1, maxinner=maxinner, tolgradnorm=1e-8))
            _on_path(h)
            dc = abs(st.cost - f_ref) / max(1.0, abs(f_ref))
            dg = abs(st.gradnorm - g_ref) / max(1.0, g_ref)
            what = f"{shape} p={p} refresh={refresh} fused={fused} start={s} maxinner={maxinner}"
            print(f"{what}: hessvecs {st.hessvecs} / {hv_ref}, stop {st.last_stop_inner} / {stop_ref}, cost {dc:.2e}, gradnorm {dg:.2e}")
            assert st.hessvecs == hv_ref, what
            assert st.last_stop_inner == stop_ref, what
            assert dc < 1e-11, what
            assert dg < 1e-8, what
        h.close()


@pytest.mark.parametrize("refresh", REFRESH)
@pytest.mark.parametrize("shape,p", SHAPES)
def test_six_iterations_with_a_rejected_step_in_one_launch(lib, shape, p, refresh):
    """Six TR iterations from a start radius of Delta_bar in ONE fused launch against one launch per iteration and against the oracle:
    the same counts.  The oracle rejects at least one step from each start (the precondition, checked on the CPU), and so must the fused
    launch: the tCG behind a rejected step restarts at the same point, with the parked vectors and `have_x` reset."""
    C, starts, _, delta_bar, six = _reference(shape, p)
    for s in range(2):
        ref = six[s]
        assert ref[3] >= 1, f"precondition: the oracle rejects no step on {shape} p={p} start={s}"
        out = []
        for fused in (0, 1):
            h = _handle(lib, C, p, refresh, fused)
            h.set_point(starts[s])
            _on_path(h)
            st = h.rtr(lib.default_opts(maxiter=6, maxinner=40, tolgradnorm=1e-9, Delta0=delta_bar))
            _on_path(h)
            out.append((st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner, st.cost, st.gradnorm, h.cost()))
            h.close()
        a, b = out
        print(f"{shape} p={p} refresh={refresh} start={s}: oracle {ref[:5]}, per-iteration {a[:5]}, fused {b[:5]}, "
              f"cost {abs(b[5] - ref[5]):.2e}, gradnorm {abs(b[6] - ref[6]):.2e}")
        assert a[:5] == b[:5]
        assert b[:5] == ref[:5]
        assert b[3] >= 1, "no rejected step inside the fused launch"
        assert abs(b[5] - ref[5]) < 1e-11 * max(1.0, abs(ref[5])) and abs(b[6] - ref[6]) < 1e-8 * max(1.0, ref[6])
        assert abs(a[5] - b[5]) < 1e-11 * max(1.0, abs(a[5])) and abs(a[6] - b[6]) < 1e-8 * max(1.0, a[6])
        assert abs(b[7] - b[5]) < 1e-10 * max(1.0, abs(b[5]))       # the resident point IS the accepted one


@pytest.mark.parametrize("refresh", REFRESH)
@pytest.mark.parametrize("p", [17, 20])
def test_fused_call_repeats_bit_for_bit(lib, p, refresh):
    """The same fused call twice on the 16-workgroup shape: a request that ran ahead of a neighbour's store, or anything the first call
    left behind (parked vectors, rows in flight), shows as a difference between the runs."""
    C, starts, _, delta_bar, _ = _reference((33, 37), p)
    h = _handle(lib, C, p, refresh, 1)
    got = []
    for _ in range(2):
        h.set_point(starts[1])
        _on_path(h)
        st = h.rtr(lib.default_opts(maxiter=6, maxinner=40, tolgradnorm=1e-9, Delta0=delta_bar))
        _on_path(h)
        got.append(((st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner, st.cost, st.gradnorm, st.Delta), h.get_point()))
    h.close()
    assert got[0][0] == got[1][0]
    assert np.all(np.isfinite(got[0][1]))
    assert np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("shape,p", SHAPES)
def test_stopping_test_with_theta_above_one(lib, shape, p):
    """theta = 2: the stopping test's norm_r0 ^ theta, which this instance forms once per tCG outside its trips (with theta = 1, the
    default of every other test here, that code is never reached).  Three TR iterations from the oracle's point after six, fused and
    per-iteration, against the oracle with the same theta."""
    from oracle import manisdp_ref as R, manopt_rtr
    C, starts, _, _, _ = _reference(shape, p)
    prob = R._OnlyUnitDiagProblem(C, C.shape[0], p, q1="correct")
    _, f_ref, info = manopt_rtr.trustregions(prob, starts[1].copy(), 3, 40, 1e-9, theta=2.0)
    ref = (info.iters, info.hessvecs, info.accepted, info.rejected, info.stop_inner[-1])
    for fused in (1, 0):
        h = _handle(lib, C, p, 4, fused)
        h.set_point(starts[1])
        _on_path(h)
        st = h.rtr(lib.default_opts(maxiter=3, maxinner=40, tolgradnorm=1e-9, theta=2.0))
        _on_path(h)
        h.close()
        got = (st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner)
        print(f"{shape} p={p} theta=2 fused={fused}: {got} / oracle {ref}, cost {abs(st.cost - f_ref):.2e}")
        assert got == ref
        assert abs(st.cost - f_ref) < 1e-11 * max(1.0, abs(f_ref))
        assert abs(st.gradnorm - info.gradnorm) < 1e-8 * max(1.0, info.gradnorm)
