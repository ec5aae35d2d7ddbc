"""The one-reduction tCG trip (msdp_pipe.h) stores its rows of H md, the refresh rows and, in the fused launch, the proposal's rows
and its gradient's rows UNCONDITIONALLY: a lane without a row or without columns is kept out of the exchange buffer by the range check
of the store descriptor (num_records = the workgroup's last row + 1, bit 31 of the offset for a lane without columns), not by EXEC.
A store that is wrongly kept lands in the bytes of a neighbour's row (the next row's columns, or the first rows of the next workgroup's
chunk); a store that is wrongly dropped leaves a row of the last trip behind.  Either changes the products of the next trip, so the
oracle's single tCG (counts exact, cost and gradient norm to rounding) catches it, and so does the comparison of the fused launch (the
five-column instance at 8 lanes per row keeps its guarded stores there) with per-iteration launches.

The persistent kernel chooses its own grid (persist_grid in msdp_persist.hip; the option `grid` belongs to the row-parallel kernels and
does not reach it): the fewest workgroups, in multiples of 8, whose row slots hold the rows -- on any device with 16 CUs or more

    shape      n     p         instance    workgroups   rows per workgroup (msdp_chunk_rows)
    (33, 37)   1221  17 20 31  <16, 5, 3>  16           77 in the first five chunks, 76 in the others: three slots of 32, the third with
                                                        13 / 12 rows; row stride 18, 20 and 32 doubles of the 32 that 16
                                                        lanes hold: lanes without columns at p = 17 and 20, a pad column at 31
    (20, 30)   600   3 10      <8, 5, 2>   8            75: two slots of 64, the second with 11 rows; ld = 4 and 10 of 16
    (20, 30)   600   32        <16, 5, 3>  8            75: 32 + 32 + 11, every lane with columns
    (7, 11)    77    32        <16, 5, 3>  8            10 in the first five chunks, 9 in the others: waves 0 and 1 full (4 rows each),
                                                        wave 2 with 2 / 1 rows, waves 3 to 7 and the second and third slot without rows
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (shape, p, pipe_refresh): pipe_refresh = 2 publishes the refresh rows on every second trip, 4 on every fourth (16: the default, which
# the short tCGs of these sizes do not reach)
CASES = [((33, 37), 17, 16), ((33, 37), 20, 4), ((33, 37), 31, 2), ((20, 30), 3, 16), ((20, 30), 10, 2), ((20, 30), 32, 4), ((7, 11), 32, 4)]


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _problem(shape, p):
    from manisdp_matlab_amd import problems
    C = problems.toroidal_grid_maxcut(shape[0], shape[1], seed=3)
    rng = np.random.default_rng(11)
    Y = rng.standard_normal((C.shape[0], p))
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    return C, Y


@pytest.mark.parametrize("shape,p,refresh", CASES)
def test_unconditional_row_stores_match_oracle(lib, shape, p, refresh):
    """ONE tCG (maxiter = 1) for every inner-iteration cap, fused and as per-iteration launches, against the oracle's tCG: the checks
    of test_persistent_tcg_matches_oracle."""
    from oracle import manisdp_ref as R, manopt_rtr
    C, Y = _problem(shape, p)
    n = C.shape[0]
    prob = R._OnlyUnitDiagProblem(C, n, p, q1="correct")
    # from the random point the first tCG leaves through the trust region's boundary within a trip or two; from the oracle's point after
    # six TR iterations it runs 7 trips to its cap, and 9 to 13 to the boundary (5 and 5 at p = 3): refresh trips at the intervals 2 and 4
    Y1 = manopt_rtr.trustregions(prob, Y.copy(), 6, 40, 1e-8)[0]
    starts = [(Y, (1, 2, 7, 100)), (Y1, (7, 20))]
    refs = {(s, m): manopt_rtr.trustregions(prob, Ys.copy(), 1, m, 1e-8) for s, (Ys, caps) in enumerate(starts) for m in caps}
    h = lib.Handle.onlyunitdiag(C, pcap=p)
    h.set_point(Y)
    assert h.tcg_path() == 1, "persistent kernel not selected"
    h.set_option("persist_pipe", 1)
    h.set_option("pipe_refresh", refresh)
    for fused in (1, 0):
        h.set_option("fused_rtr", fused)
        h.set_point(Y)
        assert h.persist_form() == 2, "one-reduction trip not selected"
        for s, maxinner in refs:
            h.set_point(starts[s][0])
            st = h.rtr(lib.default_opts(maxiter=1, maxinner=maxinner, tolgradnorm=1e-8))
            _, f_ref, info = refs[(s, maxinner)]
            dc = abs(st.cost - f_ref) / max(1.0, abs(f_ref))
            dg = abs(st.gradnorm - info.gradnorm) / max(1.0, info.gradnorm)
            print(f"{shape} p={p} refresh={refresh} fused={fused} start={s} maxinner={maxinner}: hessvecs {st.hessvecs} / {info.hessvecs}, "
                  f"stop {st.last_stop_inner} / {info.stop_inner[-1]}, cost {dc:.2e}, gradnorm {dg:.2e}")
            assert st.hessvecs == info.hessvecs
            assert st.last_stop_inner == info.stop_inner[-1]
            assert dc < 1e-11
            assert dg < 1e-8
    h.close()


@pytest.mark.parametrize("shape,p,refresh", CASES)
def test_unconditional_row_stores_fused_matches_per_iteration(lib, shape, p, refresh):
    """Six TR iterations -- accepted and rejected steps, the role swap of the point's buffers, the refresh regions -- in one launch and
    as one launch per iteration: the checks of test_fused_rtr_kernel_matches_per_iteration_path."""
    C, Y = _problem(shape, p)
    out = []
    for fused in (0, 1):
        h = lib.Handle.onlyunitdiag(C, pcap=p)
        h.set_option("persist_pipe", 1)
        h.set_option("pipe_refresh", refresh)
        h.set_option("fused_rtr", fused)
        h.set_point(Y)
        assert h.tcg_path() == 1 and h.persist_form() == 2
        st = h.rtr(lib.default_opts(maxiter=6, maxinner=40, tolgradnorm=1e-9))
        out.append((st.iters, st.hessvecs, st.accepted, st.rejected, st.cost, st.gradnorm, h.cost()))
        h.close()
    a, b = out
    print(f"{shape} p={p} refresh={refresh}: per-iteration {a[:4]}, fused {b[:4]}, cost {abs(a[4] - b[4]):.2e}, gradnorm {abs(a[5] - b[5]):.2e}")
    assert a[:4] == b[:4]
    assert abs(a[4] - b[4]) < 1e-11 * max(1.0, abs(a[4])) and abs(a[5] - b[5]) < 1e-8 * max(1.0, a[5])
    assert abs(b[6] - b[4]) < 1e-10 * max(1.0, abs(b[4]))       # the resident point IS the accepted one
