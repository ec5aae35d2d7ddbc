"""The wide plan of the fused own-column launch (msdp_pipe.h `k_tcg_pipe_ws`, option `pipe_wide`, default 1; fused_grid in
msdp_persist.hip): the fewest workgroups, in multiples of 8, whose chunks hold at most 80 rows -- two row slots of 32 and the first half
of the third.  The third slot then belongs to the waves 0..3 of a workgroup alone; the waves 4..7 run a second body of the kernel that
computes two row slots (`RW = 2` beside the layout's `R = 3`), chosen by ONE wave-uniform branch at the top of the kernel.  `pipe_wide`
0 keeps the grid of the per-iteration launches (persist_grid: the fewest workgroups that fit 96 rows) and `k_tcg_pipe_obl`.

    shape      n      p = 32: pipe_wide 0         pipe_wide 1
    (20, 30)   600    8 workgroups of 75 rows     the same 8: waves 0..2 hold rows in the third slot (11 of them), waves 4..7 two slots
    (33, 37)   1221   16 of 76 - 77 rows          the same 16: waves 0..3 three slots, wave 3's third partly filled (12 - 13 rows)
    (23, 32)   736    8 of 92 rows                16 of 46 rows: the third slot empty in every wave, the second half empty
    (100, 200) 20000  216 of 92 - 93 rows         256 of 78 - 79 rows (a device with 256 CUs)

Where both plans take the same workgroups the results are the same BITS: a slot that is not computed only ever added +0 to a sum.  Where
they differ the grid reduction sums the workgroups' partials in another order: the check is the oracle's tCG and its TR iterations, with
the bounds of tests/test_gpu_fused_row_bounds.py (counts and stop codes exact, cost to 1e-11 relative, gradient norm to 1e-8 relative).
Every run asserts the path (`tcg_path() == 1`, `persist_form() == 2`) and the plan (`fused_plan()`)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

SAME = [((33, 37), 32, 16), ((20, 30), 32, 8)]          # (shape, p, workgroups of both plans)
REFRESH = [2, 4, 16]
WIDE_SHAPE = (23, 32)                                   # 8 workgroups of 92 rows against 16 of 46


def _plan(n, cap):
    """The smallest multiple of 8, at least 8, with ceil(n / G) <= cap."""
    return max(8, -(-(-(-n // cap)) // 8) * 8)


def _grid(shape):
    from manisdp_matlab_amd import problems
    return problems.toroidal_grid_maxcut(shape[0], shape[1], seed=3)


@functools.lru_cache(maxsize=None)
def _problem(shape, p):
    """The matrix, the cold start, the oracle's point after six TR iterations and Delta_bar -- computed once, never written to."""
    from oracle import manisdp_ref as R, manopt_rtr
    C = _grid(shape)
    n = C.shape[0]
    rng = np.random.default_rng(11)
    Y = rng.standard_normal((n, p))
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    prob = R._OnlyUnitDiagProblem(C, n, p, q1="correct")
    Y1 = manopt_rtr.trustregions(prob, Y.copy(), 6, 40, 1e-8)[0]
    Y.setflags(write=False)
    Y1.setflags(write=False)
    return C, (Y, Y1), prob, prob.M.typicaldist()


@functools.lru_cache(maxsize=None)
def _oracle(shape, p):
    """The oracle's single tCGs (caps 1, 2, 7, 100 from the cold start, 7 and 20 from the second one) and its six TR iterations from
    both starts: the runs of tests/test_gpu_fused_row_bounds.py."""
    from oracle import manopt_rtr
    C, starts, prob, _ = _problem(shape, p)
    single = {}
    for s, caps in enumerate(((1, 2, 7, 100), (7, 20))):
        for m in caps:
            _, f_ref, info = manopt_rtr.trustregions(prob, starts[s].copy(), 1, m, 1e-8)
            single[(s, m)] = (f_ref, info.gradnorm, info.hessvecs, info.stop_inner[-1])
    six = []
    for s in range(2):
        _, f_ref, info = manopt_rtr.trustregions(prob, starts[s].copy(), 6, 40, 1e-9)
        six.append((info.iters, info.hessvecs, info.accepted, info.rejected, info.stop_inner[-1], f_ref, info.gradnorm))
    return single, tuple(six)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _handle(lib, C, p, refresh=16, wide=1, own=1, fused=1):
    h = lib.Handle.onlyunitdiag(C, pcap=p)
    h.set_option("persist_pipe", 1)
    h.set_option("pipe_refresh", refresh)
    h.set_option("fused_rtr", fused)
    h.set_option("pipe_own", own)
    h.set_option("pipe_wide", wide)
    return h


def _on_path(h, plan):
    assert h.tcg_path() == 1 and h.persist_form() == 2, "one-reduction persistent trip not selected"
    assert h.fused_plan() == plan, f"fused plan {h.fused_plan()}, expected {plan}"


def _stats(st):
    return (st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner, st.cost, st.gradnorm, st.Delta)


def _six(lib, h, start, plan, Delta0=None):
    h.set_point(start)
    _on_path(h, plan)
    kw = {} if Delta0 is None else {"Delta0": Delta0}
    st = h.rtr(lib.default_opts(maxiter=6, maxinner=40, tolgradnorm=1e-9, **kw))
    _on_path(h, plan)
    return _stats(st), h.get_point()


@pytest.mark.parametrize("refresh", REFRESH)
@pytest.mark.parametrize("shape,p,G", SAME)
def test_same_grid_wide_against_narrow_bit_for_bit(lib, shape, p, G, refresh):
    """Six TR iterations from Delta0 = Delta_bar (the launch rejects a step) with `pipe_wide` 1 and 0 from both starts, on the shapes
    where both plans take the same workgroups: the same point, cost, gradient norm, radius and counts, bit for bit."""
    C, starts, _, delta_bar = _problem(shape, p)
    rejected = 0
    for s in range(2):
        out = []
        for wide in (1, 0):
            h = _handle(lib, C, p, refresh, wide)
            out.append(_six(lib, h, starts[s], (G, 4 if wide else 0), delta_bar))
            h.close()
        on, off = out
        print(f"{shape} p={p} refresh={refresh} start={s}: wide {on[0]}, narrow {off[0]}")
        assert np.all(np.isfinite(on[1]))
        assert on[0] == off[0]
        assert np.array_equal(on[1], off[1])
        rejected += on[0][3]
    assert rejected >= 1, "no rejected step inside the fused launches"


@pytest.mark.parametrize("p", [32, 17])
def test_other_grid_single_tcg_matches_oracle(lib, p):
    """(23, 32): 16 workgroups of 46 rows where `pipe_wide` 0 takes 8 of 92.  ONE tCG (maxiter = 1) per inner cap against the oracle's;
    p = 17 leaves 7 of the 16 lanes of a row without columns."""
    C, starts, _, _ = _problem(WIDE_SHAPE, p)
    single, _ = _oracle(WIDE_SHAPE, p)
    h = _handle(lib, C, p, 4)
    for (s, maxinner), (f_ref, g_ref, hv_ref, stop_ref) in single.items():
        h.set_point(starts[s])
        _on_path(h, (16, 4))
        st = h.rtr(lib.default_opts(maxiter=1, maxinner=maxinner, tolgradnorm=1e-8))
        dc = abs(st.cost - f_ref) / max(1.0, abs(f_ref))
        dg = abs(st.gradnorm - g_ref) / max(1.0, g_ref)
        what = f"{WIDE_SHAPE} p={p} start={s} maxinner={maxinner}"
        print(f"{what}: hessvecs {st.hessvecs} / {hv_ref}, stop {st.last_stop_inner} / {stop_ref}, cost {dc:.2e}, gradnorm {dg:.2e}")
        assert st.hessvecs == hv_ref, what
        assert st.last_stop_inner == stop_ref, what
        assert dc < 1e-11, what
        assert dg < 1e-8, what
    h.close()


@pytest.mark.parametrize("p", [32, 17])
def test_other_grid_six_iterations_match_oracle(lib, p):
    """(23, 32): six TR iterations in one launch on 16 workgroups against the oracle's six."""
    C, starts, _, _ = _problem(WIDE_SHAPE, p)
    _, six = _oracle(WIDE_SHAPE, p)
    for s in range(2):
        h = _handle(lib, C, p, 4)
        stats, Yg = _six(lib, h, starts[s], (16, 4))
        h.close()
        ref = six[s]
        what = f"{WIDE_SHAPE} p={p} start={s}"
        print(f"{what}: oracle {ref[:5]}, fused {stats[:5]}, cost {abs(stats[5] - ref[5]):.2e}, gradnorm {abs(stats[6] - ref[6]):.2e}")
        assert np.all(np.isfinite(Yg))
        assert stats[:5] == ref[:5], what
        assert abs(stats[5] - ref[5]) < 1e-11 * max(1.0, abs(ref[5])), what
        assert abs(stats[6] - ref[6]) < 1e-8 * max(1.0, ref[6]), what


def test_switching_grids_on_one_handle(lib):
    """(23, 32) at p = 32 on ONE handle: the fused launch (16 workgroups), per-iteration launches (`fused_rtr` 0: 8 workgroups), the
    fused launch again.  Each equals what a fresh handle gives, bit for bit: the slot lines a launch on the other grid left posted are
    reset."""
    p = 32
    C, starts, _, delta_bar = _problem(WIDE_SHAPE, p)

    def run(h, fused):
        h.set_option("fused_rtr", fused)
        h.set_point(starts[1])
        assert h.tcg_path() == 1 and h.persist_form() == 2
        assert h.fused_plan() == ((16, 4) if fused else (0, 0))
        st = h.rtr(lib.default_opts(maxiter=6, maxinner=40, tolgradnorm=1e-9, Delta0=delta_bar))
        return _stats(st), h.get_point()

    fresh = {}
    for fused in (1, 0):
        h = _handle(lib, C, p, 4, fused=fused)
        fresh[fused] = run(h, fused)
        h.close()
    h = _handle(lib, C, p, 4)
    for fused in (1, 0, 1, 0, 1):
        got = run(h, fused)
        print(f"fused={fused}: {got[0]}")
        assert got[0] == fresh[fused][0]
        assert np.array_equal(got[1], fresh[fused][1])
    h.close()


@pytest.mark.parametrize("shape,plan", [((33, 37), (16, 4)), (WIDE_SHAPE, (16, 4))])
def test_wide_call_repeats_bit_for_bit(lib, shape, plan):
    """The same fused call twice on one handle: bit-identical points and statistics."""
    p = 32
    C, starts, _, delta_bar = _problem(shape, p)
    h = _handle(lib, C, p, 4)
    got = [_six(lib, h, starts[1], plan, delta_bar) for _ in range(2)]
    h.close()
    assert got[0][0] == got[1][0]
    assert np.all(np.isfinite(got[0][1]))
    assert np.array_equal(got[0][1], got[1][1])


def _matrix_z():
    """The (33, 37) grid's C plus one symmetric pair between two non-adjacent vertices without a diagonal: two rows of five off-diagonal
    entries and no diagonal, the widest row still 5 (the matrix Z of tests/test_gpu_fused_own_column.py)."""
    C = _grid((33, 37))
    A = C.tolil()
    nd = [i for i in range(C.shape[0]) if C[i, i] == 0.0]
    i = nd[0]
    k = next(k for k in nd[1:] if C[i, k] == 0.0 and k != i)
    A[i, k] = 0.25
    A[k, i] = 0.25
    Z = sp.csr_matrix(A.tocsr())
    Z.sort_indices()
    return Z


def test_other_instances_keep_their_grid_and_kernel(lib):
    """`pipe_own` 0, and a matrix with a row of five off-diagonal entries (no own-column slot): the five-gather instance on the grid of
    persist_grid, whatever `pipe_wide` says -- (23, 32) stays on 8 workgroups.  Both meet the oracle's six iterations."""
    p = 32
    C, starts, _, _ = _problem(WIDE_SHAPE, p)
    _, six = _oracle(WIDE_SHAPE, p)
    h = _handle(lib, C, p, 4, wide=1, own=0)
    stats, _ = _six(lib, h, starts[0], (8, 0))
    assert h.fused_own() == 0
    h.close()
    assert stats[:5] == six[0][:5]
    assert abs(stats[5] - six[0][5]) < 1e-11 * max(1.0, abs(six[0][5])) and abs(stats[6] - six[0][6]) < 1e-8 * max(1.0, six[0][6])
    Z = _matrix_z()
    rng = np.random.default_rng(11)
    Y = rng.standard_normal((Z.shape[0], p))
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    out = []
    for wide in (1, 0):
        h = _handle(lib, Z, p, 4, wide=wide)
        out.append(_six(lib, h, Y, (16, 0)))
        assert h.fused_own() == 0
        h.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


def test_planning_rule(lib):
    """The plans of handles with n = 600, 736, 1221 and 20000 rows at p = 32 with `pipe_wide` 1 and 0 on THIS device: the smallest
    multiple of 8, at most min(256, CUs / 8 * 8), with at most 80 (96) rows per workgroup; where the wide plan has no such grid, the
    narrow one.  (The rule itself against brute force: tests/test_fused_wide_rule_host.py.)"""
    cus = lib.fused_wide_rule(1)[1]
    gmax = 256 if cus >= 256 else (cus // 8) * 8
    assert gmax >= 16, "a device of 16 CUs or more"
    for shape in ((20, 30), (23, 32), (33, 37), (100, 200)):
        C = _grid(shape)
        n = C.shape[0]
        assert n == shape[0] * shape[1]
        Y = np.zeros((n, 32))
        Y[:, 0] = 1.0
        g0 = min(_plan(n, 96), gmax)
        if -(-n // g0) > 96:
            continue                                        # (a device too small for three row slots: not this file's subject)
        gw = _plan(n, 80)
        want = {0: (g0, 0), 1: (gw, 4) if gw <= gmax else (g0, 0)}
        for wide in (1, 0):
            h = _handle(lib, C, 32, wide=wide)
            h.set_point(Y)
            print(f"n={n} CUs={cus} pipe_wide={wide}: plan {h.fused_plan()}")
            _on_path(h, want[wide])
            h.close()
