"""The own-column instance of the fused one-reduction tCG trip at 16 lanes per row (msdp_pipe.h, `k_tcg_pipe_obl<16, 5, 3, ..., FUSE,
OWNC>`, option `pipe_own`, default 1): set-up sorts a row's entry in its OWN column -- the diagonal, or the first padding slot
(own row, 0.0) of a row without one -- to ELL column 0, and the kernel takes that row from what the lane already holds (H md of the trip
before, the gradient row at the first trip of a tCG, the proposal row in the TR tail) instead of gathering it: 12 requests a trip,
not 15.  What can go wrong:

  - the lane's copy is not the value the neighbours see (a trip too old, the wrong buffer after an accepted / rejected step, the
    refresh trip's direct gathers folded without their column 0);
  - a row without a diagonal and with 1, 2 or 3 padding slots sorts another slot to column 0, or folds in another order;
  - a handle with a row of five off-diagonal entries and no diagonal (no own column at all) takes the instance anyway;
  - the twelve spread requests leave one out, or one is not skipped in front of a refresh trip.

Shapes, oracle, bounds: those of tests/test_gpu_fused_early_gather.py -- `toroidal_grid_maxcut((7, 11), seed=3)` at p = 32, `(33, 37)`
at p = 17 and 20; `oracle.manopt_rtr` from the cold start and from its point after six TR iterations; counts and stop codes exact, cost
to 1e-11 relative, gradient norm to 1e-8 relative.  `pipe_own = 0` launches the five-gather instance: the comparison is bit for bit.
Matrix T: the (7, 11) grid's C with three symmetric off-diagonal pairs and three diagonal entries removed (rows of 2, 3 and 4 entries).
Matrix Z: the (33, 37) grid's C with one pair added between two non-adjacent vertices without a diagonal (a row of five off-diagonal
entries): the handle must refuse the instance.  Every run asserts the path taken."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

GRIDS = [((7, 11), 32), ((33, 37), 17), ((33, 37), 20)]
CASES = [("grid",) + g for g in GRIDS] + [("T", (7, 11), 32)]
REFRESH = [2, 3, 64]             # refresh trips on every second trip, mixed, never
CAPS = (1, 2, 3, 7, 20)


def _grid(shape):
    from manisdp_matlab_amd import problems
    return problems.toroidal_grid_maxcut(shape[0], shape[1], seed=3)


def _no_diag(A):
    return [i for i in range(A.shape[0]) if A[i, i] == 0.0]


def _matrix_t():
    """The (7, 11) grid's C with rows of 2, 3 and 4 entries: row i0 (no diagonal) loses two of its edges, an edge between two other
    vertices without a diagonal goes, and three rows lose their diagonal entry."""
    A = _grid((7, 11)).toarray()
    nd = _no_diag(A)
    i0 = nd[0]
    nb = [j for j in np.flatnonzero(A[i0]) if j != i0]
    for j in nb[:2]:
        A[i0, j] = A[j, i0] = 0.0
    touched = {i0, *nb[:2]}
    pair = next((a, b) for a in nd for b in np.flatnonzero(A[a]) if b > a and b in nd and a not in touched and b not in touched)
    A[pair[0], pair[1]] = A[pair[1], pair[0]] = 0.0
    touched |= set(pair)
    with_diag = [i for i in range(A.shape[0]) if A[i, i] != 0.0 and i not in touched]
    for i in with_diag[:3]:
        A[i, i] = 0.0
    T = sp.csr_matrix(A)
    T.sort_indices()
    return T


def _matrix_z():
    """The (33, 37) grid's C plus one symmetric pair between two non-adjacent vertices without a diagonal: rows i and k then hold five
    off-diagonal entries and no diagonal, and the widest row is still 5."""
    C = _grid((33, 37))
    A = C.tolil()
    nd = [i for i in range(C.shape[0]) if C[i, i] == 0.0]
    i = nd[0]
    k = next(k for k in nd[1:] if C[i, k] == 0.0 and k != i)
    A[i, k] = 0.25
    A[k, i] = 0.25
    Z = A.tocsr()
    Z.sort_indices()
    return Z, i, k


def _matrix(kind, shape):
    return _grid(shape) if kind == "grid" else (_matrix_t() if kind == "T" else _matrix_z()[0])


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, p):
    """The problem, the two start points (cold; the oracle's point after six TR iterations), the oracle's single tCGs from them for
    every inner cap, and its six TR iterations from a start radius of Delta_bar -- computed once per case, never written to."""
    from oracle import manisdp_ref as R, manopt_rtr
    C = _matrix(kind, shape)
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
    delta_bar = prob.M.typicaldist()
    six = []
    for s in range(2):
        _, f_ref, info = manopt_rtr.trustregions(prob, starts[s].copy(), 6, 40, 1e-9, Delta0=delta_bar)
        six.append((info.iters, info.hessvecs, info.accepted, info.rejected, info.stop_inner[-1], f_ref, info.gradnorm))
    for a in starts:
        a.setflags(write=False)
    return C, starts, single, delta_bar, tuple(six)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _handle(lib, C, p, refresh, own):
    h = lib.Handle.onlyunitdiag(C, pcap=p)
    h.set_option("persist_pipe", 1)
    h.set_option("pipe_refresh", refresh)
    h.set_option("fused_rtr", 1)
    h.set_option("pipe_own", own)
    return h


def _on_path(h, own):
    assert h.tcg_path() == 1 and h.persist_form() == 2, "one-reduction persistent trip not selected"
    assert h.fused_own() == own, "own-column instance: %d expected" % own


def _six(lib, C, p, refresh, own, start, delta_bar, expect_own=None):
    h = _handle(lib, C, p, refresh, own)
    h.set_point(start)
    _on_path(h, own if expect_own is None else expect_own)
    st = h.rtr(lib.default_opts(maxiter=6, maxinner=40, tolgradnorm=1e-9, Delta0=delta_bar))
    _on_path(h, own if expect_own is None else expect_own)
    out = ((st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner, st.cost, st.gradnorm, st.Delta), h.get_point())
    h.close()
    return out


def _check_six(got, ref, what):
    stats = got[0]
    print(f"{what}: oracle {ref[:5]}, fused {stats[:5]}, cost {abs(stats[5] - ref[5]):.2e}, gradnorm {abs(stats[6] - ref[6]):.2e}")
    assert stats[:5] == ref[:5], what
    assert abs(stats[5] - ref[5]) < 1e-11 * max(1.0, abs(ref[5])), what
    assert abs(stats[6] - ref[6]) < 1e-8 * max(1.0, ref[6]), what


def _check_singles(lib, h, starts, single, own, what0):
    for (s, maxinner), (f_ref, g_ref, hv_ref, stop_ref) in single.items():
        h.set_point(starts[s])
        st = h.rtr(lib.default_opts(maxiter=1, maxinner=maxinner, tolgradnorm=1e-8))
        _on_path(h, own)
        dc = abs(st.cost - f_ref) / max(1.0, abs(f_ref))
        dg = abs(st.gradnorm - g_ref) / max(1.0, g_ref)
        what = f"{what0} start={s} maxinner={maxinner}"
        print(f"{what}: hessvecs {st.hessvecs} / {hv_ref}, stop {st.last_stop_inner} / {stop_ref}, cost {dc:.2e}, gradnorm {dg:.2e}")
        assert st.hessvecs == hv_ref, what
        assert st.last_stop_inner == stop_ref, what
        assert dc < 1e-11, what
        assert dg < 1e-8, what


def test_matrices_hold_the_rows_the_instance_distinguishes():
    """Precondition, on the CPU.  The three grids hold rows with and rows without a diagonal entry, none wider than 5 and none with
    five off-diagonal entries; T holds rows with a diagonal and rows with one, two and three padding slots; Z holds a row with five
    off-diagonal entries and no diagonal while its widest row is 5."""
    for shape in ((7, 11), (33, 37)):
        C = _grid(shape)
        n = C.shape[0]
        cnt = np.diff(C.indptr)
        dg = C.diagonal() != 0.0
        assert dg.any() and (~dg).any(), shape
        assert cnt.max() == 5 and np.all(cnt[~dg] <= 4), shape
        assert n == shape[0] * shape[1]
    T = _matrix_t()
    assert abs(T - T.T).max() == 0.0
    cnt = np.diff(T.indptr)
    dg = T.diagonal() != 0.0
    assert dg.any() and cnt.max() == 5
    assert {1, 2, 3} <= set((5 - cnt[~dg]).tolist()), sorted(set((5 - cnt[~dg]).tolist()))
    Z, i, k = _matrix_z()
    assert abs(Z - Z.T).max() == 0.0
    cnt = np.diff(Z.indptr)
    assert cnt.max() == 5
    for r in (i, k):
        assert Z[r, r] == 0.0 and cnt[r] == 5, r
    C = _grid((33, 37))
    assert C[i, k] == 0.0 and i != k


@pytest.mark.gpu
@pytest.mark.parametrize("refresh", REFRESH)
@pytest.mark.parametrize("shape,p", GRIDS)
def test_own_column_on_against_off_bit_for_bit(lib, shape, p, refresh):
    """Six TR iterations from Delta0 = Delta_bar in ONE fused launch with `pipe_own` 1 and 0, from both starts: the same point bit for
    bit and the same statistics.  The oracle rejects a step on these runs, and so does the launch: together they cover the tail, a
    tCG restarting at the same point, the first trip after an accepted step, and (refresh 2, 3) refresh trips."""
    C, starts, _, delta_bar, six = _reference("grid", shape, p)
    for s in range(2):
        assert six[s][3] >= 1, f"precondition: the oracle rejects no step on {shape} p={p} start={s}"
        on = _six(lib, C, p, refresh, 1, starts[s], delta_bar)
        off = _six(lib, C, p, refresh, 0, starts[s], delta_bar)
        print(f"{shape} p={p} refresh={refresh} start={s}: on {on[0]}, off {off[0]}")
        assert on[0][3] >= 1, "no rejected step inside the fused launch"
        assert np.all(np.isfinite(on[1]))
        assert on[0] == off[0]
        assert np.array_equal(on[1], off[1])


@pytest.mark.gpu
@pytest.mark.parametrize("refresh", REFRESH)
@pytest.mark.parametrize("kind,shape,p", CASES)
def test_own_column_single_tcg_matches_oracle(lib, kind, shape, p, refresh):
    """ONE tCG (maxiter = 1) for the inner caps 1, 2, 3, 7 and 20 from both starts with `pipe_own` = 1, on the grids and on T."""
    C, starts, single, _, _ = _reference(kind, shape, p)
    h = _handle(lib, C, p, refresh, 1)
    h.set_point(starts[0])
    _on_path(h, 1)
    _check_singles(lib, h, starts, single, 1, f"{kind} {shape} p={p} refresh={refresh}")
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("refresh", REFRESH)
@pytest.mark.parametrize("kind,shape,p", CASES)
def test_own_column_six_iterations_match_oracle(lib, kind, shape, p, refresh):
    """The six-iteration runs with `pipe_own` = 1 against the oracle, on the grids and on T."""
    C, starts, _, delta_bar, six = _reference(kind, shape, p)
    for s in range(2):
        got = _six(lib, C, p, refresh, 1, starts[s], delta_bar)
        _check_six(got, six[s], f"{kind} {shape} p={p} refresh={refresh} start={s}")


@pytest.mark.gpu
def test_row_of_five_off_diagonal_entries_refuses_the_instance(lib):
    """Z: one row pair without any own-column slot.  The query answers 0 with `pipe_own` = 1, the run stays on the one-reduction
    persistent path (the five-gather instance) and meets the oracle bounds."""
    p = 17
    C, starts, single, delta_bar, six = _reference("Z", (33, 37), p)
    h = _handle(lib, C, p, 3, 1)
    h.set_point(starts[0])
    _on_path(h, 0)
    _check_singles(lib, h, starts, single, 0, f"Z p={p}")
    h.close()
    for s in range(2):
        got = _six(lib, C, p, 3, 1, starts[s], delta_bar, expect_own=0)
        _check_six(got, six[s], f"Z p={p} start={s}")


@pytest.mark.gpu
@pytest.mark.parametrize("refresh", REFRESH)
@pytest.mark.parametrize("p", [17, 20])
def test_own_column_call_repeats_bit_for_bit(lib, p, refresh):
    """The same fused call twice on the 16-workgroup shape: bit-identical points."""
    C, starts, _, delta_bar, _ = _reference("grid", (33, 37), p)
    h = _handle(lib, C, p, refresh, 1)
    got = []
    for _ in range(2):
        h.set_point(starts[1])
        _on_path(h, 1)
        st = h.rtr(lib.default_opts(maxiter=6, maxinner=40, tolgradnorm=1e-9, Delta0=delta_bar))
        _on_path(h, 1)
        got.append(((st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner, st.cost, st.gradnorm, st.Delta), h.get_point()))
    h.close()
    assert got[0][0] == got[1][0]
    assert np.all(np.isfinite(got[0][1]))
    assert np.array_equal(got[0][1], got[1][1])
