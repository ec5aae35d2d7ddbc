"""CPU tests of what tests/test_gpu_color_sweep.py compares the colour-ordered local search against (tests/color_sweep_ref.py):
with the rows in index order the ordered restatements ARE round_ref.one_opt and phase_round_ref.round_phases; the greedy
colouring is a colouring on every instance the GPU tests use; colour order really ends elsewhere than index order on those
instances (otherwise the GPU tests could pass on the serial kernels); the decision margins of the M = 8 cases in colour order;
and the argument checks of the Python entry points, raised before the library is loaded."""
import numpy as np
import pytest
import scipy.sparse as sp

import color_sweep_ref as CS
import hermitian_ref as HR
import lowrank_ref
import phase_round_ref as PR
import round_ref
from conftest import golden_path

_CACHE = {}


def _real(name):
    if name not in _CACHE:
        _CACHE[name] = CS.real_instance(name, golden_path)
    return _CACHE[name]


def _real_rounds(name, p, T, sweeps, order):
    key = (name, p, T, sweeps, order)
    if key not in _CACHE:
        C = _real(name)
        _CACHE[key] = CS.round_hyperplane(C, round_ref.table_point(C.shape[0], p), round_ref.table_directions(T, p), sweeps, order)
    return _CACHE[key]


# ------------------------------------------------------------------ 1. index order is the serial restatement
@pytest.mark.parametrize("name", ["pair", "torus_hole", "G11", "hub203"])
def test_index_order_reproduces_one_opt(name):
    C = _real(name)
    n = C.shape[0]
    X0, _ = round_ref.signs(round_ref.table_point(n, 7), round_ref.table_directions(192, 7))
    for sweeps in (1, 50):
        Xa, ia = round_ref.one_opt(C, X0, sweeps)
        Xb, ib = CS.one_opt(C, X0, sweeps, np.arange(n))
        assert np.array_equal(Xa, Xb) and np.array_equal(ia, ib)
    a, b = round_ref.round_hyperplane(C, round_ref.table_point(n, 7), round_ref.table_directions(192, 7), 50), _real_rounds(name, 7, 192, 50, "index")
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case,M,sweeps,generic", [(PR.EXACT_CASES[1], 4, 50, False), (PR.TOL_CASES[0], 8, 50, True),
                                                   (PR.TOL_CASES[0], 0, 3, False), (PR.EXACT_CASES[0], 2, 0, False)])
def test_index_order_reproduces_round_phases(case, M, sweeps, generic):
    storage, n, T, p = case[:4]
    C = HR.instance(storage, n)
    if generic:
        C = PR.generic_instance(C)
    Y, R = PR.inputs(n, p, T, case[-1])
    for dtype in ((np.float64, np.longdouble) if M == 0 else (np.float64,)):
        a, b = PR.round_phases(C, Y, R, M, sweeps, dtype=dtype), CS.round_phases(C, Y, R, M, sweeps, np.arange(n), dtype=dtype)
        assert set(a) == set(b)
        for k in a:
            assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------ 2. the colouring
def _coloring_instances():
    out = [("real", name) for name in round_ref.SPARSE]
    for n in (203, 1031):
        out += [("grid_cs", n), ("hub_cs", n), ("herm_grid", n), ("herm_hub", n)]
    return out


def _coloring_instance(kind, arg):
    if kind == "real":
        return _real(arg)
    if kind in ("grid_cs", "hub_cs"):
        return sp.csr_matrix(getattr(lowrank_ref, kind)(arg))
    return HR.instance(kind[5:], arg)


@pytest.mark.parametrize("kind,arg", _coloring_instances())
def test_the_coloring_is_a_coloring(kind, arg):
    C = _coloring_instance(kind, arg)
    nc, color = CS.coloring(C)
    print(kind, arg, "n", C.shape[0], "colours", nc, "class sizes", np.bincount(color).tolist())
    assert color.dtype == np.int32 and color.shape == (C.shape[0],) and color.min() == 0
    assert nc == int(color.max()) + 1 and len(np.unique(color)) == nc        # every colour below ncolors is used
    assert CS.is_valid(C, color)
    order = CS.visiting_order(color)
    assert sorted(order.tolist()) == list(range(C.shape[0]))
    key = color[order].astype(np.int64) * C.shape[0] + order
    assert np.all(np.diff(key) > 0)                                            # sorted by (colour, index)
    # first-fit: every smaller colour is held by an earlier neighbour
    rp, ci = CS.pattern(C)
    for i in range(C.shape[0]):
        nb = ci[rp[i]:rp[i + 1]]
        assert set(range(color[i])) <= set(color[nb[nb < i]].tolist()), i
    rows = np.diff(rp)
    if (rows == 0).any():
        assert np.all(color[rows == 0] == 0)                                   # an empty row gets colour 0


def test_the_colour_counts_of_the_table():
    """What the sweep costs in launches: the counts DESIGN.md quotes."""
    assert CS.coloring(_real("pair"))[0] == 2 and CS.coloring(_real("G11"))[0] == 2
    assert CS.coloring(_real("torus"))[0] == 4 and CS.coloring(_real("G1"))[0] == 19
    for n in (203, 1031):
        assert CS.coloring(lowrank_ref.grid_cs(n))[0] == 4 and CS.coloring(lowrank_ref.hub_cs(n))[0] == 5


def test_an_unsymmetric_pattern_is_refused():
    C = sp.csr_matrix(np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
    with pytest.raises(ValueError, match="not symmetric"):
        CS.coloring(C)


# ------------------------------------------------------------------ 3. preconditions of the GPU tests
@pytest.mark.parametrize("name", [x for x in CS.REAL_EXACT if x != "pair"])
def test_colour_order_ends_elsewhere_on_the_real_instances(name):
    for p in round_ref.P_SUBSET:
        for T in CS.REAL_T:
            for sweeps in CS.REAL_SWEEPS:
                a, b = _real_rounds(name, p, T, sweeps, "index"), _real_rounds(name, p, T, sweeps, "color")
                differ = int(np.sum(np.any(round_ref.unpack(a["masks"]) != round_ref.unpack(b["masks"]), axis=1)))
                print(name, p, T, sweeps, "trials that differ:", differ, "of", T, "best", a["values"].min(), b["values"].min())
                assert differ >= 1
                assert np.array_equal(a["values0"], b["values0"]) and np.all(b["values"] <= b["values0"])
                if sweeps == 50:
                    assert np.all(b["info"][1] == 0) and np.all(b["info"][0] < 50)     # every word reached a fixed point


@pytest.mark.parametrize("case", PR.EXACT_CASES)
def test_colour_order_ends_elsewhere_on_the_exact_hermitian_cases(case):
    storage, n, T, p, M, seed = case
    C = HR.instance(storage, n)
    Y, R = PR.inputs(n, p, T, seed)
    for sweeps in PR.EXACT_SWEEPS[1:]:
        a, b = PR.round_phases(C, Y, R, M, sweeps), CS.round_phases(C, Y, R, M, sweeps, "color")
        differ = int(np.sum(np.any(a["phases"] != b["phases"], axis=1)))
        print(case, sweeps, "trials that differ:", differ, "of", T, "info", b["info"].tolist())
        assert differ >= 1
        assert np.array_equal(a["values0"], b["values0"]) and np.all(b["values"] <= b["values0"])
        if sweeps == 50:
            assert np.all(b["info"][1] == 0) and np.all(b["info"][0] < 50) and np.all(b["info"][0] > 1)


@pytest.mark.parametrize("case", CS.COLOR_TOL_CASES)
def test_margins_of_the_tolerance_cases_in_colour_order(case):
    """M = 8 on the generic values, rows in colour order: the rounding and the sweep margins exceed MARGIN_REL of their scales,
    so a device that sums with fma must take the same decisions; and the fp64 / long double distance of the M = 0 sweeps."""
    storage, n, T, p, seed = case
    C = HR.instance(storage, n)
    Y, R = PR.inputs(n, p, T, seed)
    g8 = CS.round_phases(PR.generic_instance(C), Y, R, 8, PR.M8_SWEEPS, "color")
    print(case, "M = 8 generic, colour order: rounding margin %.2e, sweep margin %.2e of the scale, sweeps %s" % (
        g8["margin_round"] / g8["scale_round"], g8["margin_sweep"] / g8["scale_sweep"], g8["info"][0].tolist()))
    assert g8["margin_round"] > PR.MARGIN_REL * g8["scale_round"] and g8["margin_sweep"] > PR.MARGIN_REL * g8["scale_sweep"]
    assert np.all(g8["info"][1] == 0)
    for s in PR.CIRCLE_SWEEPS:
        a, b = CS.round_phases(C, Y, R, 0, s, "color"), CS.round_phases(C, Y, R, 0, s, "color", dtype=np.longdouble)
        dist = np.max(np.abs(a["phases"] - b["phases"]))
        print(case, "M = 0, %d sweeps, colour order: fp64 to long double %.3e" % (s, dist))
        assert 0 < dist < 1e-10


# ------------------------------------------------------------------ 4. the Python entry points refuse before the library loads
def test_order_arguments_are_checked_before_the_library_loads(monkeypatch):
    from manisdp_matlab_amd import _lib, problems, solvers

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", no_load)
    Cr = _real("torus")
    Cc, _ = problems.phase_synchronization(60, 6, 1.0, np.random.default_rng(7))
    for bad in ("colour", "greedy", 1, None):
        with pytest.raises(ValueError, match="order"):
            solvers.round_unitdiag(Cr, round_ref.table_point(65, 2), trials=64, order=bad)
        with pytest.raises(ValueError, match="order"):
            solvers.round_phases(Cc, PR.inputs(60, 2, 64, 1)[0], trials=64, order=bad)
        with pytest.raises(ValueError, match=r"options\['round'\]\['order'\]"):
            solvers.ManiSDP_onlyunitdiag(Cr, {"round": {"trials": 64, "order": bad}}, verbose=False)
        with pytest.raises(ValueError, match=r"options\['round_phases'\]\['order'\]"):
            solvers.ManiSDP_onlyunitdiag(Cc, {"round_phases": {"trials": 64, "order": bad}}, verbose=False)
    with pytest.raises(ValueError, match="'order'"):                             # the known-fields message names the new field
        solvers.ManiSDP_onlyunitdiag(Cr, {"round": {"trails": 64}}, verbose=False)
    with pytest.raises(ValueError, match="'order'"):
        solvers.ManiSDP_onlyunitdiag(Cc, {"round_phases": {"trails": 64}}, verbose=False)
    assert solvers._round_option({"round": {"trials": 64}}) == (64, 50, 0, "index")
    assert solvers._round_option({"round": {"trials": 64, "order": "color"}}) == (64, 50, 0, "color")
    assert solvers._round_phases_option({"round_phases": {"M": 4}}) == (4, 256, 20, 0, "index")
    assert solvers._round_phases_option({"round_phases": {"M": 4, "order": "color"}}) == (4, 256, 20, 0, "color")
