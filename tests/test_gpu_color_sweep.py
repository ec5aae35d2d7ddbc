"""The colour-ordered local search of msdp_round_hyperplane and msdp_round_phases (set_option("round_order", 1)) and
msdp_round_coloring on the device, against the ordered restatement of tests/color_sweep_ref.py.

Equality is asked for wherever tests/test_gpu_round.py and tests/test_gpu_phase_round.py ask it of the serial path: weights in
Z/4 (and the exact tables M = 2, 4), where every sum is exact in fp64 in any order.  M = 8 and M = 0 follow the acceptance rules
of tests/test_gpu_phase_round.py, on the cases of color_sweep_ref.COLOR_TOL_CASES, whose margins in colour order
tests/test_color_sweep_ref_host.py checks; that file also checks that colour order ends elsewhere than index order on every
instance here but `pair`, so none of the comparisons below can pass on the serial kernels."""
import numpy as np
import pytest
import scipy.sparse as sp

import color_sweep_ref as CS
import hermitian_ref as HR
import lowrank_ref
import phase_round_ref as PR
import round_ref
from conftest import golden_path

pytestmark = pytest.mark.gpu
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _real(name):
    if name not in _CACHE:
        _CACHE[name] = CS.real_instance(name, golden_path)
    return _CACHE[name]


def _real_ref(name, p, T, sweeps):
    """The ordered restatement, computed once per case and never modified."""
    key = (name, p, T, sweeps)
    if key not in _CACHE:
        C = _real(name)
        _CACHE[key] = CS.round_hyperplane(C, round_ref.table_point(C.shape[0], p), round_ref.table_directions(T, p), sweeps, "color")
    return _CACHE[key]


def _phase_ref(key, C, Y, R, M, sweeps, dtype=np.float64):
    k = (key, M, sweeps, np.dtype(dtype).name)
    if k not in _CACHE:
        _CACHE[k] = CS.round_phases(C, Y, R, M, sweeps, "color", dtype=dtype)
    return _CACHE[k]


def _l1(C):
    return float(np.abs(sp.csr_matrix(C)).sum())


# ------------------------------------------------------------------ 1. the colouring
def test_coloring_equals_the_restatement_and_is_cached(lib):
    cases = [(_real(name), False) for name in round_ref.SPARSE]
    for n in (203, 1031):
        cases += [(sp.csr_matrix(lowrank_ref.grid_cs(n)), False), (sp.csr_matrix(lowrank_ref.hub_cs(n)), False),
                  (HR.instance("grid", n), True), (HR.instance("hub", n), True)]
    for C, herm in cases:
        nc, color = CS.coloring(C)
        h = lib.Handle.onlyunitdiag_hermitian(C) if herm else lib.Handle.onlyunitdiag(C)
        try:
            for _ in range(2):                                                     # no resident point; the second call is the cached one
                got_nc, got = h.round_coloring()
                assert got_nc == nc and got.dtype == np.int32 and np.array_equal(got, color)
        finally:
            h.close()


def test_an_unsymmetric_pattern_is_refused_by_name(lib):
    C = sp.csr_matrix(np.array([[0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0]]))
    h = lib.Handle.onlyunitdiag(C)
    try:
        h.set_point(round_ref.table_point(4, 2))
        h.set_option("round_order", 1)
        # the handle stores row i as column i of what it was given: the stored entry without a mirror is (1, 3)
        for call in (h.round_coloring, lambda: h.round_hyperplane(np.ones((64, 2)), sweeps=1)):
            with pytest.raises(lib.MsdpError, match=r"entry \(1, 3\) is stored, entry \(3, 1\) is not") as e:
                call()
            assert e.value.code == lib.EINVAL
        h.set_option("round_order", 0)
        assert h.round_hyperplane(np.ones((64, 2)), sweeps=1)["values"].shape == (64,)   # index order still serves
    finally:
        h.close()


# ------------------------------------------------------------------ 2. the real kind, exact
@pytest.mark.parametrize("name", CS.REAL_EXACT)
def test_real_kind_equals_the_ordered_restatement(lib, name):
    C = _real(name)
    n = C.shape[0]
    for p in round_ref.P_SUBSET:
        h = lib.Handle.onlyunitdiag(C, pcap=max(32, p))
        try:
            h.set_point(round_ref.table_point(n, p))
            h.set_option("round_order", 1)
            for T in CS.REAL_T:
                R = round_ref.table_directions(T, p)
                for sweeps in CS.REAL_SWEEPS:
                    ref = _real_ref(name, p, T, sweeps)
                    got = h.round_hyperplane(R, sweeps=sweeps, masks=True)
                    print(name, p, T, sweeps, "info", got["info"].tolist(), ref["info"].tolist(), "words that differ",
                          int(np.sum(got["masks"] != ref["masks"])))
                    assert np.array_equal(got["masks"], ref["masks"])
                    assert np.array_equal(got["info"], ref["info"])
                    assert np.array_equal(got["values0"], ref["values0"]) and np.array_equal(got["values"], ref["values"])
                    assert got["best"] == ref["best"] and np.array_equal(got["x"], ref["x"])
            again = h.round_hyperplane(R, sweeps=sweeps, masks=True)                 # two identical calls, identical bytes
            for k in ("values0", "values", "info", "x", "masks"):
                assert again[k].tobytes() == got[k].tobytes(), k
        finally:
            h.close()


# ------------------------------------------------------------------ 3. the Hermitian kind, exact
@pytest.mark.parametrize("case", PR.EXACT_CASES)
def test_hermitian_kind_equals_the_ordered_restatement(lib, case):
    storage, n, T, p, M, seed = case
    C = HR.instance(storage, n)
    Y, R = PR.inputs(n, p, T, seed)
    h = lib.Handle.onlyunitdiag_hermitian(C, pcap=max(32, p))
    try:
        h.set_point(Y)
        h.set_option("round_order", 1)
        for sweeps in PR.EXACT_SWEEPS:
            ref = _phase_ref(case, C, Y, R, M, sweeps)
            res = h.round_phases(R, M=M, sweeps=sweeps, phases=True)
            print(case, "sweeps", sweeps, "info", res["info"].tolist(), ref["info"].tolist(), "phases differ at",
                  int(np.sum(res["phases"] != ref["phases"])))
            assert np.array_equal(res["phases"], ref["phases"])
            assert np.array_equal(res["values0"], ref["values0"]) and np.array_equal(res["values"], ref["values"])
            assert np.array_equal(res["info"], ref["info"]) and res["best"] == ref["best"]
            assert np.array_equal(res["z"], ref["z"]) and np.array_equal(res["k"], ref["kbest"])
            assert np.array_equal(PR.host_values(C, res["phases"]), res["values"])
            if sweeps == 50:
                assert np.all(res["info"][1] == 0) and np.all(res["info"][0] < 50)
    finally:
        h.close()


# ------------------------------------------------------------------ 4. the Hermitian kind, M = 8 and M = 0
@pytest.mark.parametrize("case", CS.COLOR_TOL_CASES)
def test_eight_psk_and_circle_against_the_ordered_restatement(lib, case):
    storage, n, T, p, seed = case
    C = HR.instance(storage, n)
    G = PR.generic_instance(C)
    Y, R = PR.inputs(n, p, T, seed)
    tol, tolg = 1e-12 * _l1(C), 1e-12 * _l1(G)
    h, hg = lib.Handle.onlyunitdiag_hermitian(C, pcap=max(32, p)), lib.Handle.onlyunitdiag_hermitian(G, pcap=max(32, p))
    try:
        for x in (h, hg):
            x.set_point(Y)
            x.set_option("round_order", 1)
        # M = 8, the sweeps, on the generic values: equal decisions, values to 1e-12 ||G||_1
        ref = _phase_ref((case, "generic"), G, Y, R, 8, PR.M8_SWEEPS)
        res = hg.round_phases(R, M=8, sweeps=PR.M8_SWEEPS, phases=True)
        print(case, "M 8 sweeps: info", res["info"].tolist(), ref["info"].tolist(), "phases differ at",
              int(np.sum(res["phases"] != ref["phases"])), "values %.2e (tol %.2e)" % (np.max(np.abs(res["values"] - ref["values"])), tolg))
        assert np.array_equal(res["phases"], ref["phases"]) and np.array_equal(res["info"], ref["info"])
        assert np.array_equal(res["k"], ref["k"][res["best"] // 64, :, res["best"] % 64])
        assert np.max(np.abs(res["values"] - ref["values"])) <= tolg and np.max(np.abs(res["values0"] - ref["values0"])) <= tolg
        assert np.max(np.abs(PR.host_values(G, res["phases"]) - res["values"])) <= tolg
        assert np.all(res["values"] <= res["values0"] + tolg) and res["best"] == int(np.argmin(res["values"]))
        # M = 0, the sweeps: within ten times the fp64 / long double distance of the restatement
        for s in PR.CIRCLE_SWEEPS:
            ref, refl = _phase_ref(case, C, Y, R, 0, s), _phase_ref(case, C, Y, R, 0, s, dtype=np.longdouble)
            yard = np.max(np.abs(ref["phases"] - refl["phases"]))
            res = h.round_phases(R, M=0, sweeps=s, phases=True)
            dist = np.max(np.abs(res["phases"] - ref["phases"]))
            print(case, "M 0, %d sweeps: device to fp64 restatement %.3e, fp64 to long double %.3e" % (s, dist, yard))
            assert dist <= 10.0 * yard
            assert np.all(res["info"][0] == s) and not res["info"][1].any()
            assert np.max(np.abs(PR.host_values(C, res["phases"]) - res["values"])) <= tol
            assert np.all(res["values"] < res["values0"])
    finally:
        h.close(); hg.close()


# ------------------------------------------------------------------ 5. switching
def test_switching_back_and_untouched_state(lib):
    C = _real("G11")
    Y, R = round_ref.table_point(800, 7), round_ref.table_directions(192, 7)
    U = np.random.default_rng(9).standard_normal((800, 7))
    h, fresh = lib.Handle.onlyunitdiag(C), lib.Handle.onlyunitdiag(C)
    try:
        h.set_point(Y); fresh.set_point(Y)
        f0, H0 = h.cost(), h.hessvec(U)
        h.set_option("round_order", 1)
        col = h.round_hyperplane(R, sweeps=50, masks=True)
        assert np.array_equal(h.get_point(), Y) and h.cost() == f0 and np.array_equal(h.hessvec(U), H0)
        h.set_option("round_order", 0)
        a, b = h.round_hyperplane(R, sweeps=50, masks=True), fresh.round_hyperplane(R, sweeps=50, masks=True)
        for k in ("values0", "values", "info", "x", "masks"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["best"] == b["best"] and not np.array_equal(a["masks"], col["masks"])
    finally:
        h.close(); fresh.close()
    Ch = HR.instance("hub", 203)
    Yc, Rc = PR.inputs(203, 3, 128, 51)
    Uc = HR.table_direction(203, 3)
    h, fresh = lib.Handle.onlyunitdiag_hermitian(Ch), lib.Handle.onlyunitdiag_hermitian(Ch)
    try:
        h.set_point(Yc); fresh.set_point(Yc)
        f0, H0 = h.cost(), h.hessvec(Uc)
        h.set_option("round_order", 1)
        for M, sweeps in ((0, 2), (4, 50)):
            col = h.round_phases(Rc, M=M, sweeps=sweeps, phases=True)
        assert np.array_equal(h.get_point(), Yc) and h.cost() == f0 and np.array_equal(h.hessvec(Uc), H0)
        h.set_option("round_order", 0)
        a, b = h.round_phases(Rc, M=4, sweeps=50, phases=True), fresh.round_phases(Rc, M=4, sweeps=50, phases=True)
        for k in ("values0", "values", "info", "z", "k", "phases"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["best"] == b["best"] and not np.array_equal(a["phases"], col["phases"])
    finally:
        h.close(); fresh.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals(lib):
    from manisdp_matlab_amd import problems
    A = _real("torus")
    V, s = lowrank_ref.lowrank_term(65, 3)
    blockC, _, _ = problems.rotation_synchronization(20, 3, 4, 0.1, 1)
    At, b, c, K = problems.theta_problem(8, seed=1)
    others = (("dense", lambda: lib.Handle.onlyunitdiag(A.toarray())), ("low-rank", lambda: lib.Handle.onlyunitdiag_lowrank(A, V, s)),
              ("unit-block-diagonal", lambda: lib.Handle.onlyunitblockdiag(blockC, 3)),
              ("unittrace", lambda: lib.Handle.affine(lib.KIND_UNITTRACE, At, b, c, K["s"])))
    for word, make in others:
        h = make()
        try:
            for call in (lambda: h.set_option("round_order", 1), h.round_coloring):
                with pytest.raises(lib.MsdpError, match=word) as e:
                    call()
                assert e.value.code == lib.EUNSUPPORTED, word
            h.set_option("round_order", 0)                                         # the default is accepted everywhere
        finally:
            h.close()
    h = lib.Handle.onlyunitdiag(A)
    try:
        for bad in (2, -1):
            with pytest.raises(lib.MsdpError, match="round_order") as e:
                h.set_option("round_order", bad)
            assert e.value.code == lib.EINVAL
        h.set_option("round_order", 1)
        with pytest.raises(lib.MsdpError) as e:                                    # the calls keep their own refusals
            h.round_hyperplane(np.ones((64, 2)), sweeps=1)
        assert e.value.code == lib.ESTATE
    finally:
        h.close()


# ------------------------------------------------------------------ 7. wrappers and solves
def test_wrappers_equal_the_handle_calls(lib):
    from manisdp_matlab_amd import solvers
    ref = _real_ref("torus", 7, 64, 50)
    x, value, info = solvers.round_unitdiag(_real("torus"), round_ref.table_point(65, 7), sweeps=50, R=round_ref.table_directions(64, 7),
                                            order="color")
    assert np.array_equal(x, ref["x"]) and value == ref["values"][ref["best"]] and np.array_equal(info["info"], ref["info"])
    case = PR.EXACT_CASES[1]
    storage, n, T, p, M, seed = case
    C = HR.instance(storage, n)
    Y, R = PR.inputs(n, p, T, seed)
    pref = _phase_ref(case, C, Y, R, M, 50)
    z, value, info = solvers.round_phases(C, Y, M=M, sweeps=50, R=R, order="color")
    assert np.array_equal(z, pref["z"]) and value == pref["values"][pref["best"]] and np.array_equal(info["info"], pref["info"])


def test_solves_with_the_colour_ordered_rounding(lib):
    from manisdp_matlab_amd import solvers
    C = _real("G11")
    Y, fval, data = solvers.ManiSDP_onlyunitdiag(C, {"p0": 20, "tol": 1e-8, "round": {"trials": 128, "sweeps": 50, "seed": 1, "order": "color"}},
                                                 verbose=False)
    r = data["round"]
    x = r["x"].astype(np.float64)
    print("G11, colour order: fval %.6f, rounded value %.1f, sweeps %s" % (fval, r["value"], r["info"][0].tolist()))
    assert r["value"] == float(x @ (C @ x)) == r["values"][r["best"]] == r["values"].min()
    h = lib.Handle.onlyunitdiag(C, pcap=max(32, Y.shape[1]))
    try:                                                                           # values0 of the same rounding, from the handle
        h.set_point(Y)
        res0 = h.round_hyperplane(np.random.default_rng(1).standard_normal((128, Y.shape[1])), sweeps=0)
    finally:
        h.close()
    assert r["value"] <= res0["values0"][r["best"]] and fval <= r["value"] + 1e-6 * (1 + abs(fval))
    m = PR.solve_instance("mpsk")
    Ch = m["C"]
    Yd, obj, dd = solvers.ManiSDP_onlyunitdiag(
        Ch, {"Y0": m["Y0"], "eig": "host", "round_phases": {"M": 4, "trials": 128, "sweeps": 20, "seed": 3, "order": "color"}}, verbose=False)
    rd = dd["round"]
    print("mpsk, colour order: obj %.8f, rounded value %.8f, sweeps %s" % (obj, rd["value"], rd["info"][0].tolist()))
    assert abs(rd["value"] - np.real(np.conj(rd["z"]) @ (Ch @ rd["z"]))) <= 1e-12 * _l1(Ch)
    assert rd["value"] == rd["values"][rd["best"]] and rd["value"] >= obj - 1e-6 * abs(obj)
    h = lib.Handle.onlyunitdiag_hermitian(Ch, pcap=max(32, Yd.shape[1]))
    try:
        h.set_point(Yd)
        res0 = h.round_phases(solvers._draw_phase_R(np.random.default_rng(3), 128, Yd.shape[1]), M=4, sweeps=0)
    finally:
        h.close()
    assert rd["value"] <= res0["values0"][rd["best"]] + 1e-12 * _l1(Ch)
    assert np.array_equal(rd["k"], np.round(np.angle(rd["z"]) / (2 * np.pi / 4)).astype(np.int64) % 4)
