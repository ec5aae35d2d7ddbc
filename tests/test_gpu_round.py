"""msdp_round_hyperplane on the device against the NumPy restatement of tests/round_ref.py.

The sparse instances have entries that are multiples of 1/4, so every sum is exact in fp64 in any order and the device must
reproduce the reference bit for bit: sign masks, values, and -- after 1, 2 and 50 sweeps -- the whole flip trajectory of the
1-opt search with its per-word sweep and flip counts.  On the dense instance with real weights the masks of the rounding are
still exact (tests/test_round_ref_host.py: no dot of the table is within 1e-10 of zero) and everything else holds within
nnz * 2^-52 * sum |C_ij|, the bound on reordering a sum of nnz terms."""
import numpy as np
import pytest
import round_ref
from conftest import golden_path

pytestmark = pytest.mark.gpu

SWEEPS = (1, 2, 50)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


_CACHE = {}


def _cost(name):
    if name not in _CACHE:
        _CACHE[name] = round_ref.instance(name, golden_path)
    return _CACHE[name]


def _reference(name, p, T, sweeps):
    key = (name, p, T, sweeps)
    if key not in _CACHE:
        C = _cost(name)
        _CACHE[key] = round_ref.round_hyperplane(C, round_ref.table_point(C.shape[0], p), round_ref.table_directions(T, p), sweeps)
    return _CACHE[key]


def _handle(lib, name, p):
    C = _cost(name)
    h = lib.Handle.onlyunitdiag(C)
    h.set_point(round_ref.table_point(C.shape[0], p))
    return h


def _cases(names):
    return [(name, p, T) for name, n, p, T in round_ref.table() if name in names]


def _pin_through_cost(lib, name, res, exact):
    """x of the best trial as a p = 1 point: the handle's own cost kernel must give the value the rounding reported.  The
    handle's cost is the reference's, 0.5 <C, Y Y'> (ManiSDP_onlyunitdiag.m:120), so twice it is x' C x (doubling is exact)."""
    C = _cost(name)
    h1 = lib.Handle.onlyunitdiag(C)
    try:
        h1.set_point(res["x"].astype(np.float64)[:, None])
        f = 2.0 * h1.cost()
    finally:
        h1.close()
    v = res["values"][res["best"]]
    if exact:
        assert f == v
    else:
        assert abs(f - v) <= round_ref.reorder_bound(C)


@pytest.mark.parametrize("name,p,T", _cases(round_ref.SPARSE))
def test_exact_parity_on_quarter_weights(lib, name, p, T):
    h = _handle(lib, name, p)
    try:
        R = round_ref.table_directions(T, p)
        Y0, f0 = h.get_point(), h.cost()
        got = h.round_hyperplane(R, sweeps=0, masks=True)
        ref = _reference(name, p, T, 0)
        assert np.array_equal(got["masks"], ref["masks"])
        assert np.array_equal(got["values0"], ref["values0"]) and np.array_equal(got["values"], ref["values0"])
        assert not got["info"].any()
        for sweeps in SWEEPS:
            got = h.round_hyperplane(R, sweeps=sweeps, masks=True)
            ref = _reference(name, p, T, sweeps)
            assert np.array_equal(got["masks"], ref["masks"]), sweeps
            assert np.array_equal(got["values0"], ref["values0"]) and np.array_equal(got["values"], ref["values"]), sweeps
            assert np.array_equal(got["info"], ref["info"]), (sweeps, got["info"], ref["info"])
            assert got["best"] == ref["best"] == int(np.argmin(got["values"]))
            assert np.array_equal(got["x"], round_ref.unpack(got["masks"])[got["best"]].astype(np.int8))
        again = h.round_hyperplane(R, sweeps=SWEEPS[-1], masks=True)          # two identical calls, identical bytes
        for k in ("values0", "values", "info", "x", "masks"):
            assert again[k].tobytes() == got[k].tobytes(), k
        assert again["best"] == got["best"]
        assert np.array_equal(h.get_point(), Y0) and h.cost() == f0            # the handle is as it was
    finally:
        h.close()
    _pin_through_cost(lib, name, got, exact=True)


@pytest.mark.parametrize("name,p,T", _cases(("dense96",)))
def test_real_weights_within_the_reordering_bound(lib, name, p, T):
    C = _cost(name)
    bound = round_ref.reorder_bound(C)
    h = _handle(lib, name, p)
    try:
        R = round_ref.table_directions(T, p)
        Y0, f0 = h.get_point(), h.cost()
        got0 = h.round_hyperplane(R, sweeps=0, masks=True)
        ref = _reference(name, p, T, 0)
        assert np.array_equal(got0["masks"], ref["masks"])
        assert np.max(np.abs(got0["values0"] - ref["values0"])) <= bound
        assert np.array_equal(got0["values"], got0["values0"])
        offdiag = C - np.diag(np.diag(C))
        row_bound = np.count_nonzero(C, axis=1) * 2.0 ** -52 * np.sum(np.abs(C), axis=1)     # nnz_i * 2^-52 * sum_j |C_ij|
        for sweeps in SWEEPS:
            got = h.round_hyperplane(R, sweeps=sweeps, masks=True)
            X = round_ref.unpack(got["masks"])
            assert np.array_equal(got["values0"], got0["values0"])
            assert np.all(got["values"] <= got["values0"] + bound)
            assert np.max(np.abs(got["values"] - round_ref.values(C, X))) <= bound
            assert np.all(got["info"][0] >= 1) and np.all(got["info"][0] <= sweeps)
            done = np.repeat(got["info"][1] == 0, 64)                          # words that report a sweep without a flip
            assert np.all((X * (X @ offdiag))[done] <= row_bound[None, :])
            assert got["best"] == int(np.argmin(got["values"]))
            assert np.array_equal(got["x"], X[got["best"]].astype(np.int8))
        again = h.round_hyperplane(R, sweeps=SWEEPS[-1], masks=True)
        for k in ("values0", "values", "info", "x", "masks"):
            assert again[k].tobytes() == got[k].tobytes(), k
        assert np.array_equal(h.get_point(), Y0) and h.cost() == f0
    finally:
        h.close()
    _pin_through_cost(lib, name, got, exact=False)


@pytest.mark.parametrize("name", ["torus", "dense96"])
def test_rtr_after_the_rounding_is_what_it_is_without(lib, name):
    p, T = 7, 64
    opts = dict(maxiter=5, maxinner=20, tolgradnorm=1e-9)
    ha, hb = _handle(lib, name, p), _handle(lib, name, p)
    try:
        ha.round_hyperplane(round_ref.table_directions(T, p), sweeps=3)
        sa, sb = ha.rtr(lib.default_opts(**opts)), hb.rtr(lib.default_opts(**opts))
        da, db = sa.as_dict(), sb.as_dict()
        for k in da:
            if k != "seconds":
                assert da[k] == db[k], k
        assert np.array_equal(ha.get_point(), hb.get_point())
    finally:
        ha.close()
        hb.close()


def test_refusals(lib):
    from manisdp_matlab_amd import problems
    h = lib.Handle.onlyunitdiag(_cost("torus"))
    try:
        with pytest.raises(lib.MsdpError) as e:                                # no point yet
            h.round_hyperplane(np.ones((64, 2)))
        assert e.value.code == lib.ESTATE
        h.set_point(round_ref.table_point(65, 2))
        for T, sweeps in ((65, 0), (0, 0), (lib.ROUND_MAX_TRIALS + 64, 0), (64, -1)):
            with pytest.raises(lib.MsdpError) as e:
                h.round_hyperplane(np.ones((T, 2)), sweeps=sweeps)
            assert e.value.code == lib.EINVAL, (T, sweeps)
        assert h.round_hyperplane(np.ones((64, 2)))["values"].shape == (64,)   # the handle still works
    finally:
        h.close()
    At, b, c, K = problems.theta_problem(8, seed=1)
    ha = lib.Handle.affine(lib.KIND_UNITTRACE, At, b, c, K["s"])
    try:
        with pytest.raises(lib.MsdpError) as e:
            ha.round_hyperplane(np.ones((64, 2)))
        assert e.value.code == lib.EUNSUPPORTED
    finally:
        ha.close()


def test_round_unitdiag_wrapper(lib):
    from manisdp_matlab_amd import solvers
    C = _cost("torus")
    Y, R = round_ref.table_point(65, 7), round_ref.table_directions(64, 7)
    x, value, info = solvers.round_unitdiag(C, Y, sweeps=50, R=R)
    ref = _reference("torus", 7, 64, 50)
    assert np.array_equal(x, ref["x"]) and value == ref["values"][ref["best"]] and np.array_equal(info["info"], ref["info"])
    x2, value2, info2 = solvers.round_unitdiag(C, Y, trials=128, sweeps=0, rng=np.random.default_rng(4))
    ref2 = round_ref.round_hyperplane(C, Y, np.random.default_rng(4).standard_normal((128, 7)), 0)
    assert value2 == ref2["values"][ref2["best"]] and info2["values"].shape == (128,)


def test_end_to_end_on_G1(lib):
    """Unit weights, so the Goemans-Williamson bound applies: the best of 256 rounded cuts, locally improved, is within 0.87856
    of the SDP bound (both negative: value <= 0.87856 fval), and is the weight of a real cut counted from the edge list."""
    from manisdp_matlab_amd import problems, solvers
    C = _cost("G1")
    Y, fval, data = solvers.ManiSDP_onlyunitdiag(C, {"p0": 40, "tol": 1e-8, "round": {"trials": 256, "sweeps": 50, "seed": 1}},
                                                 verbose=False)
    r = data["round"]
    value, x = r["value"], r["x"].astype(np.float64)
    print("G1: fval %.6f, rounded value %.1f, ratio %.4f, sweeps %s" % (fval, value, value / fval, r["info"][0]))
    assert set(r) == {"x", "value", "values", "best", "info"} and r["values"].shape == (256,) and x.shape == (800,)
    assert value == r["values"][r["best"]] == r["values"].min()
    assert fval <= value + 1e-6 * (1 + abs(fval))
    assert value == round(value)
    nv, i, j, w = problems.read_gset(golden_path("G1.txt.gz"))
    assert -value == float(np.sum(w[x[i] != x[j]]))
    assert value <= 0.87856 * fval
    # without the option nothing changes
    Y2, fval2, data2 = solvers.ManiSDP_onlyunitdiag(C, {"p0": 40, "tol": 1e-8}, verbose=False)
    assert "round" not in data2 and abs(fval2 - fval) <= 1e-6 * (1 + abs(fval))
