"""msdp_round_phases and msdp_hfactor_gram / _rotate / _append on the device (the Hermitian kind, Handle.onlyunitdiag_hermitian)
against the NumPy restatement of tests/phase_round_ref.py, the real kind's msdp_round_hyperplane at B = 0, NumPy for the
re-shaping, and whole solves with options["hermitian_factor"] = "device" and options["round_phases"].

Equality is asked for where the arithmetic is exact (M = 2, 4 on entries in Z/4: every sum of the sweeps and of the values is
exact in fp64, and the rounding, the only inexact step, has a margin above 1e-9 max|w| -- tests/test_phase_round_ref_host.py
checks the margins of every instance used here).  Elsewhere: 1e-12 on phases, 1e-12 sum|C_ij| on values (the tolerance of
tests/test_gpu_hermitian.py for operator outputs), and for the M = 0 sweeps ten times the distance between the fp64
restatement and the same restatement in long double.

M = 8 sweeps run on phase_round_ref.generic_instance of the table instance, not on the table instance itself: with entries in
Z/4 and 8th roots of unity the candidates of the local search tie exactly, so no seed gives the margin above 1e-9 of the scale
that equal indices rest on (the rounding of M = 8 is checked on the table instance)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import hermitian_ref as HR
import phase_round_ref as PR
from test_phase_round_ref_host import real_case_inputs

pytestmark = pytest.mark.gpu
_REF = {}


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _ref(key, C, Y, R, M, sweeps, dtype=np.float64):
    """The restatement, computed once per (case, M, sweeps, dtype) and never modified."""
    k = (key, M, sweeps, np.dtype(dtype).name)
    if k not in _REF:
        _REF[k] = PR.round_phases(C, Y, R, M, sweeps, dtype=dtype)
    return _REF[k]


def _l1(C):
    return float(np.abs(sp.csr_matrix(C)).sum())


def _check_common(C, res, tol):
    """What holds in every case: the values are those of the returned phases, no value rose, z is the best column."""
    ph = res["phases"]
    assert np.max(np.abs(PR.host_values(C, ph) - res["values"])) <= tol
    assert np.all(res["values"] <= res["values0"] + tol)
    b = res["best"]
    assert b == int(np.argmin(res["values"]))
    assert np.array_equal(res["z"], ph[b // 64, :, b % 64])


# ------------------------------------------------------------------ 1. exact cases
@pytest.mark.parametrize("case", PR.EXACT_CASES)
def test_exact_cases_equal_the_restatement(lib, case):
    storage, n, T, p, M, seed = case
    C = HR.instance(storage, n)
    Y, R = PR.inputs(n, p, T, seed)
    h = lib.Handle.onlyunitdiag_hermitian(C, pcap=max(32, p))
    try:
        h.set_point(Y)
        for sweeps in PR.EXACT_SWEEPS:
            ref = _ref(case, C, Y, R, M, sweeps)
            res = h.round_phases(R, M=M, sweeps=sweeps, phases=True)
            print(case, "sweeps", sweeps, "info", res["info"].tolist(), "best", res["best"], "value", res["values"][res["best"]],
                  "phases differ at", int(np.sum(res["phases"] != ref["phases"])))
            assert np.array_equal(res["phases"], ref["phases"])
            assert np.array_equal(res["values0"], ref["values0"]) and np.array_equal(res["values"], ref["values"])
            assert np.array_equal(res["info"], ref["info"]) and res["best"] == ref["best"]
            assert np.array_equal(res["z"], ref["z"]) and np.array_equal(res["k"], ref["kbest"])
            _check_common(C, res, 0.0)
            if sweeps == 0:
                assert np.array_equal(res["values"], res["values0"]) and not res["info"].any()
            if sweeps == 50:
                assert np.all(res["info"][1] == 0) and np.all(res["info"][0] < 50) and np.all(res["info"][0] > 1)
    finally:
        h.close()


# ------------------------------------------------------------------ 2. the real kind at B = 0
@pytest.mark.parametrize("case", PR.REAL_CASES)
def test_zero_imaginary_parts_are_the_hyperplane_rounding(lib, case):
    storage, n, T, p, seed = case
    A, Yr, Rr = real_case_inputs(case)
    hr, hc = lib.Handle.onlyunitdiag(A, pcap=32), lib.Handle.onlyunitdiag_hermitian(A.astype(np.complex128), pcap=32)
    try:
        hr.set_point(Yr)
        hc.set_point(Yr.astype(np.complex128))
        for sweeps in (0, 1, 50):
            a = hr.round_hyperplane(Rr, sweeps=sweeps, masks=True)
            b = hc.round_phases(Rr.astype(np.complex128), M=2, sweeps=sweeps, phases=True)
            print(case, "sweeps", sweeps, "info", a["info"].tolist(), b["info"].tolist(), "best", a["best"], b["best"])
            assert np.all(b["phases"].imag == 0) and np.all(np.abs(b["phases"].real) == 1)
            bits = (a["masks"][:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
            assert np.array_equal(bits == 1, b["phases"].real == -1)               # a bit is set where z = -1
            assert np.array_equal(a["values0"], b["values0"]) and np.array_equal(a["values"], b["values"])
            assert np.array_equal(a["info"], b["info"]) and a["best"] == b["best"]
            assert np.array_equal(a["x"], b["z"].real.astype(np.int8)) and np.array_equal(b["k"], (a["x"] < 0).astype(np.int32))
    finally:
        hr.close(); hc.close()


# ------------------------------------------------------------------ 3. M = 0 and M = 8
@pytest.mark.parametrize("case", PR.TOL_CASES)
def test_circle_and_eight_psk_against_the_restatement(lib, case):
    storage, n, T, p, seed = case
    C = HR.instance(storage, n)
    G = PR.generic_instance(C)
    Y, R = PR.inputs(n, p, T, seed)
    tol = 1e-12 * _l1(C)
    h, hg = lib.Handle.onlyunitdiag_hermitian(C, pcap=max(32, p)), lib.Handle.onlyunitdiag_hermitian(G, pcap=max(32, p))
    try:
        h.set_point(Y); hg.set_point(Y)
        for M in (0, 8):                                                           # after the rounding
            ref = _ref(case, C, Y, R, M, 0)
            res = h.round_phases(R, M=M, sweeps=0, phases=True)
            print(case, "M", M, "rounding: phases %.2e values %.2e (tol %.2e)" % (
                np.max(np.abs(res["phases"] - ref["phases"])), np.max(np.abs(res["values"] - ref["values"])), tol))
            assert np.max(np.abs(res["phases"] - ref["phases"])) <= 1e-12
            assert np.max(np.abs(res["values"] - ref["values"])) <= tol and np.array_equal(res["values"], res["values0"])
            if M:
                assert np.array_equal(res["phases"], ref["phases"])                # equal indices: bit copies of one table
                assert np.array_equal(res["k"], ref["k"][res["best"] // 64, :, res["best"] % 64])
            _check_common(C, res, tol)
        # M = 8, the sweeps, on the generic values (module docstring)
        tolg = 1e-12 * _l1(G)
        ref = _ref((case, "generic"), G, Y, R, 8, PR.M8_SWEEPS)
        res = hg.round_phases(R, M=8, sweeps=PR.M8_SWEEPS, phases=True)
        print(case, "M 8 sweeps: info", res["info"].tolist(), ref["info"].tolist(), "phases differ at",
              int(np.sum(res["phases"] != ref["phases"])), "values %.2e" % np.max(np.abs(res["values"] - ref["values"])))
        assert np.array_equal(res["phases"], ref["phases"]) and np.array_equal(res["info"], ref["info"])
        assert np.array_equal(res["k"], ref["k"][res["best"] // 64, :, res["best"] % 64])
        assert np.max(np.abs(res["values"] - ref["values"])) <= tolg and np.max(np.abs(res["values0"] - ref["values0"])) <= tolg
        _check_common(G, res, tolg)
        # M = 0, the sweeps: within ten times the fp64 / long double distance of the restatement
        for s in PR.CIRCLE_SWEEPS:
            ref, refl = _ref(case, C, Y, R, 0, s), _ref(case, C, Y, R, 0, s, dtype=np.longdouble)
            yard = np.max(np.abs(ref["phases"] - refl["phases"]))
            res = h.round_phases(R, M=0, sweeps=s, phases=True)
            dist = np.max(np.abs(res["phases"] - ref["phases"]))
            print(case, "M 0, %d sweeps: device to fp64 restatement %.3e, fp64 to long double %.3e" % (s, dist, yard))
            assert dist <= 10.0 * yard
            assert np.all(res["info"][0] == s) and not res["info"][1].any()
            _check_common(C, res, tol)
            assert np.all(res["values"] < res["values0"])
    finally:
        h.close(); hg.close()


# ------------------------------------------------------------------ 4. call surface
def test_refusals_arguments_and_untouched_state(lib):
    from manisdp_matlab_amd import problems
    n, p = 203, 3
    C = HR.instance("hub", n)
    Y, R = PR.inputs(n, p, 64, 51)
    A = sp.csr_matrix(C.real)
    blockC, _, _ = problems.rotation_synchronization(20, 3, 4, 0.1, 1)
    for other, Yo in ((lib.Handle.onlyunitdiag(A), Y.real), (lib.Handle.onlyunitdiag(A.toarray()), Y.real),
                      (lib.Handle.onlyunitblockdiag(blockC, 3), None)):
        try:
            if Yo is not None:
                other.set_point(np.ascontiguousarray(Yo / np.linalg.norm(Yo, axis=1, keepdims=True)))
            with pytest.raises(lib.MsdpError, match="round_phases") as e:
                other.round_phases(R, M=2)
            assert e.value.code == lib.EUNSUPPORTED
            for call in (lambda: other.hfactor_gram(), lambda: other.hfactor_rotate(np.eye(3)), lambda: other.hfactor_append(np.ones((other.n, 1)), 0.5)):
                with pytest.raises(lib.MsdpError, match="hfactor_") as e:
                    call()
                assert e.value.code == lib.EUNSUPPORTED
        finally:
            other.close()
    h = lib.Handle.onlyunitdiag_hermitian(C, pcap=8)
    try:
        for call in (lambda: h.round_phases(R), lambda: h.hfactor_gram(), lambda: h.hfactor_rotate(np.eye(3)),
                     lambda: h.hfactor_append(np.ones((n, 1)), 0.5)):
            with pytest.raises(lib.MsdpError, match="no resident point") as e:
                call()
            assert e.value.code == lib.ESTATE
        h.set_point(Y)
        f0 = h.cost()
        pool0 = lib.pool_stats()
        for kw in (dict(M=1), dict(M=65), dict(M=-2), dict(sweeps=-1)):
            with pytest.raises(lib.MsdpError, match="round_phases") as e:
                h.round_phases(R, **kw)
            assert e.value.code == lib.EINVAL
        for T in (0, 32, 96, lib.ROUND_PHASES_MAX_TRIALS + 64):
            with pytest.raises(lib.MsdpError, match="round_phases") as e:
                h.round_phases(np.ones((T, p), dtype=np.complex128))
            assert e.value.code == lib.EINVAL
        # null R / values / best, and k with M = 0, through the raw call
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        Rb, vals, best, kk = R.view(np.float64), np.zeros(64), ctypes.c_int32(), np.zeros(n, dtype=np.int32)
        raw = h._lib.msdp_round_phases
        args = lambda M, Rp, vp, bp, kp: (h._h, M, 64, Rp, 0, None, vp, None, None, bp, None, kp)
        assert raw(*args(0, None, vals.ctypes.data_as(dp), ctypes.byref(best), None)) == lib.EINVAL
        assert raw(*args(0, Rb.ctypes.data_as(dp), None, ctypes.byref(best), None)) == lib.EINVAL
        assert raw(*args(0, Rb.ctypes.data_as(dp), vals.ctypes.data_as(dp), None, None)) == lib.EINVAL
        assert raw(*args(0, Rb.ctypes.data_as(dp), vals.ctypes.data_as(dp), ctypes.byref(best), kk.ctypes.data_as(ip))) == lib.EINVAL
        assert raw(*args(0, Rb.ctypes.data_as(dp), vals.ctypes.data_as(dp), ctypes.byref(best), None)) == 0      # every optional output NULL
        assert raw(*args(4, Rb.ctypes.data_as(dp), vals.ctypes.data_as(dp), ctypes.byref(best), kk.ctypes.data_as(ip))) == 0
        assert best.value == int(np.argmin(vals)) and kk.min() >= 0 and kk.max() <= 3
        # the handle is as it was
        for M, sweeps in ((0, 2), (4, 5)):
            h.round_phases(R, M=M, sweeps=sweeps, phases=True)
            assert np.array_equal(h.get_point(), Y) and h.cost() == f0
        assert lib.pool_stats() == pool0
        assert abs(f0 - HR.cost(C, Y)) <= 1e-12 * abs(f0)
        assert np.linalg.norm(h.rgrad() - HR.rgrad(C, Y)) <= 1e-12 * np.linalg.norm(HR.rgrad(C, Y))    # the cost state still serves
    finally:
        h.close()


# ------------------------------------------------------------------ 5. the re-shaping
def _check_state(h, C, Y):
    """cost, gradient and Hess-vec of the handle are those of the restatement at Y: the adopted width is right."""
    n, p = Y.shape
    U = HR.table_direction(n, p)
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
    assert h.p == p
    assert np.max(np.abs(h.get_point() - Y)) <= 1e-12
    assert abs(h.cost() - HR.cost(C, Y)) <= 1e-12 * max(1.0, abs(HR.cost(C, Y)))
    assert rel(h.rgrad(), HR.rgrad(C, Y)) < 1e-12 and rel(h.hessvec(U), HR.hessvec(C, Y, U)) < 1e-12


@pytest.mark.parametrize("storage,n", [("grid", 203), ("hub", 1031)])
def test_hfactor_calls_against_numpy(lib, storage, n):
    C = HR.instance(storage, n)
    pcap = max(HR.P_GRID) + 2
    h = lib.Handle.onlyunitdiag_hermitian(C, pcap=pcap)
    g = np.random.default_rng(61)
    try:
        for p in HR.P_GRID:
            Y = HR.table_point(n, p)
            h.set_point(Y)
            h.cost()
            G = h.hfactor_gram()
            Gref = Y.conj().T @ Y
            assert G.shape == (p, p) and G.dtype == np.complex128
            assert np.linalg.norm(G - Gref) <= 1e-12 * np.linalg.norm(Gref), p
            assert np.array_equal(h.get_point(), Y)
            # the cut: an orthonormal Q of r columns (r = p, and r < p where p allows it)
            for r in sorted({p, max(1, p // 2)}):
                h.set_point(Y)
                Q = np.linalg.qr(g.standard_normal((p, p)) + 1j * g.standard_normal((p, p)))[0][:, :r]
                h.hfactor_rotate(Q)
                Yq = Y @ Q
                assert np.max(np.abs(h.get_point() - Yq)) <= 1e-12, (p, r)
                _check_state(h, C, Yq)
            # the widening by k = 1 and 2 columns as msdp_escape_eigs lays them out
            for k in (1, 2):
                h.set_point(Y)
                V = g.standard_normal((n, k)) + 1j * g.standard_normal((n, k))
                h.hfactor_append(V, 0.5)
                Ya = np.hstack([Y, 0.5 * V])
                Ya = Ya / np.sqrt(np.sum(np.abs(Ya) ** 2, axis=1, keepdims=True))
                assert np.max(np.abs(h.get_point() - Ya)) <= 1e-12, (p, k)
                _check_state(h, C, Ya)
        # r outside 1..p
        Y = HR.table_point(n, 3)
        h.set_point(Y)
        for bad in (np.zeros((3, 0)), np.ones((3, 4))):
            with pytest.raises(lib.MsdpError, match="hfactor_rotate") as e:
                h.hfactor_rotate(bad)
            assert e.value.code == lib.EINVAL
        # over the capacity: refused with nothing modified
        Y = HR.table_point(n, pcap - 1)
        h.set_point(Y)
        f0 = h.cost()
        with pytest.raises(lib.MsdpError, match="allocated capacity") as e:
            h.hfactor_append(np.ones((n, 2), dtype=np.complex128), 0.5)
        assert e.value.code == lib.EUNSUPPORTED
        assert np.array_equal(h.get_point(), Y) and h.cost() == f0
        h.hfactor_append(np.ones((n, 1), dtype=np.complex128), 0.5)              # exactly the capacity is taken
        assert h.p == pcap
        # the real calls stay refused
        for call in (lambda: h.factor_gram(), lambda: h.factor_rotate(np.eye(h.p)), lambda: h.factor_append(np.ones((n, 1)), 0.5)):
            with pytest.raises(lib.MsdpError, match="Hermitian") as e:
                call()
            assert e.value.code == lib.EUNSUPPORTED
    finally:
        h.close()


# ------------------------------------------------------------------ 6. solves
@pytest.mark.parametrize("name", ["sync", "mpsk", "sync3"])
def test_solves_with_the_device_factor_and_the_rounding(lib, name):
    """The phase-error comparison allows 1e-6: on a rank-1 solution the device rounding and Y[:, 0] / |Y[:, 0]| are the same
    phases up to a global one, so their errors differ by rounding and by the gradient tolerance of the solve only -- "no larger"
    is asked up to the accuracy the two solves themselves agree to."""
    from manisdp_matlab_amd import problems, solvers
    m = PR.solve_instance(name)
    C, M = m["C"], m["M"]
    base = {"Y0": m["Y0"], "eig": "host"}
    Yh, objh, dh = solvers.ManiSDP_onlyunitdiag(C, dict(base), verbose=False)
    Yd, objd, dd = solvers.ManiSDP_onlyunitdiag(
        C, dict(base, hermitian_factor="device", round_phases={"M": M, "trials": 128, "sweeps": 20, "seed": 3}), verbose=False)
    rank = lambda Y: int(np.sum(np.linalg.svd(Y, compute_uv=False) >= 0.1 * np.linalg.svd(Y, compute_uv=False)[0]))   # theta of the solve
    rd = dd["round"]
    print(name, "host %.10f (%d iterations, rank %d) device %.10f (%d iterations, rank %d) restatement %.10f; rounded %.10f" % (
        objh, dh["iters"], rank(Yh), objd, dd["iters"], rank(Yd), m["obj"], rd["value"]))
    assert dh["status"] == 0 and dd["status"] == 0
    assert abs(objd - objh) <= 1e-6 * abs(objh) and abs(objh - m["obj"]) <= 1e-6 * abs(m["obj"])
    assert rank(Yd) == rank(Yh) == m["data"]["rank"] and dd["iters"] == dh["iters"]
    assert rd["value"] >= objd - 1e-6 * abs(objd)                                  # the SDP optimum is a lower bound
    assert abs(rd["value"] - np.real(np.conj(rd["z"]) @ (C @ rd["z"]))) <= 1e-12 * _l1(C)
    assert np.max(np.abs(np.abs(rd["z"]) - 1.0)) <= 1e-12
    if name == "sync3":
        return                                                                     # (not rank 1: the bound is all that is known)
    if M == 0:
        assert abs(rd["value"] - objd) <= 1e-6 * abs(objd)                         # rank 1, unit circle: the rounding attains the bound
    u = Yd[:, 0] / np.abs(Yd[:, 0])
    err_dev, err_host = problems.phase_error(rd["z"], m["z"], M), problems.phase_error(u, m["z"], 0)
    print(name, "phase error: device %.6e, host rounding %.6e" % (err_dev, err_host))
    assert err_dev <= err_host + 1e-6
    if M:
        assert np.array_equal(rd["k"], np.round(np.angle(rd["z"]) / (2 * np.pi / M)).astype(np.int64) % M)
