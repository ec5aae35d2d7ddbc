"""The sparse-plus-low-rank cost kind C = Cs + V diag(s) V' on the device (msdp_create_onlyunitdiag_csc_lowrank) against the
dense handle of the same matrix, the CPU oracle and the NumPy restatement of tests/lowrank_ref.py: derivatives over every
instance of the row kernels, the identity with the plain sparse handle at s = 0, one trustregions() call, the Lanczos escape, a
whole solve of a modularity instance, the rounding (bit for bit on the quarter-valued instances) and the refusals.

Tolerances are those of tests/test_gpu_onlyunitdiag.py and tests/test_gpu_dense.py for the same quantities against the oracle
(1e-12 relative on operator outputs; counts equal and the cost to 1e-11 for a trustregions() call; 1e-6 on a solve's optimum)
and those of tests/test_gpu_escape.py for the Lanczos path."""
import numpy as np
import pytest
import scipy.sparse as sp

import lowrank_ref
import round_ref

pytestmark = pytest.mark.gpu

SWEEPS = (1, 2, 50)
MOD_SEED = 5                 # planted partition: n = 300, p_in = 0.10, p_out = 0.02 (the oracle reaches status 0 in two iterations)
MOD_SHARE = 1.0              # share of the planted labels the restatement's rounding (256 trials, 50 sweeps, seed 1) of the oracle's
                             # solution recovers on that instance, computed on the CPU


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _relerr(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _lowrank_handle(lib, C, pcap=32):
    return lib.Handle.onlyunitdiag_lowrank(C.Cs, C.V, C.s, pcap=pcap)


# ------------------------------------------------------------------ derivatives
@pytest.mark.parametrize("storage", lowrank_ref.STORAGES)
@pytest.mark.parametrize("q", lowrank_ref.Q_GRID)
@pytest.mark.parametrize("n", lowrank_ref.N_GRID)
def test_derivatives_against_dense_handle_oracle_and_restatement(lib, n, q, storage):
    from oracle import manisdp_ref as R
    C, Cd = lowrank_ref.instance(storage, n, q)
    h, hd = _lowrank_handle(lib, C, pcap=max(lowrank_ref.P_GRID)), lib.Handle.onlyunitdiag(Cd, pcap=max(lowrank_ref.P_GRID))
    try:
        for p in lowrank_ref.P_GRID:
            Y, U = lowrank_ref.table_point(n, p), lowrank_ref.table_direction(n, p)
            h.set_point(Y); hd.set_point(Y)
            f, G, H, z = h.cost(), h.rgrad(), h.hessvec(U), h.get_z()
            prob = R._OnlyUnitDiagProblem(Cd, n, p)
            f_ref = prob.cost(Y)
            args = (C.Cs, C.V, C.s)
            print("n %d q %d %s p %d: cost %.2e grad %.2e hess %.2e z %.2e" % (
                n, q, storage, p, abs(f - f_ref) / max(1.0, abs(f_ref)), _relerr(G, prob.grad(Y)),
                _relerr(H, R.hessvec_onlyunitdiag(Cd, Y, U)), _relerr(z, np.sum((Cd @ Y) * Y, axis=1))))
            # the CPU oracle on the dense equivalent
            assert abs(f - f_ref) <= 1e-12 * max(1.0, abs(f_ref)), p
            assert _relerr(G, prob.grad(Y)) < 1e-12, p
            assert _relerr(H, R.hessvec_onlyunitdiag(Cd, Y, U)) < 1e-12, p
            assert _relerr(z, np.sum((Cd @ Y) * Y, axis=1)) < 1e-12, p
            # the restatement in the split form
            assert abs(f - lowrank_ref.cost(*args, Y)) <= 1e-12 * max(1.0, abs(f_ref)), p
            assert _relerr(G, lowrank_ref.rgrad(*args, Y)) < 1e-12 and _relerr(H, lowrank_ref.hessvec(*args, Y, U)) < 1e-12, p
            assert _relerr(z, lowrank_ref.get_z(*args, Y)) < 1e-12, p
            # the dense handle of .toarray() at the same point and direction
            assert abs(f - hd.cost()) <= 1e-12 * max(1.0, abs(f_ref)), p
            assert _relerr(G, hd.rgrad()) < 1e-12 and _relerr(H, hd.hessvec(U)) < 1e-12 and _relerr(z, hd.get_z()) < 1e-12, p
            assert np.array_equal(H, h.hessvec(U)) and np.array_equal(G, h.rgrad())       # fixed summation orders, no atomics
    finally:
        h.close(); hd.close()


@pytest.mark.parametrize("storage", lowrank_ref.STORAGES)
@pytest.mark.parametrize("p", lowrank_ref.P_WIDE)
def test_derivatives_beyond_the_lds_staged_widths(lib, p, storage):
    """Row instances wider than 128 columns read T = diag(s) V' X in place (no LDS copy, a bounds test per column chunk): the
    same comparisons as above at n = 203, q = 3 and 8."""
    from oracle import manisdp_ref as R
    n = 203
    for q in (3, 8):
        C, Cd = lowrank_ref.instance(storage, n, q)
        Y, U = lowrank_ref.table_point(n, p), lowrank_ref.table_direction(n, p)
        h, hd, hs = _lowrank_handle(lib, C, pcap=p), lib.Handle.onlyunitdiag(Cd, pcap=p), None
        try:
            h.set_point(Y); hd.set_point(Y)
            f, G, H, z = h.cost(), h.rgrad(), h.hessvec(U), h.get_z()
            prob = R._OnlyUnitDiagProblem(Cd, n, p)
            f_ref = prob.cost(Y)
            args = (C.Cs, C.V, C.s)
            print("n %d q %d %s p %d: cost %.2e grad %.2e hess %.2e" % (n, q, storage, p, abs(f - f_ref) / max(1.0, abs(f_ref)),
                                                                    _relerr(G, prob.grad(Y)), _relerr(H, R.hessvec_onlyunitdiag(Cd, Y, U))))
            assert abs(f - f_ref) <= 1e-12 * max(1.0, abs(f_ref))
            assert _relerr(G, prob.grad(Y)) < 1e-12 and _relerr(H, R.hessvec_onlyunitdiag(Cd, Y, U)) < 1e-12
            assert _relerr(z, np.sum((Cd @ Y) * Y, axis=1)) < 1e-12
            assert _relerr(G, lowrank_ref.rgrad(*args, Y)) < 1e-12 and _relerr(H, lowrank_ref.hessvec(*args, Y, U)) < 1e-12
            assert _relerr(G, hd.rgrad()) < 1e-12 and _relerr(H, hd.hessvec(U)) < 1e-12 and _relerr(z, hd.get_z()) < 1e-12
            hs = lib.Handle.onlyunitdiag_lowrank(C.Cs, C.V, np.zeros(q), pcap=p)      # s = 0: the sparse handle to the bit
            h0 = lib.Handle.onlyunitdiag(C.Cs, pcap=p)
            try:
                hs.set_point(Y); h0.set_point(Y)
                assert hs.cost() == h0.cost() and np.array_equal(hs.rgrad(), h0.rgrad()) and np.array_equal(hs.hessvec(U), h0.hessvec(U))
            finally:
                h0.close()
        finally:
            h.close(); hd.close()
            if hs is not None:
                hs.close()


@pytest.mark.parametrize("storage", lowrank_ref.STORAGES)
@pytest.mark.parametrize("n", lowrank_ref.N_GRID)
def test_zero_term_is_the_sparse_handle_bit_for_bit(lib, n, storage):
    """With s = 0 the low-rank instances add exact zeros behind the same sparse gather: cost, gradient, Hess-vec and z equal the
    plain sparse handle's to the bit."""
    C, _ = lowrank_ref.instance(storage, n, 3)
    h, hs = lib.Handle.onlyunitdiag_lowrank(C.Cs, C.V, np.zeros(3), pcap=max(lowrank_ref.P_GRID)), lib.Handle.onlyunitdiag(C.Cs, pcap=max(lowrank_ref.P_GRID))
    try:
        for p in lowrank_ref.P_GRID:
            Y, U = lowrank_ref.table_point(n, p), lowrank_ref.table_direction(n, p)
            h.set_point(Y); hs.set_point(Y)
            assert h.cost() == hs.cost(), p
            assert np.array_equal(h.rgrad(), hs.rgrad()), p
            assert np.array_equal(h.hessvec(U), hs.hessvec(U)), p
            assert np.array_equal(h.get_z(), hs.get_z()), p
    finally:
        h.close(); hs.close()


# ------------------------------------------------------------------ trustregions()
@pytest.mark.parametrize("n,p,q,storage", [(203, 5, 3, "grid"), (1031, 17, 8, "hub"), (1031, 33, 1, "grid")])
def test_rtr_matches_the_oracle_on_the_dense_matrix(lib, n, p, q, storage):
    from oracle import manisdp_ref as R, manopt_rtr
    C, Cd = lowrank_ref.instance(storage, n, q)
    Y = lowrank_ref.table_point(n, p)
    prob = R._OnlyUnitDiagProblem(Cd, n, p, q1="correct")
    _, f_ref, info = manopt_rtr.trustregions(prob, Y.copy(), 3, 20, 1e-8)
    h = _lowrank_handle(lib, C, pcap=p)
    try:
        h.set_point(Y)
        assert h.tcg_path() == 0 and h.persist_form() == -1                  # the generic per-iteration path
        st = h.rtr(lib.default_opts(maxiter=3, maxinner=20, tolgradnorm=1e-8))
        print("rtr: device", (st.iters, st.hessvecs, st.accepted, st.rejected, st.cost), "oracle",
              (info.iters, info.hessvecs, info.accepted, info.rejected, f_ref))
        assert (st.iters, st.hessvecs, st.accepted, st.rejected) == (info.iters, info.hessvecs, info.accepted, info.rejected)
        assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
        assert abs(h.cost() - st.cost) < 1e-10 * max(1.0, abs(st.cost))
        assert h.tcg_path() == 0 and h.persist_form() == -1
    finally:
        h.close()


# ------------------------------------------------------------------ escape
@pytest.mark.parametrize("n,p,q,storage", [(1031, 6, 3, "grid"), (203, 4, 8, "hub")])
def test_escape_eigs_against_lapack(lib, n, p, q, storage):
    C, Cd = lowrank_ref.instance(storage, n, q)
    Y = lowrank_ref.table_point(n, p)                                        # not a stationary point: S*Y != 0
    h = _lowrank_handle(lib, C)
    try:
        h.set_point(Y)
        z = h.get_z()
        k = 4
        lam, V, lmax, its = h.escape_eigs(k, tol=1e-9, maxit=600)
        assert h.escape_method() == 0                                        # Lanczos: the block eigen-solver stays sparse-only
    finally:
        h.close()
    S = Cd - np.diag(z)
    dS = np.linalg.eigh(S)[0]
    scale = max(abs(dS[0]), abs(dS[-1]))
    print("escape: lmax err %.2e lmin err %.2e (scale %.3f, %d steps)" % (abs(lmax - dS[-1]), abs(lam[0] - dS[0]), scale, its))
    assert abs(lmax - dS[-1]) < 1e-5 * scale
    assert abs(lam[0] - dS[0]) < 1e-8 * scale
    for t in range(k):
        if lam[t] < -1e-9 * scale:
            v = V[:, t]
            assert abs(np.linalg.norm(v) - 1.0) < 1e-8
            assert np.linalg.norm(S @ v - lam[t] * v) < 1e-5 * scale
            assert np.min(np.abs(dS - lam[t])) < 1e-8 * scale
    assert lam[0] < 0


# ------------------------------------------------------------------ solve
_MOD = {}


def _modularity_instance():
    if not _MOD:
        from manisdp_matlab_amd import problems
        from oracle import manisdp_ref as R
        A, labels = lowrank_ref.planted_partition(300, 0.10, 0.02, MOD_SEED)
        C = problems.modularity(A)
        Y0 = lowrank_ref.table_point(300, 2)
        _, obj_ref, data_ref = R.ManiSDP_onlyunitdiag(C.toarray(), {"Y0": Y0}, q1="correct")
        assert data_ref["status"] == 0 and data_ref["dinf"] < 1e-8
        _MOD.update(A=A, labels=labels, C=C, Y0=Y0, obj_ref=obj_ref)
    return _MOD


@pytest.mark.parametrize("eig", ["host", "device"])
def test_modularity_solve_matches_dense_solve_and_oracle(lib, eig):
    from manisdp_matlab_amd import solvers
    m = _modularity_instance()
    C, Y0 = m["C"], m["Y0"]
    Y, obj, data = solvers.ManiSDP_onlyunitdiag(C, {"Y0": Y0, "eig": eig}, verbose=False)
    assert data["status"] == 0 and data["dinf"] < 1e-8
    if "dense_obj" not in m:
        _, m["dense_obj"], dd = solvers.ManiSDP_onlyunitdiag(C.toarray(), {"Y0": Y0}, verbose=False)
        assert dd["status"] == 0 and dd["dinf"] < 1e-8
    print("modularity solve (%s): %.10f, dense C %.10f, oracle %.10f" % (eig, obj, m["dense_obj"], m["obj_ref"]))
    assert abs(obj - m["dense_obj"]) < 1e-6 * abs(m["dense_obj"])
    assert abs(obj - m["obj_ref"]) < 1e-6 * abs(m["obj_ref"])
    assert data["S"] is not None and data["S"].shape == (300, 300)           # n <= dense_X_max
    if eig == "device":
        assert data["escape_method"] == 0
        _, _, d2 = solvers.ManiSDP_onlyunitdiag(C, {"Y0": Y0, "eig": "device", "dense_X_max": 100}, verbose=False)
        assert d2["S"] is None and d2["X"] is None


def test_round_option_recovers_the_planted_partition(lib):
    from manisdp_matlab_amd import solvers
    m = _modularity_instance()
    Y, obj, data = solvers.ManiSDP_onlyunitdiag(m["C"], {"Y0": m["Y0"], "round": {"trials": 256, "sweeps": 50, "seed": 1}}, verbose=False)
    r = data["round"]
    x = r["x"].astype(np.float64)
    share = max(np.mean(x == m["labels"]), np.mean(x == -m["labels"]))
    print("modularity: bound %.6f, labels %.6f, share %.4f" % (-obj / (2 * m["A"].sum()), lowrank_ref.modularity_value(m["A"], x), share))
    assert r["value"] == r["values"][r["best"]] == r["values"].min()
    assert abs(r["value"] - x @ m["C"].matvec(x)) <= 1e-9 * abs(r["value"])
    assert obj <= r["value"] + 1e-6 * (1 + abs(obj))                        # the SDP bounds every labelling
    assert share >= MOD_SHARE


# ------------------------------------------------------------------ rounding
def _round_reference(storage, n, q, p, T, sweeps, cache={}):
    key = (storage, n, q, p, T, sweeps)
    if key not in cache:
        C, _ = lowrank_ref.instance(storage, n, q)
        cache[key] = lowrank_ref.round_hyperplane(C, lowrank_ref.table_point(n, p), round_ref.table_directions(T, p), sweeps)
    return cache[key]


@pytest.mark.parametrize("T", lowrank_ref.ROUND_T)
@pytest.mark.parametrize("p", lowrank_ref.ROUND_P)
@pytest.mark.parametrize("n,q,storage", [(203, 1, "grid"), (203, 3, "hub"), (203, 8, "grid"), (203, 8, "hub"), (1031, 3, "grid"), (1031, 8, "hub")])
def test_rounding_is_the_restatement_bit_for_bit(lib, n, q, storage, p, T):
    C, _ = lowrank_ref.instance(storage, n, q)
    h = _lowrank_handle(lib, C)
    try:
        h.set_point(lowrank_ref.table_point(n, p))
        R = round_ref.table_directions(T, p)
        Y0, f0 = h.get_point(), h.cost()
        got = h.round_hyperplane(R, sweeps=0, masks=True)
        ref = _round_reference(storage, n, q, p, T, 0)
        assert np.array_equal(got["masks"], ref["masks"])
        assert np.array_equal(got["values0"], ref["values0"]) and np.array_equal(got["values"], ref["values0"])
        assert not got["info"].any()
        for sweeps in SWEEPS:
            got = h.round_hyperplane(R, sweeps=sweeps, masks=True)
            ref = _round_reference(storage, n, q, p, T, sweeps)
            assert np.array_equal(got["masks"], ref["masks"]), sweeps
            assert np.array_equal(got["values0"], ref["values0"]) and np.array_equal(got["values"], ref["values"]), sweeps
            assert np.array_equal(got["info"], ref["info"]), (sweeps, got["info"], ref["info"])
            assert got["best"] == ref["best"] == int(np.argmin(got["values"]))
            assert np.array_equal(got["x"], round_ref.unpack(got["masks"])[got["best"]].astype(np.int8))
        again = h.round_hyperplane(R, sweeps=SWEEPS[-1], masks=True)          # two identical calls, identical bytes
        for k in ("values0", "values", "info", "x", "masks"):
            assert again[k].tobytes() == got[k].tobytes(), k
        assert np.array_equal(h.get_point(), Y0) and h.cost() == f0            # the handle is as it was
        # the best vector through the handle's own cost kernel at p = 1: 0.5 <C, x x'> doubled is x' C x, exactly
        h.set_point(got["x"].astype(np.float64)[:, None])
        assert 2.0 * h.cost() == got["values"][got["best"]]
    finally:
        h.close()


def test_round_unitdiag_accepts_the_class(lib):
    from manisdp_matlab_amd import solvers
    C, _ = lowrank_ref.instance("hub", 203, 3)
    Y, R = lowrank_ref.table_point(203, 17), round_ref.table_directions(64, 17)
    x, value, info = solvers.round_unitdiag(C, Y, sweeps=50, R=R)
    ref = _round_reference("hub", 203, 3, 17, 64, 50)
    assert np.array_equal(x, ref["x"]) and value == ref["values"][ref["best"]] and np.array_equal(info["info"], ref["info"])


# ------------------------------------------------------------------ refusals
def test_refusals_leave_no_allocation(lib):
    C, _ = lowrank_ref.instance("grid", 203, 3)
    before = lib.pool_stats()[1]
    for q in (0, 9):
        with pytest.raises(lib.MsdpError) as e:
            lib.Handle.onlyunitdiag_lowrank(C.Cs, np.ones((203, q)), np.ones(q))
        assert e.value.code == lib.EINVAL, q
        assert lib.pool_stats()[1] == before, q
    h = _lowrank_handle(lib, C)
    try:
        with pytest.raises(lib.MsdpError) as e:
            h.comm_init_local(1, 0, 4242)
        assert e.value.code == lib.EUNSUPPORTED
        h.set_point(lowrank_ref.table_point(203, 2))                        # the handle still works
        assert np.isfinite(h.cost())
    finally:
        h.close()
    assert lib.pool_stats()[1] == before
    from manisdp_matlab_amd import problems, solvers
    with pytest.raises(ValueError, match="comm"):
        solvers.ManiSDP_onlyunitdiag(C, {"comm": ("local", 1, 0, 4243)}, verbose=False)
    assert lib.pool_stats()[1] == before
