"""The block-Jacobi preconditioned tCG of the pose-graph handle (msdp_set_option "precon", msdp_precon_apply,
msdp_pose_precon.hip) against the NumPy restatement of tests/posegraph_precon_ref.py: the preconditioner over every dispatched
<LPR, NCH> instance for d = 2 and 3, one tCG per instance, trustregions() counts on the count cases (chunk graphs and plain
launches), the option's plumbing (graph re-capture, block_persist), the refused handles, and whole solves through
solvers.ManiSDP_posegraph.  The reference of the error rule of the one-step test is the generic path of the same handle."""
import numpy as np
import pytest
import scipy.sparse as sp

import posegraph_precon_ref as P
import posegraph_ref as B

pytestmark = pytest.mark.gpu

SHAPES = B.INSTANCES                                       # (41, 2, 4), (67, 3, 6), (343, 3, 6), noise 0.3
# one width per dispatched <LPR, NCH> instance (ld = 2 .. 256), odd widths for the padding column; d and d + 1 are added per shape
WIDTHS = (4, 7, 12, 24, 33, 64, 100, 130, 256)


@pytest.fixture(scope="module")
def lib():
    from manisdp_matlab_amd import _lib
    _lib.load()
    return _lib


def _relerr(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _widths(d):
    return sorted({d, d + 1} | {p for p in WIDTHS if p >= d})


def _tuple(st):
    return (st.iters, st.hessvecs, st.accepted, st.rejected, st.last_stop_inner)


# ------------------------------------------------------------------ the preconditioner
@pytest.mark.parametrize("shape", SHAPES)
def test_precon_apply_against_restatement(lib, shape):
    n, d, degree = shape
    C = B.instance(n, d, degree, 0.3)[0]
    Minv = P.minv_blocks(C, d)
    h = lib.Handle.posegraph(C, d, pcap=256)
    try:
        h.set_option("precon", 1)
        for p in _widths(d):
            Y = B.point(n, d, p)
            M = B.StiefelEuclid(n, d, p)
            g = np.random.default_rng(900 + p)
            h.set_point(Y)
            errs = {}
            for name, R in (("ambient", g.standard_normal(Y.shape)), ("tangent", B.tangent_direction(Y, d, g))):
                Z = h.precon_apply(R)
                errs[name] = _relerr(Z, P.precon(Y, R, Minv, d))
                errs[name + "_tan"] = _relerr(M.proj(Y, Z), Z)
                assert np.array_equal(Z, h.precon_apply(R))                  # fixed summation orders
            print("n %d d %d p %d: " % (n, d, p) + " ".join("%s %.1e" % kv for kv in errs.items()))
            assert all(v < 1e-12 for v in errs.values()), (p, errs)
            assert np.array_equal(h.get_point(), Y)
    finally:
        h.close()


# ------------------------------------------------------------------ one tCG per instance
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_tcg_per_instance(lib, shape, wide):
    """trustregions() with maxiter = 1, maxinner = 8 at every width: Hess-vecs and stop reason of the restatement, and a point whose
    error against the restatement is within 10 x the error of the option-off call on the same handle against
    posegraph_ref.trustregions.  With the default radius the tCG of these starts leaves through the boundary on its first trip;
    wide = True repeats the test with Delta_bar = Delta0 = 1000 typicaldist, where it runs two or three trips (z, beta, the new
    direction) before it meets negative curvature.  That step is rejected and the point stays, so there the step eta the tCG
    left (msdp_debug_get_tcg_step) is what is compared: to the kind's operator tolerance 1e-12, since eta is a combination of
    at most eight directions, each a few applications of operators that are held to 1e-12 (the plain path runs fewer trips from
    these starts, so its error is no yardstick for eta)."""
    n, d, degree = shape
    C = B.instance(n, d, degree, 0.3)[0]
    Minv = P.minv_blocks(C, d)
    skipped, stops = [], set()
    h = lib.Handle.posegraph(C, d, pcap=256)
    try:
        for p in _widths(d):
            Y = B.point(n, d, p)
            typical = B.StiefelEuclid(n, d, p).typicaldist()
            radii = dict(Delta_bar=1e3 * typical, Delta0=1e3 * typical) if wide else {}
            opts = lib.default_opts(maxiter=1, maxinner=8, tolgradnorm=1e-8, **radii)
            Yr_off, _, i_off = P.plain_trustregions(C, Y, d, 1, 8, 1e-8, **radii)
            Yr_on, _, i_on = P.trustregions(C, Y, d, 1, 8, 1e-8, Minv, **radii)
            h.set_option("precon", 0)
            h.set_point(Y)
            st_off = h.rtr(opts)
            e_off = _relerr(h.get_point(), Yr_off)
            Delta = radii.get("Delta0", typical / 8.0)
            s_off = _relerr(h.debug_get_tcg_step()[0], P.tcg_step(C, Y, d, Delta, 8)[0])
            h.set_option("precon", 1)
            h.set_point(Y)
            assert h.tcg_path() == 0
            st_on = h.rtr(opts)
            Yd = h.get_point()
            e_on = _relerr(Yd, Yr_on)
            s_on = _relerr(h.debug_get_tcg_step()[0], P.tcg_step(C, Y, d, Delta, 8, Minv)[0])
            prob = P.Problem(C, n, d, p, Minv)
            prob.cost(Y)
            margin = P.stop_margin(prob, Y, prob.grad(Y), Delta, 8)
            print("n %d d %d p %d: on (%d Hess-vecs, stop %d; restatement %d, %d) point %.2e eta %.2e; off (%d, %d; %d, %d) point %.2e eta %.2e; margin %.1e"
                  % (n, d, p, st_on.hessvecs, st_on.last_stop_inner, i_on.hessvecs, i_on.stop_inner[-1], e_on, s_on,
                     st_off.hessvecs, st_off.last_stop_inner, i_off.hessvecs, i_off.stop_inner[-1], e_off, s_off, margin))
            Y3 = B.rot(Yd, d)
            assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(d))) < 1e-13
            if margin < 1e-10:                                               # a stop test within rounding of equality: no counts
                skipped.append(p)
                continue
            assert (st_on.hessvecs, st_on.last_stop_inner) == (i_on.hessvecs, i_on.stop_inner[-1]), p
            assert (st_off.hessvecs, st_off.last_stop_inner) == (i_off.hessvecs, i_off.stop_inner[-1]), p
            assert e_on <= 10.0 * e_off, (p, e_on, e_off)
            assert s_on < 1e-12 and s_off < 1e-12, (p, s_on, s_off)
            stops.add((st_on.last_stop_inner, st_on.hessvecs > 1))
        assert len(skipped) <= 2, skipped
        assert stops <= ({(1, True)} if wide else {(2, False)}), stops          # (what the two radii are there for)
    finally:
        h.close()


# ------------------------------------------------------------------ trustregions() counts
@pytest.mark.parametrize("graph", [1, 0])
@pytest.mark.parametrize("name", sorted(P.COUNT_CASES))
def test_rtr_counts_match_the_restatement(lib, name, graph):
    c = P.COUNT_CASES[name]
    C, Y0 = P.count_case(name)
    _, f_ref, info = P.count_reference(name)
    h = lib.Handle.posegraph(C, c["d"], pcap=c["p"])
    try:
        h.set_option("precon", 1)
        h.set_option("graph", graph)
        h.set_point(Y0)
        assert h.tcg_path() == 0
        st = h.rtr(lib.default_opts(maxiter=c["maxiter"], maxinner=c["maxinner"], tolgradnorm=c["tolgradnorm"]))
        print("case %s graph %d: device" % (name, graph), _tuple(st), st.cost, "restatement", P.counts(info), f_ref)
        assert _tuple(st) == P.counts(info)
        assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
        Y3 = B.rot(h.get_point(), c["d"])
        assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(c["d"]))) < 1e-13
    finally:
        h.close()


# ------------------------------------------------------------------ option plumbing
def test_option_off_again_gives_the_plain_counts(lib):
    """On, off, on on one handle: the chunk graph is captured again each time (its signature holds what selects the launchers)."""
    c = B.COUNT_CASE
    C, Y0 = B.count_case()
    _, f_plain, i_plain = B.trustregions(C, Y0, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
    a = P.COUNT_CASES["A"]
    assert {k: a[k] for k in c} == c                                         # case A is COUNT_CASE's instance, start and budget
    _, f_on, i_on = P.count_reference("A")
    assert P.counts(i_on) != B.counts(i_plain)
    opts = lib.default_opts(maxiter=c["maxiter"], maxinner=c["maxinner"], tolgradnorm=c["tolgradnorm"])
    h = lib.Handle.posegraph(C, c["d"], pcap=c["p"])
    try:
        for on in (0, 1, 0, 1):
            h.set_option("precon", on)
            h.set_point(Y0)
            st = h.rtr(opts)
            want, f_want = (P.counts(i_on), f_on) if on else (B.counts(i_plain), f_plain)
            print("precon %d:" % on, _tuple(st), st.cost, "restatement", want, f_want)
            assert _tuple(st) == want
            assert abs(st.cost - f_want) <= 1e-11 * abs(f_want)
        with pytest.raises(lib.MsdpError):
            h.set_option("precon", 2)
        # a wider point than the handle was created for: the vectors are allocated again, the preconditioner's with them
        p = 12
        Y = B.point(c["n"], c["d"], p)
        h.set_point(Y)
        Z = h.precon_apply(Y)
        assert _relerr(Z, P.precon(Y, Y, P.minv_blocks(C, c["d"]), c["d"])) < 1e-12
        st = h.rtr(lib.default_opts(maxiter=1, maxinner=8, tolgradnorm=1e-8))
        i1 = P.trustregions(C, Y, c["d"], 1, 8, 1e-8)[2]
        assert (st.hessvecs, st.last_stop_inner) == (i1.hessvecs, i1.stop_inner[-1])
    finally:
        h.close()


def test_precon_without_the_option_is_refused(lib):
    n, d = 41, 2
    h = lib.Handle.posegraph(B.instance(n, d, 4, 0.3)[0], d)
    try:
        Y = B.point(n, d, 4)
        h.set_point(Y)
        with pytest.raises(lib.MsdpError, match="precon") as e:
            h.precon_apply(Y)
        assert e.value.code == lib.ESTATE
    finally:
        h.close()


def test_precon_takes_the_generic_path_under_block_persist(lib):
    c = P.COUNT_CASES["A"]
    C, Y0 = P.count_case("A")
    _, f_ref, info = P.count_reference("A")
    h = lib.Handle.posegraph(C, c["d"], pcap=c["p"])
    try:
        h.set_option("block_persist", 1)
        h.set_option("precon", 1)
        h.set_point(Y0)
        assert h.tcg_path() == 0 and h.persist_form() == -1
        st = h.rtr(lib.default_opts(maxiter=c["maxiter"], maxinner=c["maxinner"], tolgradnorm=c["tolgradnorm"]))
        print("block_persist + precon:", _tuple(st), st.cost, "restatement", P.counts(info), f_ref)
        assert _tuple(st) == P.counts(info)
        assert abs(st.cost - f_ref) <= 1e-11 * abs(f_ref)
        assert h.bench_tcg_trip(16) > 0                                      # the measurement entry point times the same trips
    finally:
        h.close()


# ------------------------------------------------------------------ refusals
def test_refused_handles_name_the_kind_or_the_block(lib):
    from manisdp_matlab_amd import problems
    n, d, degree = 67, 3, 6
    C = sp.csr_matrix(B.instance(n, d, degree, 0.3)[0])
    keep = np.ones(n * (d + 1), dtype=bool)
    keep[d::d + 1] = False
    Dk = sp.diags(keep.astype(np.float64))
    Cz = sp.csr_matrix(Dk @ C @ Dk)                                          # zero free rows and columns: singular diagonal blocks
    Cz.eliminate_zeros()
    Cr = sp.csr_matrix(C[keep][:, keep])                                     # the rotation submatrix of order n d
    Cm = problems.toroidal_grid_maxcut(6, 8, seed=1)
    Y = B.point(n, d, d + 2)
    g = np.random.default_rng(5)
    Ym = g.standard_normal((Cm.shape[0], 4))
    Ym /= np.linalg.norm(Ym, axis=1, keepdims=True)
    opts = lib.default_opts(maxiter=3, maxinner=10, tolgradnorm=1e-8)
    cases = ((lib.Handle.posegraph(Cz, d), Y, "block 0 "),
             (lib.Handle.onlyunitblockdiag(Cr, d), np.ascontiguousarray(Y[keep]), "unit-block-diagonal"),
             (lib.Handle.onlyunitdiag(Cm), Ym, "onlyunitdiag"))
    try:
        for h, Y0, word in cases:
            h.set_point(Y0)
            f, G = h.cost(), h.rgrad()
            st0 = h.rtr(opts)
            Y1 = h.get_point()
            with pytest.raises(lib.MsdpError, match=word) as e:
                h.set_option("precon", 1)
            print(word, "->", e.value)
            assert e.value.code == lib.EUNSUPPORTED
            h.set_point(Y0)
            assert h.cost() == f and np.array_equal(h.rgrad(), G)
            st1 = h.rtr(opts)
            assert _tuple(st1) == _tuple(st0) and st1.cost == st0.cost and np.array_equal(h.get_point(), Y1)
    finally:
        for h, _, _ in cases:
            h.close()


# ------------------------------------------------------------------ solves
@pytest.mark.parametrize("n,d,degree", SHAPES)
def test_preconditioned_solves(lib, n, d, degree):
    from manisdp_matlab_amd import solvers
    C = B.instance(n, d, degree, 0.3)[0]
    _, obj_r, data_r = B.reference_solve(n, d, degree, 0.3)
    assert data_r["status"] == 0 and max(data_r["dinf"], data_r["gap"]) < 1e-8
    Y, obj, data = solvers.ManiSDP_posegraph(C, d, {"precon": "blockjacobi"}, verbose=False)
    _, obj_off, data_off = solvers.ManiSDP_posegraph(C, d, verbose=False)
    print("n %d d %d: %.10f, restatement %.10f; Hess-vecs %d with the preconditioner, %d without; dinf %.1e, gap %.1e, p %d"
          % (n, d, obj, obj_r, data["hessvecs"], data_off["hessvecs"], data["dinf"], data["gap"], data["p"]))
    assert data["status"] == 0 and data["dinf"] < 1e-8 and data["gap"] < 1e-8
    assert abs(obj - obj_r) <= 1e-6 * abs(obj_r)
    Y3 = B.rot(Y, d)
    assert np.max(np.abs(Y3 @ np.swapaxes(Y3, 1, 2) - np.eye(d))) < 1e-12
    if (n, d, degree) != SHAPES[0]:
        assert data["hessvecs"] < data_off["hessvecs"]
