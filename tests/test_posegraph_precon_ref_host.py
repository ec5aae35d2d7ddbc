"""CPU checks of the NumPy restatement of the block-Jacobi preconditioned tCG of the pose-graph kind
(tests/posegraph_precon_ref.py), which tests/test_gpu_posegraph_precon.py holds the device to: the preconditioner is symmetric
and positive on tangent vectors, the preconditioned tCG collapses to the oracle's with the identity, the count cases keep their
counts under perturbations of the start, and whole solves reach the optima posegraph_ref.reference_solve certifies with fewer
Hess-vecs.  These tests need no device and do not prove the device feature."""
import numpy as np
import pytest

import posegraph_precon_ref as P
import posegraph_ref as B
from manisdp_matlab_amd import problems, solvers


@pytest.mark.parametrize("n,d,degree", B.INSTANCES)
def test_preconditioner_is_symmetric_and_positive_on_tangent_vectors(n, d, degree):
    C = B.instance(n, d, degree, 0.3)[0]
    Minv = P.minv_blocks(C, d)
    M = P.diag_blocks(C, d)
    assert np.array_equal(M, np.swapaxes(M, 1, 2))
    assert np.max(np.abs(Minv @ M - np.eye(d + 1))) <= 1e-12                       # the inverse of the diagonal blocks
    w = np.linalg.eigvalsh(M)
    assert w.min() > 0.0
    print("n %d d %d: eig(M_i) in [%.3g, %.3g]" % (n, d, w.min(), w.max()))
    for p in (d, d + 2, 9):
        Y = B.point(n, d, p)
        man = B.StiefelEuclid(n, d, p)
        g = np.random.default_rng(40 + p)
        for _ in range(3):
            u, v = B.tangent_direction(Y, d, g), B.tangent_direction(Y, d, g)
            pu, pv = P.precon(Y, u, Minv, d), P.precon(Y, v, Minv, d)
            assert np.max(np.abs(man.proj(Y, pu) - pu)) <= 1e-13 * np.max(np.abs(pu))      # tangent
            a, b = float(np.sum(u * pv)), float(np.sum(pu * v))
            assert abs(a - b) <= 1e-13 * np.linalg.norm(u) * np.linalg.norm(pv), (a, b)    # <u, precon v> = <precon u, v>
            assert float(np.sum(u * pu)) > 0.0 and float(np.sum(v * pv)) > 0.0             # positive
        # an ambient argument: the result is tangent, and only the tangent part of the argument counts in <u, precon r>
        R = g.standard_normal(Y.shape)
        Z = P.precon(Y, R, Minv, d)
        assert np.max(np.abs(man.proj(Y, Z) - Z)) <= 1e-13 * np.max(np.abs(Z))


def test_a_block_without_a_factor_is_named():
    n, d = 11, 2
    C = B.instance(n, d, 4, 0.3)[0].tolil()
    C[3 * (d + 1) + d, :] = 0.0                                                    # the free row and column of block 3
    C[:, 3 * (d + 1) + d] = 0.0
    with pytest.raises(ValueError, match="block 3 "):
        P.minv_blocks(C.tocsr(), d)


def test_identity_blocks_give_the_unpreconditioned_solver():
    """The preconditioned tCG with Manopt's identity preconditioner (getPrecon.m:65, z = r) is the oracle's tCG bit for bit.
    With every M_i = I the preconditioner is the tangent projection: counts, inner iterations and stop reasons equal those of
    posegraph_ref.trustregions exactly; the iterates are bit-equal only as long as projecting the (tangent) residual changes no
    bit, which it does from the first iteration on: measured on COUNT_CASE, |Y - Y_plain| is 1e-15 after one TR iteration and
    8.6e-11 after fifteen (cost 5.8e-12 relative) -- what posegraph_ref.trustregions itself gives when its start moves by
    1e-16 relative (up to 9.6e-11 and 6.5e-12).  So beyond the first iteration the cost is held to the 1e-11 of the count rule."""
    from oracle import manopt_rtr
    c = B.COUNT_CASE
    C, Y0 = B.count_case()
    n, d = c["n"], c["d"]
    Ya, fa, ia = B.trustregions(C, Y0, d, c["maxiter"], c["maxinner"], c["tolgradnorm"])

    class Plain(P.Problem):
        def precon(self, Y, R):
            return R

    plain_tcg = manopt_rtr.tCG
    manopt_rtr.tCG = P.tCG
    try:
        Yc, fc, ic = manopt_rtr.trustregions(Plain(C, n, d, c["p"], None), np.array(Y0), c["maxiter"], c["maxinner"], c["tolgradnorm"])
    finally:
        manopt_rtr.tCG = plain_tcg
    assert np.array_equal(Yc, Ya) and fc == fa and B.counts(ic) == B.counts(ia) and ic.numinner == ia.numinner

    I = P.identity_blocks(n, d)
    Yb, fb, ib = P.trustregions(C, Y0, d, c["maxiter"], c["maxinner"], c["tolgradnorm"], I)
    assert B.counts(ib) == B.counts(ia) and ib.numinner == ia.numinner and ib.stop_inner == ia.stop_inner
    print("identity blocks: max |Y - Y_plain| %.2e, cost %.2e relative" % (np.max(np.abs(Ya - Yb)), abs(fa - fb) / abs(fa)))
    assert abs(fa - fb) <= 1e-11 * abs(fa)
    Y1a = B.trustregions(C, Y0, d, 1, c["maxinner"], c["tolgradnorm"])[0]
    Y1b = P.trustregions(C, Y0, d, 1, c["maxinner"], c["tolgradnorm"], I)[0]
    assert np.max(np.abs(Y1a - Y1b)) <= 1e-14


@pytest.mark.parametrize("name", sorted(P.COUNT_CASES))
def test_count_cases_are_stable_under_perturbations_of_the_start(name):
    """The rule of test_posegraph_ref_host.py for COUNT_CASE, with twenty perturbations: the counts, the inner iterations of
    every call and the cost (1e-11 relative) do not move when the start is perturbed by 1e-14 relative."""
    c = P.COUNT_CASES[name]
    C, Y0 = P.count_case(name)
    Minv = P.minv_blocks(C, c["d"])
    _, f0, i0 = P.count_reference(name)
    print("case %s: %s, tCG stops seen %s" % (name, P.counts(i0), sorted(set(i0.stop_inner))))
    assert i0.iters >= 4 and i0.hessvecs >= 20 and i0.accepted >= 3
    g = np.random.default_rng(99)
    for _ in range(20):
        Yp = B.polar_blocks(Y0 * (1.0 + 1e-14 * g.standard_normal(Y0.shape)), c["d"])
        _, f1, i1 = P.trustregions(C, Yp, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"], Minv)
        assert P.counts(i1) == P.counts(i0) and i1.numinner == i0.numinner
        assert abs(f1 - f0) <= 1e-11 * abs(f0)


def test_count_cases_cover_the_stop_reasons():
    seen = {name: set(P.count_reference(name)[2].stop_inner) for name in P.COUNT_CASES}
    assert seen["A"] == {2} and seen["B"] == {2, 3} and seen["D"] == {1, 2, 3} and seen["C"] == {1, 2, 3, 5}
    assert P.counts(P.count_reference("A")[2]) != B.counts(B.trustregions(*B.count_case(), 3, 15, 30, 1e-5)[2])   # not the plain counts


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("shape", B.INSTANCES)
def test_one_step_margins_leave_at_most_two_widths_per_shape(shape, wide):
    """The device's one-step test skips a width whose stop tests come within 1e-10 relative of equality, at the default radius
    and at the 1000 times wider one it also runs: the restatement alone shows how many widths that is."""
    n, d, degree = shape
    C = B.instance(n, d, degree, 0.3)[0]
    Minv = P.minv_blocks(C, d)
    close = []
    for p in sorted({d, d + 1} | {q for q in (4, 7, 12, 24, 33, 64, 100, 130, 256) if q >= d}):
        Y = B.point(n, d, p)
        prob = P.Problem(C, n, d, p, Minv)
        prob.cost(Y)
        Delta = prob.M.typicaldist() * (1e3 if wide else 0.125)
        if P.stop_margin(prob, Y, prob.grad(Y), Delta, 8) < 1e-10:
            close.append(p)
    assert len(close) <= 2, close


@pytest.mark.parametrize("n,d,degree", [(41, 2, 4), (67, 3, 6)])
def test_preconditioned_solves_reach_the_certified_optima_with_fewer_hessvecs(n, d, degree):
    _, obj_r, data_r = B.reference_solve(n, d, degree, 0.3)
    assert data_r["status"] == 0 and max(data_r["dinf"], data_r["gap"]) < 1e-8
    _, obj, data = P.reference_solve(n, d, degree, 0.3)
    print("n %d d %d: %.10f (plain %.10f), Hess-vecs %d (plain %d)" % (n, d, obj, obj_r, data["hessvecs"], data_r["hessvecs"]))
    assert data["status"] == 0 and max(data["dinf"], data["gap"]) < 1e-8
    assert abs(obj - obj_r) <= 1e-8 * abs(obj_r)
    assert data["hessvecs"] < data_r["hessvecs"]


def test_the_solvers_check_the_option_before_the_library_is_loaded():
    C = problems.pose_graph(6, 3, 2, 0.5, 0.5, 0)[0]
    for value in ("jacobi", True, 1, "ichol"):
        with pytest.raises(ValueError, match="precon"):
            solvers.ManiSDP_posegraph(C, 3, {"precon": value}, verbose=False)
    Cr = problems.rotation_synchronization(6, 3, 2, 0.5, 0)[0]
    with pytest.raises(ValueError, match="precon"):
        solvers.ManiSDP_onlyunitblockdiag(Cr, 3, {"precon": "blockjacobi"}, verbose=False)
