"""CPU checks of the NumPy restatement of the pose-graph problem (tests/posegraph_ref.py), of problems.pose_graph / round_poses /
pose_error, and of what solvers.ManiSDP_posegraph refuses before it loads the library.  The restatement is what
tests/test_gpu_posegraph.py holds the device to; its optima are proven by their own certificate (weak duality at a stationary
point with S PSD, lambda_min from LAPACK's eigh)."""
import numpy as np
import pytest
import scipy.sparse as sp

import posegraph_ref as B
from manisdp_matlab_amd import problems, solvers

COUNT_CASE, count_case, _counts = B.COUNT_CASE, B.count_case, B.counts


@pytest.mark.parametrize("n,d,degree", B.INSTANCES)
def test_cost_construction(n, d, degree):
    """<C, Y Y'> is the residual sum of the definition, at the planted point and at a random feasible one; C symmetric PSD."""
    for sigma in (0.0, 0.3):
        C, R, t, edges, MR, mt = B.instance(n, d, degree, sigma)
        assert C.shape == (n * (d + 1),) * 2 and abs(C - C.T).nnz == 0
        assert np.max(np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(d))) <= 1e-14 and np.all(np.linalg.det(R) > 0)
        assert np.max(np.abs(MR @ np.swapaxes(MR, 1, 2) - np.eye(d))) <= 1e-14 and np.all(np.linalg.det(MR) > 0)
        for Y in (B.planted_point(R, t), B.point(n, d, d + 2)):
            direct = B.residual_cost(Y, d, edges, MR, mt)
            quad = 2.0 * B.cost(C, Y, d)
            assert abs(quad - direct) <= 1e-10 * max(abs(direct), 1.0), (sigma, quad, direct)
            if sigma == 0.0 and Y.shape[1] == d:
                assert abs(direct) <= 1e-20 * n and abs(quad) <= 1e-10               # the noise-free planted point has cost 0
            else:
                assert direct > 1e-3
    if n <= 100:
        w = np.linalg.eigvalsh(C.toarray())
        assert w[0] >= -1e-10 * w[-1]
    # other weights: the same identity
    C2, R, t, edges, MR, mt = problems.pose_graph(n, d, degree, 0.2, 0.1, 3, kappa=2.5, omega=0.4)
    Y = B.point(n, d, d + 1)
    direct = B.residual_cost(Y, d, edges, MR, mt, kappa=2.5, omega=0.4)
    assert abs(2.0 * B.cost(C2, Y, d) - direct) <= 1e-10 * direct


def test_lambda_min_of_the_larger_cost_matrix():
    C = B.instance(343, 3, 6, 0.5)[0]
    w = np.linalg.eigvalsh(C.toarray())
    assert w[0] >= -1e-10 * w[-1]


@pytest.mark.parametrize("d", [2, 3])
def test_derivatives_against_central_differences(d):
    n, p = 23, d + 3
    C = B.instance(n, d, 6, 0.3)[0]
    Y = B.point(n, d, p)
    M = B.StiefelEuclid(n, d, p)
    g = np.random.default_rng(11)
    U, V = B.tangent_direction(Y, d, g), B.tangent_direction(Y, d, g)
    U /= np.linalg.norm(U)
    V /= np.linalg.norm(V)
    G = B.rgrad(C, Y, d)
    assert np.max(np.abs(M.proj(Y, G) - G)) <= 1e-12 * np.max(np.abs(G))          # the gradient is tangent
    assert np.array_equal(B.free(G, d), B.free(C @ Y, d))                          # its free rows are those of C Y
    f = lambda t: B.cost(C, M.retr(Y, t * U), d)
    t = 1e-4
    d1 = (f(t) - f(-t)) / (2 * t)
    assert abs(d1 - np.sum(G * U)) <= 1e-6 * max(1.0, abs(d1))
    d2 = (f(t) - 2 * f(0.0) + f(-t)) / (t * t)                                     # the retraction is second order
    H = B.hessvec(C, Y, U, d)
    assert abs(d2 - np.sum(U * H)) <= 1e-4 * max(1.0, abs(d2))
    assert np.max(np.abs(M.proj(Y, H) - H)) <= 1e-12 * np.max(np.abs(H))          # the Hess-vec is tangent
    huv, hvu = np.sum(U * B.hessvec(C, Y, V, d)), np.sum(V * H)
    assert abs(huv - hvu) <= 1e-12 * max(1.0, abs(huv))                            # and self-adjoint
    # with Lambda U left unprojected it is not tangent
    Hb = B.hessvec(C, Y, U, d, project_lambda_term=False)
    assert np.max(np.abs(M.proj(Y, Hb) - Hb)) > 1e-6
    # the Problem object: cost = <C, Y Y'> / 2 with the free rows' share, not half the dual value
    prob = B.Problem(C, n, d, p)
    assert abs(prob.cost(Y) - B.cost(C, Y, d)) <= 1e-12 * abs(B.cost(C, Y, d))
    assert abs(0.5 * B.dual_value(C, Y, d) - B.cost(C, Y, d)) > 1e-3
    assert np.array_equal(prob.grad(Y), G) and np.array_equal(prob.hess(Y, U), H)
    assert abs(np.sum(B.get_z(C, Y, d)) - B.dual_value(C, Y, d)) <= 1e-12 * abs(B.dual_value(C, Y, d))
    assert np.all(B.get_z(C, Y, d).reshape(n, d + 1)[:, d] == 0.0)
    S = B.slack(C, Y, d)
    assert abs(S - S.T).max() <= 1e-12
    assert M.typicaldist() == np.sqrt(n * (p * d - d * (d + 1) / 2) + n * p)


@pytest.mark.parametrize("d", [2, 3])
def test_retraction(d):
    n, p = 31, d + 2
    Y = B.point(n, d, p)
    M = B.StiefelEuclid(n, d, p)
    for bn in (1e-3, 1.0, 10.0):
        U = B.tangent_direction(Y, d, np.random.default_rng(5), blocknorm=bn)
        Z = M.retr(Y, U)
        Zr = B.rot(Z, d)
        assert np.max(np.abs(Zr @ np.swapaxes(Zr, 1, 2) - np.eye(d))) <= 1e-14
        assert np.array_equal(B.free(Z, d), B.free(Y + U, d))                      # tau + eta
        # the solver's re-orthonormalisation after a cut or widening is the same map: rotation rows only
        assert np.array_equal(solvers._polar_rotation_rows(Y + U, d), Z)
        A = B.rot(Y + U, d)
        w, Q = np.linalg.eigh(A @ np.swapaxes(A, 1, 2))                            # (A A')^(-1/2) A: what the device forms
        assert np.min(w) >= 1.0 - 1e-12
        P = (Q / np.sqrt(w)[:, None, :]) @ np.swapaxes(Q, 1, 2) @ A
        assert np.max(np.abs(P - Zr)) <= 1e-13


def test_count_case_is_stable_under_perturbations_of_the_start():
    """The instance and start of the device's trustregions() count test: the restatement's counts do not change when the start
    is perturbed by 1e-14 relative in five random directions (so that the device's summation order cannot change them)."""
    c = COUNT_CASE
    assert (c["n"], c["d"], c["degree"], c["sigma"], c["p"]) == (67, 3, 6, 0.3, 5)
    C, Y0 = count_case()
    _, f0, i0 = B.trustregions(C, Y0, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
    assert i0.iters >= 4 and i0.hessvecs >= 20 and i0.accepted >= 3
    g = np.random.default_rng(99)
    for _ in range(5):
        Yp = B.polar_blocks(Y0 * (1.0 + 1e-14 * g.standard_normal(Y0.shape)), c["d"])
        _, f1, i1 = B.trustregions(C, Yp, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
        assert _counts(i1) == _counts(i0) and i1.numinner == i0.numinner
        assert abs(f1 - f0) <= 1e-11 * abs(f0)


@pytest.mark.parametrize("n,d,degree", [(41, 2, 4), (67, 3, 6)])
def test_noise_free_solve_and_rounding(n, d, degree):
    C, R, t = B.instance(n, d, degree, 0.0)[:3]
    Y, obj, data = B.reference_solve(n, d, degree, 0.0)
    assert abs(obj) <= 1e-7 and data["rank"] == d
    err = problems.pose_error(*problems.round_poses(Y, d), R, t)
    assert max(err) <= 1e-6, err
    # a reflected solution, shifted inside its row space, rounds to the same poses (the majority rule; the gauge of pose_error)
    F = np.eye(Y.shape[1])
    F[0, 0] = -1.0
    Ys = B.to3(Y @ F, d).copy()
    Ys[:, d, :] += np.random.default_rng(4).standard_normal(d) @ Ys[0, :d, :]
    err = problems.pose_error(*problems.round_poses(Ys.reshape(Y.shape), d), R, t)
    assert max(err) <= 1e-6, err
    Rr, tr = problems.round_poses(Y, d)
    assert Rr.shape == (n, d, d) and tr.shape == (n, d) and np.all(np.linalg.det(Rr) > 0)


@pytest.mark.parametrize("n,d,degree,sigma", [(41, 2, 4, 0.3), (67, 3, 6, 0.3), (67, 3, 6, 1.0)])
def test_noisy_solves_carry_their_certificate(n, d, degree, sigma):
    """Stationary (gap) with S PSD (dinf, LAPACK): by weak duality obj is the optimum of the SDP."""
    C = B.instance(n, d, degree, sigma)[0]
    Y, obj, data = B.reference_solve(n, d, degree, sigma)
    assert data["status"] == 0 and max(data["dinf"], data["gap"]) < 1e-8
    dS = np.linalg.eigvalsh(B.slack(C, Y, d).toarray())
    assert max(0.0, -dS[0]) / (1.0 + dS[-1]) < 1e-8
    assert abs(np.sum(data["z"]) - obj) <= 1e-8 * (1.0 + 2.0 * abs(obj))
    assert abs(2.0 * B.cost(C, Y, d) - obj) <= 1e-12 * abs(obj)
    assert np.linalg.norm(B.rgrad(C, Y, d)) <= 1e-6
    Yr = B.rot(Y, d)
    assert np.max(np.abs(Yr @ np.swapaxes(Yr, 1, 2) - np.eye(d))) < 1e-12
    if sigma == 1.0:
        assert data["widened"] >= 1 and data["p"] > d + 2                          # the staircase fires


def test_ring_is_not_optimal_after_the_first_trustregions_call():
    """(101, 2, 2, 0.2): the first trustregions() call ends at its iteration cap with S PSD already and a gap near 1: the
    dinf test alone would stop the loop at a point that is not stationary."""
    n, d = 101, 2
    C = B.instance(n, d, 2, 0.2)[0]
    Y, obj, data = B.solve(C, d, B.start_point(n, d, d + 2, np.random.default_rng(0)), {"AL_maxiter": 2})
    it1 = data["log"][0]
    assert it1[2] < 1e-8 and it1[3] > 1e-3, it1                                    # dinf, gap after the first call
    assert data["iters"] == 2 and data["reruns"] >= 1 and data["widened"] == 0     # the loop went on, on the same factor
    assert data["log"][1][1] < it1[1]                                              # and the cost fell


def test_refusals_and_defaults_without_the_library():
    assert solvers.posegraph_defaults(3) == dict(solvers.DEFAULTS["onlyunitdiag"], p0=5, delta=3)
    assert solvers.posegraph_defaults(2)["p0"] == 4 and solvers.posegraph_defaults(2)["delta"] == 2
    C = problems.pose_graph(6, 3, 2, 0.5, 0.5, 0)[0]
    for opts in ({"line_search": 1}, {"device_factor": True}, {"round": {"trials": 64}}, {"comm": ("local", 2, 0, 1)},
                 {"eig": "host_sparse"}, {"p0": 2}):
        with pytest.raises(ValueError):
            solvers.ManiSDP_posegraph(C, 3, opts, verbose=False)
    with pytest.raises(ValueError):
        solvers.ManiSDP_posegraph(C, 4, None, verbose=False)                       # d outside {2, 3}
    with pytest.raises(ValueError):
        solvers.ManiSDP_posegraph(C[:18, :18], 3, None, verbose=False)             # N % (d + 1) != 0
    assert sp.issparse(C)
