"""CPU checks of the NumPy restatement of the unit-block-diagonal problem (tests/blockdiag_ref.py), of
problems.rotation_synchronization / round_rotations / rotation_error, and of what solvers.ManiSDP_onlyunitblockdiag refuses
before it loads the library.  The restatement is what tests/test_gpu_blockdiag.py holds the device to."""
import numpy as np
import pytest
import scipy.sparse as sp

import blockdiag_ref as B
from manisdp_matlab_amd import problems, solvers
from oracle import manisdp_ref as R
from oracle import manopt_rtr

COUNT_CASE, count_case, _counts = B.COUNT_CASE, B.count_case, B.counts


def test_d1_equals_the_oblique_oracle():
    g = np.random.default_rng(3)
    n, p = 60, 4
    A = sp.random(n, n, density=0.1, random_state=5, format="csr")
    C = sp.csr_matrix(A + A.T)
    Y = g.standard_normal((n, p))
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    U = g.standard_normal((n, p))
    U -= Y * np.sum(Y * U, axis=1, keepdims=True)
    prob = R._OnlyUnitDiagProblem(C, n, p, q1="correct")
    f = prob.cost(Y)
    scale = max(1.0, abs(f))
    assert abs(B.cost(C, Y, 1) - f) <= 1e-14 * scale
    G = prob.grad(Y)
    assert np.max(np.abs(B.rgrad(C, Y, 1) - G)) <= 1e-14 * max(1.0, np.max(np.abs(G)))
    H = prob.hess(Y, U)
    assert np.max(np.abs(B.hessvec(C, Y, U, 1) - H)) <= 1e-14 * max(1.0, np.max(np.abs(H)))
    _, f1, i1 = manopt_rtr.trustregions(R._OnlyUnitDiagProblem(C, n, p, q1="correct"), Y.copy(), 20, 40, 1e-8,
                                        Delta_bar=np.pi * np.sqrt(n))
    prob_b = B.Problem(C, n, 1, p)
    _, f2, i2 = manopt_rtr.trustregions(prob_b, Y.copy(), 20, 40, 1e-8, Delta_bar=np.pi * np.sqrt(n))
    assert _counts(i1) == _counts(i2) and i1.numinner == i2.numinner
    assert abs(f1 - f2) <= 1e-12 * max(1.0, abs(f1))


@pytest.mark.parametrize("d", [2, 3])
def test_derivatives_against_central_differences(d):
    n, p = 23, d + 3
    C, _, _ = B.instance(n, d, 6, 1.0, diag=True)
    Y = B.point(n, d, p)
    M = B.StiefelStacked(n, d, p)
    g = np.random.default_rng(11)
    U, V = B.tangent_direction(Y, d, g), B.tangent_direction(Y, d, g)
    U /= np.linalg.norm(U)
    V /= np.linalg.norm(V)
    G = B.rgrad(C, Y, d)
    assert np.max(np.abs(M.proj(Y, G) - G)) <= 1e-12 * np.max(np.abs(G))          # the gradient is tangent
    f = lambda t: B.cost(C, M.retr(Y, t * U), d)
    t = 1e-4
    d1 = (f(t) - f(-t)) / (2 * t)
    assert abs(d1 - np.sum(G * U)) <= 1e-6 * max(1.0, abs(d1))
    d2 = (f(t) - 2 * f(0.0) + f(-t)) / (t * t)                                     # the polar retraction is second order
    H = B.hessvec(C, Y, U, d)
    assert abs(d2 - np.sum(U * H)) <= 1e-4 * max(1.0, abs(d2))
    assert np.max(np.abs(M.proj(Y, H) - H)) <= 1e-12 * np.max(np.abs(H))          # the Hess-vec is tangent
    # self-adjoint on the tangent space; not so when Lambda U is left unprojected
    huv, hvu = np.sum(U * B.hessvec(C, Y, V, d)), np.sum(V * H)
    assert abs(huv - hvu) <= 1e-12 * max(1.0, abs(huv))
    Hb_u, Hb_v = B.hessvec(C, Y, U, d, project_lambda_term=False), B.hessvec(C, Y, V, d, project_lambda_term=False)
    assert np.max(np.abs(M.proj(Y, Hb_u) - Hb_u)) > 1e-6                           # ... it is not even tangent
    assert np.max(np.abs(Hb_v - B.hessvec(C, Y, V, d))) > 1e-6


@pytest.mark.parametrize("d", [2, 3])
def test_retraction_is_the_polar_factor(d):
    n, p = 31, d + 2
    Y = B.point(n, d, p)
    M = B.StiefelStacked(n, d, p)
    for bn in (1e-3, 1.0, 10.0):
        U = B.tangent_direction(Y, d, np.random.default_rng(5), blocknorm=bn)
        Z = M.retr(Y, U)
        Z3 = B.to3(Z, d)
        assert np.max(np.abs(Z3 @ np.swapaxes(Z3, 1, 2) - np.eye(d))) <= 1e-14
        # (A A')^(-1/2) A through the eigen-decomposition of the Gram matrix: what the device forms
        A3 = B.to3(Y + U, d)
        w, Q = np.linalg.eigh(A3 @ np.swapaxes(A3, 1, 2))
        assert np.min(w) >= 1.0 - 1e-12                                            # I + eta eta' for tangent eta
        P = (Q / np.sqrt(w)[:, None, :]) @ np.swapaxes(Q, 1, 2) @ A3
        assert np.max(np.abs(P - Z3)) <= 1e-13


@pytest.mark.parametrize("d", [2, 3])
def test_noise_free_known_answer(d):
    n = 40
    C, Rt, edges = problems.rotation_synchronization(n, d, 6, 0.0, 0)
    assert abs(C - C.T).nnz == 0 and C.shape == (n * d, n * d)
    assert np.max(np.abs(Rt @ np.swapaxes(Rt, 1, 2) - np.eye(d))) <= 1e-14 and np.all(np.linalg.det(Rt) > 0)
    import scipy.sparse.csgraph as cg
    G = sp.coo_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(n, n))
    assert cg.connected_components(G, directed=False)[0] == 1
    Y, obj, data = B.solve(C, d, B.random_point(n, d, d + 2, np.random.default_rng(2)))
    assert data["status"] == 0 and data["rank"] == d
    assert abs(obj + 2 * len(edges) * d) <= 1e-6
    assert problems.rotation_error(problems.round_rotations(Y, d), Rt) <= 1e-6
    # a reflected solution rounds to the same rotations (the majority rule)
    F = np.eye(Y.shape[1])
    F[0, 0] = -1.0
    assert problems.rotation_error(problems.round_rotations(Y @ F, d), Rt) <= 1e-6


@pytest.mark.parametrize("n,d,sigma", [(20, 3, 1.0), (25, 2, 1.5)])
def test_noisy_instances_against_the_affine_formulation(n, d, sigma):
    C, _, _ = problems.rotation_synchronization(n, d, 6, sigma, 0)
    Y, obj, data = B.solve(C, d, B.random_point(n, d, d, np.random.default_rng(1)))
    assert data["status"] == 0 and data["dinf"] < 1e-8
    assert data["widened"] >= 1                                                    # the staircase fires from p0 = d
    assert abs(np.sum(data["z"]) - obj) <= 1e-10 * abs(obj)
    At, b, c, K = B.affine_formulation(C, d)
    _, obj_a, data_a = R.ManiSDP_unitdiag(At, b, c, K, {"tol": 1e-9})
    assert data_a["status"] == 0
    assert abs(obj - obj_a) <= 1e-6


def test_count_case_is_stable_under_perturbations_of_the_start():
    """The instance and start of the device's trustregions() count test: the restatement's counts do not change when the start
    is perturbed by 1e-14 relative in five random directions (so that the device's summation order cannot change them)."""
    c = COUNT_CASE
    C, Y0 = count_case()
    _, f0, i0 = B.trustregions(C, Y0, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
    assert i0.iters >= 4 and i0.hessvecs >= 20 and i0.accepted >= 3
    g = np.random.default_rng(99)
    for _ in range(5):
        Yp = B.polar_blocks(Y0 * (1.0 + 1e-14 * g.standard_normal(Y0.shape)), c["d"])
        _, f1, i1 = B.trustregions(C, Yp, c["d"], c["maxiter"], c["maxinner"], c["tolgradnorm"])
        assert _counts(i1) == _counts(i0) and i1.numinner == i0.numinner
        assert abs(f1 - f0) <= 1e-11 * abs(f0)


def test_refusals_and_defaults_without_the_library():
    assert solvers.onlyunitblockdiag_defaults(3) == dict(solvers.DEFAULTS["onlyunitdiag"], p0=5, delta=3)
    assert solvers.onlyunitblockdiag_defaults(2)["p0"] == 4 and solvers.onlyunitblockdiag_defaults(2)["delta"] == 2
    C, _, _ = problems.rotation_synchronization(6, 3, 2, 0.5, 0)
    for opts in ({"line_search": 1}, {"device_factor": True}, {"round": {"trials": 64}}, {"comm": ("local", 2, 0, 1)},
                 {"eig": "host_sparse"}, {"p0": 2}):
        with pytest.raises(ValueError):
            solvers.ManiSDP_onlyunitblockdiag(C, 3, opts, verbose=False)
    with pytest.raises(ValueError):
        solvers.ManiSDP_onlyunitblockdiag(C, 4, None, verbose=False)               # d outside {2, 3}
    with pytest.raises(ValueError):
        solvers.ManiSDP_onlyunitblockdiag(C[:16, :16], 3, None, verbose=False)     # N % d != 0
