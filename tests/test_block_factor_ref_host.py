"""CPU tests of tests/block_factor_ref.py, the restatement the device's block-factor calls (msdp_blockfactor.hip) are held to:
its two-pass polar factor against LAPACK's SVD over well- and ill-conditioned blocks, its rounding against
problems.round_rotations / round_poses, and the options of the two solvers that select the device path."""
import numpy as np
import pytest

import block_factor_ref as F
import blockdiag_ref as BD
import posegraph_ref as BP
from manisdp_matlab_amd import problems, solvers

NBLK = 20000


def _ill_conditioned(A, g):
    """A quarter of the blocks squeezed towards rank d - 1: row 1 <- a combination of the other rows plus 10^-s of itself,
    s uniform in [0, 5.8] (cond(A A') up to about 4e11, below the degenerate ratio)."""
    A = np.array(A)
    k = A.shape[0] // 4
    s = 10.0 ** (-g.uniform(0.0, 5.8, size=k))
    A[:k, 1, :] = A[:k, 0, :] * g.standard_normal((k, 1)) + s[:, None] * A[:k, 1, :]
    return A


@pytest.mark.parametrize("d", [2, 3])
def test_two_pass_polar_factor_against_the_svd(d):
    """Measured on this restatement: orthonormality <= 3.6e-15 at every width, also at cond(G) = 1e12, and
    |P - P_svd|_max <= 11.9 eps cond(G_i) block by block; asserted: 1e-12 and 64 eps cond (the margin is for the kernel's
    Jacobi sweeps against LAPACK and the order of its group sums: the device's largest ratio is 22.8)."""
    worst_o = worst_r = 0.0
    for p in (d, d + 1, 5, 8, 33, 256):
        g = np.random.default_rng(1000 * d + p)
        A = _ill_conditioned(g.standard_normal((NBLK, d, p)), g)
        keep = ~F.degenerate(F.block_gram(A))              # (beyond the degenerate ratio: not the contract; a few per cent at p = d)
        assert np.sum(keep) >= 0.95 * NBLK
        A = A[keep]
        G = F.block_gram(A)
        kappa = F.cond(G)
        P, Ps = F.polar_two_pass(A), F.polar_svd(A)
        orth = np.max(np.abs(F.block_gram(P) - np.eye(d)))
        ratio = np.max(np.max(np.abs(P - Ps), axis=(1, 2)) / (F.EPS * kappa))
        print("d %d p %3d: max cond %.1e, orthonormality %.2e, max |P - P_svd| / (eps cond) %.2f" % (d, p, kappa.max(), orth, ratio))
        worst_o, worst_r = max(worst_o, orth), max(worst_r, ratio)
        assert orth <= 1e-12
        assert ratio <= 64.0
    assert worst_o <= 1e-12 and worst_r <= 64.0


def test_one_pass_is_not_enough():
    """Why the kernel applies G^(-1/2) twice: one pass leaves |A A' - I| of the order eps cond(G)."""
    g = np.random.default_rng(5)
    A = _ill_conditioned(g.standard_normal((2000, 3, 8)), g)
    one = F._invsqrt(F.block_gram(A)) @ A
    assert np.max(np.abs(F.block_gram(one) - np.eye(3))) > 1e-9
    assert np.max(np.abs(F.block_gram(F.polar_two_pass(A)) - np.eye(3))) <= 1e-12


def test_degenerate_rule():
    G = np.array([np.eye(3), np.diag([1.0, 1e-13, 1.0]), np.zeros((3, 3)), np.diag([1.0, 2e-12, 1.0]),
                  np.outer([1.0, 2.0, 3.0], [1.0, 2.0, 3.0])])
    assert list(F.degenerate(G)) == [False, True, True, False, True]


@pytest.mark.parametrize("d,efree", [(2, 0), (3, 0), (2, 1), (3, 1)])
def test_rotate_and_append_touch_the_rotation_rows_only(d, efree):
    n, p = 37, 7
    g = np.random.default_rng(3)
    Y = (BP if efree else BD).random_point(n, d, p, g)
    Q = np.linalg.qr(g.standard_normal((p, p)))[0][:, :d + 1]
    V = g.standard_normal((Y.shape[0], 2))
    for Z, plain in ((F.rotate(Y, d, efree, Q), Y @ Q), (F.append(Y, d, efree, V, 0.5), np.hstack([Y, 0.5 * V]))):
        Z3, P3 = F.blocks(Z, d, efree), F.blocks(plain, d, efree)
        assert np.max(np.abs(F.block_gram(Z3[:, :d]) - np.eye(d))) <= 1e-14
        assert np.allclose(Z3[:, :d], F.polar_svd(P3[:, :d]), rtol=0, atol=1e-13)
        if efree:
            assert np.array_equal(Z3[:, d], P3[:, d])


@pytest.mark.parametrize("d", [2, 3])
def test_round_blocks_equals_the_host_rounding_of_rotations(d):
    n = 101
    C, Rt, _ = problems.rotation_synchronization(n, d, 6, 0.0, 0)
    g = np.random.default_rng(8)
    Qg = np.linalg.qr(g.standard_normal((d + 2, d + 2)))[0][:, :d]
    for reflect in (False, True):                          # the planted point in a frame of either orientation: all-majority inputs
        Y = Rt.reshape(n * d, d) @ Qg.T
        if reflect:
            Y = Y @ np.diag([1.0] * (d + 1) + [-1.0])
        W = F.top_eigenvectors(Y, d)
        R, t, flipped, ndeg = F.round_blocks(Y, d, 0, W)
        assert t is None and ndeg == 0
        assert np.allclose(np.linalg.det(R), 1.0, rtol=0, atol=1e-13)
        Rh = problems.round_rotations(Y, d)
        # the host takes its own basis of the top-d subspace: the two roundings agree up to one rotation of the frame
        assert problems.rotation_error(R, Rh) <= 1e-12
        assert problems.rotation_error(R, Rt) <= 1e-12
        # ... and entry by entry when both are given the same W
        Z = (Y @ W).reshape(n, d, d)
        Rw = F.polar_svd(Z)
        if flipped:
            Rw[:, :, -1] *= -1.0
        assert np.max(np.abs(R - problems._to_so(Rw))) <= 1e-13


@pytest.mark.parametrize("d", [2, 3])
def test_round_blocks_equals_the_host_rounding_of_poses(d):
    n = 67
    C, Rt, tt = problems.pose_graph(n, d, 6, 0.0, 0.0, 0)[:3]
    Y = BP.planted_point(Rt, tt)
    g = np.random.default_rng(9)
    Y = np.hstack([Y, np.zeros((Y.shape[0], 2))]) @ np.linalg.qr(g.standard_normal((d + 2, d + 2)))[0]
    W = F.top_eigenvectors(Y, d)
    R, t, flipped, ndeg = F.round_blocks(Y, d, 1, W)
    assert ndeg == 0 and np.allclose(np.linalg.det(R), 1.0, rtol=0, atol=1e-13)
    Rh, th = problems.round_poses(Y, d)
    assert max(problems.pose_error(R, t, Rh, th)) <= 1e-11
    assert max(problems.pose_error(R, t, Rt, tt)) <= 1e-11


def test_minority_block_goes_to_its_nearest_rotation():
    d, n, p = 3, 41, 8
    W = F.top_eigenvectors(BD.point(n, d, p), d)
    Y = F.oriented(BD.point(n, d, p), d, 0, W)             # every det(Y_i W) positive
    R0, _, flipped0, _ = F.round_blocks(Y, d, 0, W)
    assert flipped0 == 0 and np.all(np.linalg.det((Y @ W).reshape(n, d, d)) > 0)
    Y[[0, 1]] = Y[[1, 0]]                                  # block 0 reflected: the one determinant of n that is negative
    R1, _, flipped1, ndeg = F.round_blocks(Y, d, 0, W)
    assert flipped1 == 0 and ndeg == 0
    assert np.array_equal(R1[1:], R0[1:])
    assert abs(np.linalg.det(R1[0]) - 1.0) <= 1e-13
    Z = (Y @ W).reshape(n, d, d)
    assert np.linalg.det(Z[0]) < 0
    assert np.max(np.abs(R1[0] - F.nearest_rotation_svd(Z[:1])[0])) <= 64 * F.EPS * F.cond(F.block_gram(Z[:1]))[0]


def test_block_factor_option_and_defaults():
    assert solvers._block_factor_option({}, "x") == "host"
    assert solvers._block_factor_option({"block_factor": "device"}, "x") == "device"
    for d in (2, 3):
        assert "block_factor" not in solvers.onlyunitblockdiag_defaults(d) and "round_blocks" not in solvers.onlyunitblockdiag_defaults(d)
        assert "block_factor" not in solvers.posegraph_defaults(d) and "round_blocks" not in solvers.posegraph_defaults(d)
    C, _, _ = problems.rotation_synchronization(6, 3, 2, 0.5, 0)
    Cp = problems.pose_graph(6, 3, 2, 0.1, 0.1, 0)[0]
    for bad in ("gpu", True, 1, None, "Device"):
        with pytest.raises(ValueError, match="block_factor"):
            solvers.ManiSDP_onlyunitblockdiag(C, 3, {"block_factor": bad}, verbose=False)
        with pytest.raises(ValueError, match="block_factor"):
            solvers.ManiSDP_posegraph(Cp, 3, {"block_factor": bad}, verbose=False)
    # the old names stay refused beside the new ones
    with pytest.raises(ValueError, match="device_factor"):
        solvers.ManiSDP_onlyunitblockdiag(C, 3, {"device_factor": True, "block_factor": "device"}, verbose=False)
    with pytest.raises(ValueError, match="round"):
        solvers.ManiSDP_posegraph(Cp, 3, {"round": {"trials": 64}, "round_blocks": True}, verbose=False)
