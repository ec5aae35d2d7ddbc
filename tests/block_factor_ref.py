"""NumPy restatement of what msdp_blockfactor.hip computes between two trustregions() calls of the block kinds, and of its
rounding: the Gram matrix, the two-pass polar factor of the d rotation rows of every block (LAPACK's eigh in place of the
kernel's Jacobi iteration), the rank cut Y Q and the widening [Y, alpha V] followed by it, the degenerate rule, and
round_blocks.  A factor Y is (n (d + efree)) x p: blocks of d orthonormal rows and, for efree = 1, one free row."""
import numpy as np

EPS = np.finfo(np.float64).eps
DEGENERATE_RATIO = 1e-12            # lambda_min <= 1e-12 lambda_max of a block's first-pass Gram matrix


def blocks(Y, d, efree):
    """(n, d + efree, p) view of the factor."""
    B = d + efree
    return np.asarray(Y).reshape(Y.shape[0] // B, B, Y.shape[1])


def gram(Y):
    return Y.T @ Y


def block_gram(A):
    """A A' of a stack of blocks A (n, d, p)."""
    return A @ np.swapaxes(A, 1, 2)


def degenerate(G):
    """The blocks (boolean mask) whose Gram matrices G (n, d, d) the device refuses: lambda_min <= 1e-12 lambda_max."""
    w = np.linalg.eigvalsh(G)
    return ~(w[:, 0] > DEGENERATE_RATIO * w[:, -1])


def cond(G):
    w = np.linalg.eigvalsh(G)
    return w[:, -1] / np.maximum(w[:, 0], np.finfo(np.float64).tiny)


def _invsqrt(G, flip=None):
    """V diag(s / sqrt(lambda)) V' of a stack of symmetric matrices; s = -1 on the smallest eigenvalue of the blocks in `flip`."""
    w, V = np.linalg.eigh(G)
    s = 1.0 / np.sqrt(np.maximum(w, np.finfo(np.float64).tiny))
    if flip is not None:
        s[:, 0] = np.where(flip, -s[:, 0], s[:, 0])
    return (V * s[:, None, :]) @ np.swapaxes(V, 1, 2)


def polar_two_pass(A, flip=None):
    """(A A')^(-1/2) A of every block of the stack A (n, d, p), applied twice: the second pass starts from a block that is
    orthonormal to about 4 eps cond(A A') and ends at rounding.  flip: see round_blocks."""
    A = np.asarray(A, dtype=np.float64)
    A = _invsqrt(block_gram(A), flip) @ A
    return _invsqrt(block_gram(A)) @ A


def polar_svd(A):
    """The polar factor u v' of every block through LAPACK's SVD: the reference of the tests."""
    u, _, vt = np.linalg.svd(A, full_matrices=False)
    return u @ vt


def _reorthonormalise(Z, d, efree, polar):
    A = np.array(blocks(Z, d, efree))
    A[:, :d, :] = polar(A[:, :d, :])
    return np.ascontiguousarray(A.reshape(Z.shape))


def rotate(Y, d, efree, Q, polar=polar_two_pass):
    """polar_blocks(Y Q): the rotation rows re-orthonormalised, a free row the plain product."""
    return _reorthonormalise(Y @ Q, d, efree, polar)


def append(Y, d, efree, V, alpha, polar=polar_two_pass):
    """polar_blocks([Y, alpha V])."""
    return _reorthonormalise(np.hstack([Y, alpha * V]), d, efree, polar)


def nearest_rotation_svd(Z):
    """U diag(1, .., det(U V')) V' of every block: the nearest rotation through LAPACK's SVD (unique where the smallest singular
    value is simple or the determinant positive)."""
    U, _, Vt = np.linalg.svd(Z)
    s = np.where(np.linalg.det(U @ Vt) < 0, -1.0, 1.0)
    U = U.copy()
    U[:, :, -1] *= s[:, None]
    return U @ Vt


def round_blocks(Y, d, efree, W):
    """(R, t, flipped, ndeg) as msdp_blockfactor_round defines them: Z_i = Y_i W, t_i = tau_i W; where more than half of det Z_i
    are negative the last column of every Z_i and the last entry of every t_i change sign; R_i = V diag(lambda^(-1/2) s) V' Z_i
    from Z_i Z_i' = V diag(lambda) V', s = -1 on the smallest eigenvalue where det Z_i < 0, then the plain second pass."""
    A = blocks(Y, d, efree)
    Z = A[:, :d, :] @ W
    t = np.array(A[:, d, :] @ W) if efree else None
    flipped = int(np.sum(np.linalg.det(Z) < 0) > Z.shape[0] / 2)
    if flipped:
        Z = Z.copy()
        Z[:, :, -1] *= -1.0
        if efree:
            t[:, -1] *= -1.0
    ndeg = int(np.sum(degenerate(block_gram(Z))))
    R = polar_two_pass(Z, flip=np.linalg.det(Z) < 0)
    return R, t, flipped, ndeg


def oriented(Y, d, efree, W):
    """Y with rows 0 and 1 of every block of negative det(Y_i W) exchanged: a point of the same manifold with the same Y'Y
    whose blocks all have det(Y_i W) > 0."""
    Yo = np.array(Y)
    B = d + efree
    for i in np.nonzero(np.linalg.det(blocks(Y, d, efree)[:, :d, :] @ W) < 0)[0]:
        Yo[[i * B, i * B + 1]] = Yo[[i * B + 1, i * B]]
    return Yo


def top_eigenvectors(Y, d):
    """The top-d eigenvectors of Y'Y (p x d), as Handle.round_blocks(W=None) takes them."""
    w, Q = np.linalg.eigh(gram(Y))
    return np.ascontiguousarray(Q[:, np.argsort(w)[::-1][:d]])
