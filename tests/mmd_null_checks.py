"""numpy restatement of the permutation null of the MMD statistic (scrubvae_amd.eval.mmd_permutation_test), used by
test_mmd_null_cpu.py (against the reference's recipe on relabelled arrays) and test_gpu_mmd_null.py (against csrc/mmd_null.hip)."""
import numpy as np

from tests import mmd_checks as MC


def kernel_matrix(X, Y, h, dtype=np.float64):
    """K [n, n] over Z = [X; Y]: exp(-(dist^2) / h) with the fp64 distances of mmd_checks.pair_dist, exp in `dtype`.  Symmetric to
    the bit: (a - b)^2 == (b - a)^2."""
    Z = np.vstack([np.asarray(X, np.float64), np.asarray(Y, np.float64)])
    v = MC.pair_dist(Z, Z).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.exp(-(v ** 2) / dtype(h))


def null_terms(X, Y, h, perms, dtype=np.float64):
    """(kxx, kyy, kxy) [P] each: for every row of perms, rows perms[p, :nx] of Z relabelled X and the rest Y, the means of K over
    the upper triangle of the relabelled XX and YY blocks and over the cross block, in `dtype`: mmd_checks.mmd_terms of the
    relabelled arrays, element for element"""
    nx = len(X)
    K = kernel_matrix(X, Y, h, dtype)
    perms = np.asarray(perms)
    iu_x, iu_y = np.triu_indices(nx, 1), np.triu_indices(K.shape[0] - nx, 1)
    out = np.empty((3, len(perms)), dtype=dtype)
    for p, perm in enumerate(perms):
        ix, iy = perm[:nx], perm[nx:]
        out[0, p] = np.mean(K[np.ix_(ix, ix)][iu_x])
        out[1, p] = np.mean(K[np.ix_(iy, iy)][iu_y])
        out[2, p] = np.mean(K[np.ix_(ix, iy)].ravel())
    return out


def null_stats(X, Y, h, perms, dtype=np.float64):
    """T_p = kxx + kyy - 2 kxy [P] of every relabelling, in `dtype`"""
    kxx, kyy, kxy = null_terms(X, Y, h, perms, dtype)
    return kxx + kyy - 2 * kxy


def null_gate(X, Y, h, perms, restated=None):
    """mmd_checks.mmd_gate's rule for every relabelled split -> (truth [P] longdouble, tolerance [P], u [P], restated [P]):
    tolerance = 8 max(e_ref, u), e_ref = |fp64 restatement - truth|, u = 2^-53 (kxx + kyy + 2 kxy)"""
    kxx, kyy, kxy = null_terms(X, Y, h, perms, np.longdouble)
    truth = kxx + kyy - 2 * kxy
    u = (2.0 ** -53 * (kxx + kyy + 2 * kxy)).astype(np.float64)
    if restated is None:
        restated = null_stats(X, Y, h, perms)
    e_ref = np.abs((restated.astype(np.longdouble) - truth).astype(np.float64))
    return truth, 8 * np.maximum(e_ref, u), u, restated


def unpack_bits(bits, P):
    """[n, words] int64 / uint64 label words -> membership [P, n] of 0 / 1"""
    b = np.asarray(bits).view(np.uint64)
    p = np.arange(P)
    return ((b[:, p >> 6] >> (p & 63).astype(np.uint64)) & np.uint64(1)).T.astype(np.int64)
