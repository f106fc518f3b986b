"""numpy restatement of the Hilbert-Schmidt independence criterion and its permutation null (scrubvae_amd.eval.independence), used
by test_hsic_cpu.py (against the textbook matrix forms) and test_gpu_hsic.py (against csrc/hsic.hip).

Kernel matrices in the contract's arithmetic: squared distances as mmd_checks.pair_dist sums them (feature order, every operation
rounded on its own) but without the square root, K = exp(-s / h) with exp and everything after it in `dtype`; integer y gives the
delta matrix.  Under a permutation `perm`, row perm[i] of y is paired with row i of z: L is read as L[perm][:, perm]."""
import functools

import numpy as np

from tests import mmd_checks as MC

ESTIMATORS = ("biased", "unbiased")


def sq_dist(A):
    """s [n, n] = ((a_i0 - a_j0)^2 + (a_i1 - a_j1)^2) + ... in feature order, fp64"""
    A = np.asarray(A, np.float64)
    if A.ndim == 1:
        A = A[:, None]
    s = np.zeros((len(A), len(A)))
    for j in range(A.shape[1]):
        e = A[:, j, None] - A[None, :, j]
        s = s + e * e
    return s


def bandwidth(A):
    """mmd_checks.bandwidth for one set: h = med * med, med = np.median over the pairs i < j of the rows of A"""
    A = np.asarray(A, np.float64)
    if A.ndim == 1:
        A = A[:, None]
    v = np.sort(MC.upper(MC.pair_dist(A, A)))
    M = len(v)
    med = v[M // 2] if M % 2 else (v[M // 2 - 1] + v[M // 2]) / 2
    return med * med


def gauss_matrix(A, h, dtype=np.float64):
    """exp(-s / h) on the fp64 squared distances of the rows of A, exp in `dtype`"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.exp(-sq_dist(A).astype(dtype) / dtype(h))


def delta_matrix(c, dtype=np.float64):
    c = np.asarray(c)
    return (c[:, None] == c[None, :]).astype(dtype)


def kernel_matrices(z, y, hz, hy, dtype=np.float64):
    """(K, L): the Gaussian matrix of z, and of y -- or the delta matrix when y holds integers"""
    y = np.asarray(y)
    return gauss_matrix(z, hz, dtype), (delta_matrix(y, dtype) if y.dtype.kind in "iu" else gauss_matrix(y, hy, dtype))


def hsic_terms(K, L, perm, estimator, dtype=np.float64):
    """The estimator's three terms (t1, t2, t3), the statistic being t1 - t2 + t3, for one permutation [n] or several [P, n]
    (arrays [P] then), sums and closing arithmetic in `dtype`:
      biased    t1 = tr(K L) / n^2,  t2 = 2 sum_i k_i l_i / n^3,  t3 = C D / n^4               (tr(K L) = 2 A + n)
      unbiased  t1 = tr(K~ L~) / (n (n - 3)),  t2 = 2 sum_i k~_i l~_i / ((n - 2) n (n - 3)),
                t3 = C~ D~ / ((n - 1)(n - 2) n (n - 3)), the tilde matrices with a zero diagonal   (tr(K~ L~) = 2 A)"""
    assert estimator in ESTIMATORS
    K, L = np.array(K, dtype=dtype), np.array(L, dtype=dtype)
    n = len(K)
    if estimator == "unbiased":
        np.fill_diagonal(K, 0)
        np.fill_diagonal(L, 0)
    perms = np.atleast_2d(np.asarray(perm))
    k, l = K.sum(1), L.sum(1)
    C, D = K.sum(), L.sum()  # no permutation changes the total of L
    T = np.empty(len(perms), dtype=dtype)
    S = np.empty(len(perms), dtype=dtype)
    for p, row in enumerate(perms):
        T[p] = np.sum(K * L[np.ix_(row, row)])
        S[p] = np.sum(k * l[row])
    nn = dtype(n)
    if estimator == "biased":
        t1, t2, t3 = T / (nn * nn), 2 * S / (nn * nn * nn), np.full(len(perms), C * D / (nn * nn * nn * nn), dtype=dtype)
    else:
        den = nn * (nn - 3)
        t1, t2 = T / den, 2 * S / ((nn - 2) * den)
        t3 = np.full(len(perms), C * D / ((nn - 1) * (nn - 2) * den), dtype=dtype)
    return (t1[0], t2[0], t3[0]) if np.ndim(perm) == 1 else (t1, t2, t3)


def hsic_value(K, L, perm, estimator, dtype=np.float64):
    t1, t2, t3 = hsic_terms(K, L, perm, estimator, dtype)
    return t1 - t2 + t3


def gate_of(K, L, Kl, Ll, perm, estimator, restated=None):
    """The project's rule for these estimators, mmd_checks.mmd_gate carried over -> (truth longdouble, tolerance, u, restated):
    tolerance = 8 max(e_ref, u), truth from the longdouble matrices Kl, Ll, e_ref = |fp64 restatement (from K, L) - truth|,
    u = 2^-53 (|t1| + |t2| + |t3|).  Scalars for one permutation, arrays [P] for several."""
    t1, t2, t3 = hsic_terms(Kl, Ll, perm, estimator, np.longdouble)
    truth = t1 - t2 + t3
    u = np.asarray(2.0 ** -53 * (np.abs(t1) + np.abs(t2) + np.abs(t3)), dtype=np.float64)
    if restated is None:
        restated = hsic_value(K, L, perm, estimator)
    e_ref = np.abs(np.asarray(np.asarray(restated, dtype=np.longdouble) - truth, dtype=np.float64))
    return truth, 8 * np.maximum(e_ref, u), u, restated


def hsic_gate(z, y, hz, hy, perm, estimator, restated=None):
    """gate_of on the kernel matrices of (z, y)"""
    K, L = kernel_matrices(z, y, hz, hy)
    Kl, Ll = kernel_matrices(z, y, hz, hy, np.longdouble)
    return gate_of(K, L, Kl, Ll, perm, estimator, restated)


def err_of(got, truth):
    return np.abs(np.asarray(np.asarray(got, dtype=np.longdouble) - truth, dtype=np.float64))


def numpy_permutations(n, P, seed):
    g = np.random.default_rng(seed)
    return np.stack([g.permutation(n) for _ in range(P)])


def rows(n, d, q, seed):
    """z [n, d] and a dependent y [n, q], float32-representable"""
    g = np.random.default_rng(seed)
    z = (g.normal(size=(n, d)) * np.exp(0.3 * g.normal(size=d))).astype(np.float32).astype(np.float64)
    mix = g.normal(size=(d, q)) / np.sqrt(d)
    y = (0.4 * z @ mix + g.normal(size=(n, q))).astype(np.float32).astype(np.float64)
    return z, y


def labels_of(y, classes=4):
    """integer labels with `classes` values from the first column of y, by its quantiles"""
    v = np.asarray(y, np.float64).reshape(len(y), -1)[:, 0]
    return np.searchsorted(np.quantile(v, np.arange(1, classes) / classes), v).astype(np.int64)


# ---- the issue's p-value cases: inputs, permutations and the restated null, computed once and left unchanged ----------------------
PVALUE_REAL = {0.0: (455, 0.456), 0.15: (7, 0.008), 0.5: (0, 0.001)}   # a -> (count of null >= statistic, p-value)
PVALUE_LABELS = {0.0: (129, 0.13), 0.25: (0, 0.001)}


@functools.lru_cache(maxsize=None)
def pvalue_case(a, labels):
    g = np.random.default_rng(7)
    z = g.normal(size=(301, 5)).astype(np.float32).astype(np.float64)
    e = g.normal(size=(301, 2))
    y = (a * z[:, :2] + e).astype(np.float32).astype(np.float64)
    if labels:
        y = (y[:, 0] > 0).astype(np.int64) + 2 * (y[:, 1] > 0.5).astype(np.int64)
    perms = numpy_permutations(301, 999, 107)
    hz, hy = bandwidth(z), (None if labels else bandwidth(y))
    K, L = kernel_matrices(z, y, hz, hy)
    t0 = hsic_value(K, L, np.arange(301), "biased")
    restated = hsic_value(K, L, perms, "biased")
    for arr in (z, y, perms, restated):
        arr.setflags(write=False)
    return dict(z=z, y=y, perms=perms, hz=hz, hy=hy, t0=t0, restated=restated)
