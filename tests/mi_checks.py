"""numpy restatement of the kNN mutual-information estimators (scrubvae_amd/eval/mutual_info.py, csrc/mi.hip), used by
test_mi_cpu.py (against sklearn and scipy) and test_gpu_mi.py (against the device: rho2, nz and ny with exact equality, I within
mi_gate).

The contract.  z is [n, d] fp64 rows; y is real [n, q], 1 <= q <= 4, or integer labels [n].  s^z_ij and s^y_ij are sq_dist: per
feature e = a - b; s = s + e * e in feature order (numpy never fuses).  Every comparison is on s; non-negative doubles order like
their bit patterns, so numpy's < on the values is the device's < on the bits.

  real y (KSG, algorithm 1), k = n_neighbors:
      m_ij = max(s^z_ij, s^y_ij);  rho2_i = the k-th smallest m_ij over j != i (the row is left out by index: a duplicate row
      counts at 0);  nz_i = #{j != i : s^z_ij < rho2_i},  ny_i = #{j != i : s^y_ij < rho2_i}, both strict
      I = psi(n) + psi(k) - mean_i psi(nz_i + 1) - mean_i psi(ny_i + 1), in nats
  labels (Ross 2014, as sklearn's _compute_mi_cd): rows whose label occurs once are dropped first; n counts the kept rows
      c_i = the size of row i's class, k_i = min(k, c_i - 1);  rho2_i = the k_i-th smallest s^z_ij over j != i with
      lab_j == lab_i;  nz_i = #{j != i : s^z_ij < rho2_i} over all labels
      I = psi(n) + mean psi(k_i) - mean psi(c_i) - mean psi(nz_i + 1)

The strict < is sklearn's nextafter(radius, 0) followed by <=.  A row with rho2 = 0 counts 0 (sklearn counts the duplicates there;
no sklearn equality is claimed on such rows).

psi on a positive integer m: for m < 16, -0.5772156649015329 + (1/1 + ... + 1/(m - 1)) added in ascending order; from 16 on, with
x = float(m) and t = 1 / (x x), log(x) - 0.5 / x - t (1/12 - t (1/120 - t (1/252 - t (1/240 - t / 132)))).

The means here are exactly rounded sums (math.fsum) over n; the device's are compensated sums at fixed positions and a tree:
mi_gate bounds the difference."""
import functools
import math

import numpy as np

from tests import silhouette_checks as SC
from tests.knn_checks import grid_rows, sq_dist  # noqa: F401

MAX_K, MAX_Y = 32, 4

#          n,   d, q,  k
SIZES = [(301, 3, 1, 3),      # partial row and column tiles
         (130, 37, 2, 5),     # partial feature chunk
         (131, 128, 4, 7),    # rows not resident in LDS
         (70, 2, 1, 32),      # k at its maximum
         (30, 2, 1, 29),      # k = n - 1
         (1037, 1, 3, 10)]    # more than 16 row tiles, several column chunks
LABEL_CASE = (301, 3, 5)                 # n kept, d, k
LABEL_SIZES = (150, 100, 46, 3, 2)       # class sizes: k_i in {5, 2, 1}; two more rows carry labels of their own
SCORES = [(301, 4, 3), (523, 6, 5)]      # n, d, k of the latent_mi_scores cases
PERM_CASE = (203, 6, 2, 4, 48)           # n, d, q, k, P of the permutation test
GRID_K = 12                              # of the 25 grid points some have fewer and some more than 12 duplicates
SANITY = (1037, 3, 3, 19)                # n, d, k, P of the dependent / independent pair


def psi_int(m):
    """psi of the positive integers m, elementwise, one value at a time"""
    out = []
    for v in np.asarray(m).reshape(-1):
        v = int(v)
        assert v >= 1
        if v < 16:
            h = np.float64(0.0)
            for j in range(1, v):
                h = h + np.float64(1.0) / np.float64(j)
            out.append(np.float64(-0.5772156649015329) + h)
        else:
            x = np.float64(v)
            t = 1.0 / (x * x)
            out.append(np.log(x) - 0.5 / x - t * (1.0 / 12.0 - t * (1.0 / 120.0 - t * (1.0 / 252.0 - t * (1.0 / 240.0 - t / 132.0)))))
    return np.array(out, np.float64).reshape(np.shape(m))


@functools.lru_cache(maxsize=None)
def _psi_table(n):
    return psi_int(np.arange(1, n + 1))


def psi_of(m, n):
    """psi_int(m) for 1 <= m <= n through a table"""
    return _psi_table(n)[np.asarray(m) - 1]


def mean_of(v):
    return math.fsum(v) / np.float64(len(v))


def ksg(z, y, k):
    """(I, rho2 [n], nz [n] int64, ny [n] int64)"""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    y = y.reshape(len(y), -1)
    n = len(z)
    assert z.ndim == 2 and len(y) == n and 1 <= y.shape[1] <= MAX_Y and 1 <= k <= min(n - 1, MAX_K)
    sz, sy = sq_dist(z), sq_dist(y)
    other = ~np.eye(n, dtype=bool)
    m = np.maximum(sz, sy)
    rho2 = np.partition(np.where(other, m, np.inf), k - 1, axis=1)[:, k - 1]   # the k-th smallest over j != i
    nz = ((sz < rho2[:, None]) & other).sum(1)
    ny = ((sy < rho2[:, None]) & other).sum(1)
    I = ((psi_of(n, n) + psi_of(k, n)) - mean_of(psi_of(nz + 1, n))) - mean_of(psi_of(ny + 1, n))
    return float(I), rho2, nz, ny


def ross(z, lab, k):
    """(I, rho2, nz int64, k_i, c_i int64, kept): all but kept (a mask over the given rows) over the kept rows"""
    z, lab = np.asarray(z, np.float64), np.asarray(lab)
    uniq, inv, count = np.unique(lab, return_inverse=True, return_counts=True)
    kept = count[inv] > 1
    z, lab = z[kept], inv[kept]
    n = len(z)
    assert n >= 3 and 1 <= k <= min(n - 1, MAX_K)
    c = count[lab]
    ki = np.minimum(k, c - 1)
    sz = sq_dist(z)
    other = ~np.eye(n, dtype=bool)
    same = other & (lab[:, None] == lab[None, :])
    rho2 = np.sort(np.where(same, sz, np.inf), axis=1)[np.arange(n), ki - 1]      # the k_i-th smallest over the row's class
    nz = ((sz < rho2[:, None]) & other).sum(1)
    # the class terms per class in ascending class order, exactly rounded
    classes = [cl for cl in range(len(uniq)) if count[cl] > 1]
    mk = math.fsum(np.float64(count[cl]) * psi_of(min(k, count[cl] - 1), n) for cl in classes) / np.float64(n)
    mc = math.fsum(np.float64(count[cl]) * psi_of(count[cl], n) for cl in classes) / np.float64(n)
    I = ((psi_of(n, n) + mk) - mc) - mean_of(psi_of(nz + 1, n))
    return float(I), rho2, nz, ki, c, kept


def scores_inputs(z, y, discrete_target, random_state):
    """the preprocessing of latent_mi_scores (sklearn's _estimate_mi, all features continuous): columns over their population
    standard deviation (0 read as 1), plus 1e-10 max(1, mean |x|) noise from RandomState(random_state), z first, then a real y"""
    x = np.array(z, dtype=np.float64)
    rng = np.random.RandomState(random_state)
    sd = np.std(x, axis=0)
    x = x / np.where(sd == 0.0, 1.0, sd)
    x = x + 1e-10 * np.maximum(1, np.mean(np.abs(x), axis=0)) * rng.standard_normal(size=x.shape)
    if discrete_target:
        return x, np.asarray(y)
    t = np.array(y, dtype=np.float64)
    sd = np.std(t)
    t = t / (1.0 if sd == 0.0 else sd)
    t = t + 1e-10 * np.maximum(1, np.mean(np.abs(t))) * rng.standard_normal(size=len(t))
    return x, t


def latent_scores(z, y, discrete_target, k, random_state):
    """[d]: one clipped estimate per column of the preprocessed z"""
    x, t = scores_inputs(z, y, discrete_target, random_state)
    est = (lambda col: ross(col, t, k)[0]) if discrete_target else (lambda col: ksg(col, t, k)[0])
    return np.array([max(est(x[:, c:c + 1]), 0.0) for c in range(x.shape[1])])


def mi_gate(n):
    """54 x 2^-53 x max(1, ln n): the first-order bound on |I_device - I_restated| for one (z, y) of n rows.

    Both sides hold the same integers rho2, nz, ny (tested with exact equality), so only the arithmetic after the counts differs.
    Write u = 2^-53 and L = max(1, ln n); every psi(m) with 1 <= m <= n has |psi(m)| <= L, and so has every mean of them.
      log         the device's and numpy's log are each within 1 ulp <= 2 u |log x| of the true value: the two differ by at
                  most 4 u L.
      the series  m < 16 is divisions and additions, correctly rounded on both sides: no difference.  From 16 on, the terms
                  after the log are the same correctly rounded operations on the same inputs; the two subtractions that follow
                  the log round a perturbed value, each adding at most 1 ulp <= 2 u L to the difference: 4 u L.
                  So |psi_device(m) - psi_numpy(m)| <= 8 u L per row, and so for the mean over the rows.
      the sum     the device's compensated per-thread sum is within 2 u of its own value (second order in u apart): 2 u L on the
                  mean.  The tree over 256 threads has 8 levels, each rounding once: 8 u L on the mean.  The restatement's sum is
                  exactly rounded: 1 u L, counted with the division below.
      the mean    one division on each side: 2 u L.
                  One mean: (8 + 2 + 8 + 2) u L = 20 u L.
      closing     I = ((psi(n) + a) - m1) - m2.  psi(n), psi(k) and the label-side class terms are host numpy on both sides:
                  no difference.  Real y: m1 and m2 are device means, 40 u L; the subtraction of m1 rounds a value of at most
                  3 L and that of m2 one of at most 4 L, each differently on the two sides by at most 2 u |value|: 14 u L.
                  Labels: one device mean and the last subtraction only, 20 + 8 = 28 u L.
    Real y: (40 + 14) u L = 54 u L, which also covers labels.  latent_mi_scores clips both sides at 0, which moves them no
    further apart.  (A derived gate above 64 u L would mean a mistake in this derivation.)"""
    gate = 54 * 2.0 ** -53 * max(1.0, math.log(n))
    assert gate <= 64 * 2.0 ** -53 * max(1.0, math.log(n))
    return gate


def one_class_arguments(x, k):
    """what mutual_info._mi_check would hand to the device for rows x that all carry one label, a case it refuses (one class is
    no estimate): the only place the tests spell out that dict"""
    n = len(x)
    return dict(x=x, kind="labels", n=n, k=k, kept=np.ones(n, bool), lab=np.zeros(n, np.int32), count=np.array([n]),
                kk=np.full(n, k, np.int32))


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def real_rows(n, d, q, seed):
    """(z [n, d] blobs, y [n, q] with y_f = 0.8 z_(f mod d) + 0.6 noise), float32-representable"""
    z, _ = SC.blobs(n, d, 4, seed=seed)
    g = np.random.default_rng(seed + 1)
    y = 0.8 * z[:, np.arange(q) % d] + 0.6 * g.normal(size=(n, q))
    return z, y.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def real_case(n, d, q, k):
    """one input and its restatement, computed once: (z, y, I, rho2, nz, ny), read-only"""
    z, y = real_rows(n, d, q, seed=n + d)
    return _freeze(z, y) + (ksg(z, y, k)[0],) + _freeze(*ksg(z, y, k)[1:])


def label_rows():
    """(z [303, 3], labels [303]): classes of LABEL_SIZES rows, z shifted by its class, and two rows with labels of their own, in
    a shuffled order; the labels are not 0..K-1"""
    n, d, _ = LABEL_CASE
    g = np.random.default_rng(11)
    lab = np.concatenate([np.full(c, 7 * i - 4) for i, c in enumerate(LABEL_SIZES)] + [np.array([100, -50])])
    assert len(lab) == n + 2
    lab = lab[g.permutation(len(lab))]
    z = g.normal(size=(len(lab), d)) + 0.5 * (lab[:, None] % 5)
    return z.astype(np.float32).astype(np.float64), lab.astype(np.int64)


@functools.lru_cache(maxsize=None)
def label_case():
    """(z, labels, I, rho2, nz, k_i, c_i, kept), read-only"""
    z, lab = label_rows()
    return _freeze(z, lab) + (ross(z, lab, LABEL_CASE[2])[0],) + _freeze(*ross(z, lab, LABEL_CASE[2])[1:])


@functools.lru_cache(maxsize=None)
def grid_case(labels, k=GRID_K):
    """knn_checks.grid_rows() against its own first coordinate, as a real y or as labels: exact ties and rho2 = 0 rows"""
    z = grid_rows()
    if labels:
        lab = z[:, 0].astype(np.int64)
        return _freeze(z, lab) + (ross(z, lab, k)[0],) + _freeze(*ross(z, lab, k)[1:])
    y = z[:, :1].copy()
    return _freeze(z, y) + (ksg(z, y, k)[0],) + _freeze(*ksg(z, y, k)[1:])


def cpu_rows(n, seed, classes=0):
    """the sklearn comparison's data: Gaussian 1-D x and y = 0.8 x + 0.6 e, or (classes > 0) labels and x shifted by its label"""
    g = np.random.default_rng(seed)
    x = g.normal(size=n)
    if classes:
        lab = g.integers(0, classes, n)
        return x + lab, lab
    return x, 0.8 * x + 0.6 * g.normal(size=n)


def tie_free(keys, k):
    """keys: per row, the candidate keys of its neighbour search; True when the first k + 1 of every row are distinct"""
    return all((np.diff(np.sort(s)[:k + 1]) > 0).all() for s in keys)


def scores_rows(n, d, seed):
    """(z [n, d], y real [n] depending on columns 0 and 1, labels [n] in 0..3 depending on column 0)"""
    g = np.random.default_rng(seed)
    z = g.normal(size=(n, d)) * np.arange(1, d + 1)
    y = z[:, 0] + 0.5 * z[:, 1] ** 2 / 2.0 + 0.3 * g.normal(size=n)
    lab = np.digitize(z[:, 0] + 0.5 * g.normal(size=n), [-1.0, 0.0, 1.0])
    return z, y, lab.astype(np.int64)


@functools.lru_cache(maxsize=None)
def perm_case():
    """(z, y, perms [P, n] with row 0 the identity), read-only"""
    n, d, q, k, P = PERM_CASE
    z, y = real_rows(n, d, q, seed=n)
    g = np.random.default_rng(5)
    perms = np.stack([np.arange(n)] + [g.permutation(n) for _ in range(P - 1)])
    return _freeze(z, y, perms)


@functools.lru_cache(maxsize=None)
def sanity_case(dependent):
    """(z, y [n], perms [P, n]) with fixed seeds: y = 0.8 z_0 + noise, or a y drawn on its own"""
    n, d, k, P = SANITY
    g = np.random.default_rng(2024)
    z = g.normal(size=(n, d))
    y = 0.8 * z[:, 0] + 0.6 * g.normal(size=n) if dependent else np.random.default_rng(78).normal(size=n)
    perms = np.stack([np.random.default_rng(1000 + p).permutation(n) for p in range(P)])
    return _freeze(z, y, perms)
