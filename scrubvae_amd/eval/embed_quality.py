"""Is a 2-D picture of the latents faithful?  Trustworthiness, continuity and the co-ranking curves of an embedding, on the device
(csrc/rank.hip on top of the exact kNN search of csrc/knn.hip).

    neighbor_ranks(x, idx)                                             int32 [n, K]: the rank in x of the given neighbours
    trustworthiness(X, X_embedded, *, n_neighbors=5)                   sklearn.manifold.trustworthiness, Euclidean; a float
    continuity(X, X_embedded, *, n_neighbors=5)                        the same with the two spaces swapped
    embedding_quality(X, X_embedded, *, max_neighbors=30, rows_at=None)    EmbeddingQuality: the curves for k = 1..K

X [n, d] and X_embedded [n, d'] are numpy or torch, host or device, any float dtype; the rows go to fp64 uncentred, as for
kneighbors.  Everything is built on one integer: rank_x(i, j) = 1 + #{l != i : key_x(i, l) < key_x(i, j)}, the place of row j
among the n - 1 other rows as seen from row i in the space x, with the strict key of kneighbors (the squared distance of
csrc/pair_tiles.h compared by its bit pattern, then the lower index).  Rank 1 is the nearest other row.  With N_k^x(i) the k
neighbours of row i in x (kneighbors(x, k)):

  trustworthiness  T(k) = 1 - 2 / (n k (2 n - 3 k - 1)) sum_i sum_{j in N_k^emb(i)} max(0, rank_X(i, j) - k): are the neighbours
                   that a reader sees on the scatter neighbours in latent space?
  continuity       C(k): the same sum over j in N_k^X(i) of max(0, rank_emb(i, j) - k): do latent neighbours stay together?
  co-ranking       Q_NX(k) = sum_i |N_k^X(i) & N_k^emb(i)| / (n k), the share of each k-neighbourhood that survives, and
                   R_NX(k) = ((n - 1) Q_NX(k) - k) / (n - 1 - k), the same rescaled so that a random embedding scores 0
                   (Lee & Verleysen 2009; Lee et al. 2015).  auc_r_nx = sum_k R_NX(k) / k / sum_k 1 / k over k <= K: the area under
                   R_NX on a logarithmic k axis, truncated at K = max_neighbors (the published figure runs to n - 2).

The kernels return exact integers (the ranks; the penalty and intersection sums as int64) and the closing formulas below run once
on the host in fp64, trustworthiness in sklearn's own order of operations: on tie-free rows the result equals sklearn's bit for
bit, and it is independent of how the device splits the work.  sklearn stores the n x n distances and their argsort; here one
all-pairs pass per rank table stores nothing of size n^2, so n = 10^5 and more is fine.  n_neighbors <= KNN_MAX_K = 90.

ValueError, before any device work: mismatched row counts, non-finite rows, inputs that are not 2-D, a neighbour count that is not
an integer in range (trustworthiness and continuity: 1 <= k < n / 2 as in sklearn; embedding_quality: 1 <= K <= n - 1, with T and
C NaN at k >= n / 2), and for neighbor_ranks an idx that is not an integer [n, K] table of distinct in-range entries other than the
row itself.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _on_device
from ._inputs import _feature_rows, _is_int
from .neighbors import KNN_MAX_K, _knn_device

_RANK_CALLS = {"ranks": 0, "curves": 0}   # launches of the entry points by this process
_RANK_LAST = {"work": 0, "chunks": 0}     # bytes of work and column chunks per row tile of the last rank pass

_device_of = functools.partial(_device._device_of, who="the embedding scores run on the GPU (csrc/rank.hip); no device is available")


# ---- the closing formulas: exact integers in, fp64 out, elementwise over k ------------------------------------------------------
def trustworthiness_from_penalty(pen, n, k):
    """T(k) from pen = sum_i sum_{j in N_k(i)} max(0, rank(i, j) - k), an exact integer, in sklearn's order of operations; k may be
    an array (with pen [len(k)])"""
    if np.ndim(k) == 0:
        return 1.0 - pen * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))
    pen, k = np.asarray(pen, np.int64), np.asarray(k, np.int64)
    return 1.0 - pen * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def q_nx_from_hits(hit, n, k):
    """Q_NX(k) = hit / (n k) from hit = sum_i |N_k^X(i) & N_k^emb(i)|"""
    return np.asarray(hit, np.int64) / (n * np.asarray(k, np.int64)).astype(np.float64)


def r_nx_from_q(q, n, k):
    """R_NX(k) = ((n - 1) Q_NX(k) - k) / (n - 1 - k); NaN at k = n - 1, where every row is a neighbour in both spaces"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.int64)
    den = np.where(k < n - 1, n - 1 - k, 1).astype(np.float64)
    return np.where(k < n - 1, ((n - 1.0) * q - k) / den, np.nan)


def auc_r_nx(r, k):
    """sum_k R_NX(k) / k / sum_k 1 / k over the given k (those with a finite R_NX), added in ascending k"""
    r, k = np.asarray(r, np.float64).reshape(-1), np.asarray(k, np.int64).reshape(-1)
    num = den = np.float64(0.0)
    for rv, kv in zip(r, k):
        if np.isfinite(rv):
            num = num + rv / np.float64(kv)
            den = den + 1.0 / np.float64(kv)
    return float(num / den) if den > 0 else float("nan")


class EmbeddingQuality:
    """The curves of embedding_quality.  k = arange(1, K + 1); trustworthiness, continuity, q_nx, r_nx are fp64 [K] with entry
    k - 1 the value at k (T and C NaN at k >= n / 2, R_NX NaN at k = n - 1); auc_r_nx a float.  penalty and hits are the int64 [K]
    sums they were made of (penalty: {"trustworthiness", "continuity"}).  With rows_at = k, intrusion_rows [n] and extrusion_rows
    [n] (int64) are each row's share of the trustworthiness and continuity penalties at that k: rows whose scatter neighbours are
    far away in latent space, and rows whose latent neighbours were torn apart; both None otherwise."""
    __slots__ = ("n", "k", "trustworthiness", "continuity", "q_nx", "r_nx", "auc_r_nx", "penalty", "hits", "rows_at", "intrusion_rows",
                 "extrusion_rows")

    def __init__(self, n, pen_t, pen_c, hit, rows_at=None, intrusion_rows=None, extrusion_rows=None):
        K = len(hit)
        k = np.arange(1, K + 1, dtype=np.int64)
        self.n, self.k = int(n), k
        half = 2 * k < n
        safe = np.where(half, k, 1)
        self.penalty = {"trustworthiness": np.asarray(pen_t, np.int64), "continuity": np.asarray(pen_c, np.int64)}
        self.hits = np.asarray(hit, np.int64)
        self.trustworthiness = np.where(half, trustworthiness_from_penalty(self.penalty["trustworthiness"], n, safe), np.nan)
        self.continuity = np.where(half, trustworthiness_from_penalty(self.penalty["continuity"], n, safe), np.nan)
        self.q_nx = q_nx_from_hits(self.hits, n, k)
        self.r_nx = r_nx_from_q(self.q_nx, n, k)
        self.auc_r_nx = auc_r_nx(self.r_nx, k)
        self.rows_at, self.intrusion_rows, self.extrusion_rows = rows_at, intrusion_rows, extrusion_rows

    def __repr__(self):
        K = len(self.k)
        return (f"EmbeddingQuality(n={self.n}, K={K}, trustworthiness[K]={self.trustworthiness[-1]!r}, continuity[K]="
                f"{self.continuity[-1]!r}, q_nx[K]={self.q_nx[-1]!r}, auc_r_nx={self.auc_r_nx!r})")


# ---- argument checks, before any device work ------------------------------------------------------------------------------------
def _eq_rows(a, name):
    x = _feature_rows(a, name)
    if x.shape[0] >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 rows are supported, got {x.shape[0]}")
    return x


def _eq_pair(X, X_embedded):
    x, y = _eq_rows(X, "X"), _eq_rows(X_embedded, "X_embedded")
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"X and X_embedded must have one row count, got {x.shape[0]} and {y.shape[0]}")
    return x, y


def _eq_count(value, n, name, half):
    if not _is_int(value):
        raise ValueError(f"{name} must be an integer, got {value!r}")
    k = int(value)
    if k < 1:
        raise ValueError(f"{name} must be at least 1, got {k}")
    if half and k >= n / 2:
        raise ValueError(f"{name} ({k}) should be less than n_samples / 2 ({n / 2})")
    if k > n - 1:
        raise ValueError(f"{name} must be at most n_samples - 1 = {n - 1}, got {k}")
    if k > KNN_MAX_K:
        raise ValueError(f"at most {KNN_MAX_K} neighbours are supported, got {name} = {k}")
    return k


def _eq_idx(idx, n):
    """idx -> int32 [n, K] numpy, checked: shape, integer dtype, range, no self, distinct entries per row"""
    a = idx.detach().cpu().numpy() if torch.is_tensor(idx) else np.asarray(idx)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"idx must hold integers, got {a.dtype}")
    if a.ndim != 2 or a.shape[0] != n:
        raise ValueError(f"idx must be [n, K] with n = {n} rows, got shape {a.shape}")
    K = a.shape[1]
    if not 1 <= K <= min(n - 1, KNN_MAX_K):
        raise ValueError(f"idx must have between 1 and min(n - 1, {KNN_MAX_K}) columns with n = {n} rows, got {K}")
    if a.min() < 0 or a.max() >= n:
        raise ValueError(f"idx must lie in [0, {n}), got values in [{a.min()}, {a.max()}]")
    if (a == np.arange(n)[:, None]).any():
        raise ValueError("a row of idx names the row itself")
    if K > 1 and (np.diff(np.sort(a, axis=1), axis=1) == 0).any():
        raise ValueError("a row of idx names one row twice")
    return np.ascontiguousarray(a, dtype=np.int32)


# ---- the device side ------------------------------------------------------------------------------------------------------------
def _ranks_device(Z, idx):
    """rank int32 [n, K] on the device of Z (fp64 rows, contiguous) for idx int32 [n, K] on the same device"""
    n, d = Z.shape
    K = idx.shape[1]
    lib = _lib.lib()
    nbytes = lib.svae_rank_work(n, K)
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=Z.device)
    rank = torch.empty(n, K, dtype=torch.int32, device=Z.device)
    _RANK_CALLS["ranks"] += 1
    check(lib.svae_knn_ranks(Z.data_ptr(), d, d, n, idx.data_ptr(), K, work.data_ptr(), rank.data_ptr(), ops._stream()), "knn_ranks")
    _RANK_LAST.update(work=nbytes, chunks=(nbytes - n * K * 16) // (n * K * 4))
    return rank


def _curves_device(rank, row_k=0):
    """(pen int64 [K], hit int64 [K], pen_row int64 [n] or None) as numpy from a rank table on the device"""
    n, K = rank.shape
    sums = torch.empty(2, K, dtype=torch.int64, device=rank.device)
    rows = torch.empty(n, dtype=torch.int64, device=rank.device) if row_k else None
    _RANK_CALLS["curves"] += 1
    check(_lib.lib().svae_rank_curves(rank.data_ptr(), n, K, row_k, sums[0].data_ptr(), sums[1].data_ptr(), ops._p(rows), ops._stream()),
          "rank_curves")
    sums = sums.cpu().numpy()
    return sums[0], sums[1], None if rows is None else rows.cpu().numpy()


def _cross_ranks(Zin, Zof, k):
    """the ranks in Zin of each row's k neighbours in Zof, in neighbour order: int32 [n, k] on the device"""
    _, idx = _knn_device(Zof, k, None)
    return _ranks_device(Zin, idx)


def neighbor_ranks(x, idx):
    """rank [n, K] int32 numpy: rank[i, m] = 1 + the number of rows l != i whose key (s_il, l) is below that of idx[i, m], so 1 for
    the nearest other row of row i and n - 1 for the farthest.  idx [n, K]: integers, numpy or torch, K <= min(n - 1, KNN_MAX_K),
    every row holding distinct indices in [0, n) other than its own.  The ranks of kneighbors(x, K)'s own table are 1..K."""
    z = _eq_rows(x, "x")
    if z.shape[0] < 2:
        raise ValueError(f"ranks need at least 2 rows, got {z.shape[0]}")
    table = _eq_idx(idx, z.shape[0])
    dev = _device_of(z)
    with torch.cuda.device(dev):
        return _ranks_device(_on_device(z, dev), torch.from_numpy(table).to(dev)).cpu().numpy()


def _one_sided(inside, seen, k):
    """the penalty sum at k of the k neighbours in `seen`, ranked in `inside`"""
    dev = _device_of(inside, seen)
    with torch.cuda.device(dev):
        rank = _cross_ranks(_on_device(inside, dev), _on_device(seen, dev), k)
        pen, _, _ = _curves_device(rank)
    return int(pen[k - 1])


def trustworthiness(X, X_embedded, *, n_neighbors=5):
    """sklearn.manifold.trustworthiness(X, X_embedded, n_neighbors=n_neighbors) with the Euclidean metric: 1 when every row's
    n_neighbors neighbours in the embedding are among its n_neighbors neighbours in X, lower the farther away in X they are."""
    x, y = _eq_pair(X, X_embedded)
    k = _eq_count(n_neighbors, x.shape[0], "n_neighbors", half=True)
    return float(trustworthiness_from_penalty(_one_sided(x, y, k), x.shape[0], k))


def continuity(X, X_embedded, *, n_neighbors=5):
    """trustworthiness with the two spaces swapped: 1 when every row's n_neighbors neighbours in X are among its n_neighbors
    neighbours in the embedding, lower the farther apart the embedding puts them."""
    x, y = _eq_pair(X, X_embedded)
    k = _eq_count(n_neighbors, x.shape[0], "n_neighbors", half=True)
    return float(trustworthiness_from_penalty(_one_sided(y, x, k), x.shape[0], k))


def embedding_quality(X, X_embedded, *, max_neighbors=30, rows_at=None):
    """Trustworthiness, continuity, Q_NX and R_NX for every k = 1..max_neighbors, and auc_r_nx -> EmbeddingQuality.  Two kNN
    searches and two rank passes, whatever max_neighbors is.  rows_at = k (1 <= k <= max_neighbors) also returns each row's share
    of the two penalties at that k, to colour a scatter by where the map lies."""
    x, y = _eq_pair(X, X_embedded)
    n = x.shape[0]
    K = _eq_count(max_neighbors, n, "max_neighbors", half=False)
    at = 0
    if rows_at is not None:
        at = _eq_count(rows_at, n, "rows_at", half=False)
        if at > K:
            raise ValueError(f"rows_at must be at most max_neighbors = {K}, got {at}")
    dev = _device_of(x, y)
    with torch.cuda.device(dev):
        Zx, Zy = _on_device(x, dev), _on_device(y, dev)
        pen_t, hit, rows_t = _curves_device(_cross_ranks(Zx, Zy, K), at)
        pen_c, _, rows_c = _curves_device(_cross_ranks(Zy, Zx, K), at)
    return EmbeddingQuality(n, pen_t, pen_c, hit, rows_at=at or None, intrusion_rows=rows_t, extrusion_rows=rows_c)
