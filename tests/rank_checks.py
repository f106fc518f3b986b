"""numpy restatement of the neighbour ranks and the embedding scores built on them (scrubvae_amd/eval/embed_quality.py,
csrc/rank.hip), used by test_rank_cpu.py (against sklearn) and test_gpu_rank.py (against the device, with exact equality).

The contract.  x is [n, d] fp64 rows, s_ij is knn_checks.sq_dist (per feature e = a - b; s = s + e * e in feature order, numpy
never fuses).  The key of (i, l) is (s_il, l), compared strictly: s as values (non-negative doubles order like their bits), then
the lower index.  rank[i, m] = 1 + #{l != i : key(i, l) < key(i, idx[i, m])}: 1 for the nearest other row, n - 1 for the farthest.

From a rank table whose column m belongs to the neighbour of order m + 1 in the other space, for k = 1..K (int64, exact):
    pen[k] = sum_i sum_{m < k} max(0, rank[i, m] - k)        hit[k] = sum_i #{m < k : rank[i, m] <= k}
The closing formulas are the module's public helpers, imported here: both sides run the same arithmetic on the same integers, and
test_rank_cpu.py pins that arithmetic to sklearn.manifold.trustworthiness."""
import functools

import numpy as np

from tests.knn_checks import grid_rows, neighbors, sorted_keys, sq_dist  # noqa: F401

MAX_K = 90

#         n,    d, K
ROWS = [(130, 5, 20),      # partial row and column tile, partial feature chunk
        (301, 3, 12),      # 5 column chunks
        (1037, 8, 30)]     # 6 column chunks
WIDE = (200, 70, 90)       # rows not resident in LDS; K at its maximum
FULL = (91, 4, 90)         # K = n - 1: every other row is a threshold
GRID_K = 12


def rows(n, d):
    """(X [n, d], Y [n, 2]): Gaussian rows and a noisy copy of their first two features"""
    r = np.random.default_rng(n)
    X = r.standard_normal((n, d))
    Y = X[:, :2] + 0.5 * r.standard_normal((n, 2))
    return X, Y


def ranks(x, idx):
    """rank [n, K] int32 of the entries of idx [n, K] among the other rows of x"""
    s = sq_dist(x)
    idx = np.asarray(idx)
    n = len(s)
    out = np.empty(idx.shape, np.int32)
    l = np.arange(n)
    for i in range(n):
        j = idx[i][:, None]
        below = (s[i][None] < s[i, idx[i]][:, None]) | ((s[i][None] == s[i, idx[i]][:, None]) & (l[None] < j))
        below[:, i] = False
        out[i] = 1 + below.sum(1)
    return out


def knn(x, K):
    """idx [n, K] int64: the K smallest keys of every row, in key order"""
    return neighbors(x, K)[1]


def curve_sums(rank):
    """(pen [K], hit [K], pen_rows [K, n]) int64; entry k - 1 belongs to k"""
    rank = np.asarray(rank, np.int64)
    n, K = rank.shape
    pen_rows = np.stack([np.maximum(rank[:, :k] - k, 0).sum(1) for k in range(1, K + 1)])
    hit = np.array([(rank[:, :k] <= k).sum() for k in range(1, K + 1)], np.int64)
    return pen_rows.sum(1), hit, pen_rows


@functools.lru_cache(maxsize=None)
def quality(n, d, K):
    """the restated embedding_quality of rows(n, d), computed once: a dict of read-only arrays and floats"""
    from scrubvae_amd.eval import embed_quality as EQ
    X, Y = rows(n, d)
    return quality_of(X, Y, K, EQ)


def quality_of(X, Y, K, EQ):
    n = len(X)
    idx_x, idx_y = knn(X, K), knn(Y, K)
    rank_t, rank_c = ranks(X, idx_y), ranks(Y, idx_x)      # trustworthiness: the embedding's neighbours ranked in X
    pen_t, hit_t, rows_t = curve_sums(rank_t)
    pen_c, hit_c, rows_c = curve_sums(rank_c)
    assert np.array_equal(hit_t, hit_c)                    # |N_k^X(i) & N_k^Y(i)| counted from either side
    k = np.arange(1, K + 1)
    half = 2 * k < n
    T = np.array([EQ.trustworthiness_from_penalty(int(pen_t[a - 1]), n, int(a)) if 2 * a < n else np.nan for a in k])
    C = np.array([EQ.trustworthiness_from_penalty(int(pen_c[a - 1]), n, int(a)) if 2 * a < n else np.nan for a in k])
    q = EQ.q_nx_from_hits(hit_t, n, k)
    r = EQ.r_nx_from_q(q, n, k)
    out = dict(X=X, Y=Y, idx_x=idx_x, idx_y=idx_y, rank_t=rank_t, rank_c=rank_c, pen_t=pen_t, pen_c=pen_c, hit=hit_t, rows_t=rows_t,
               rows_c=rows_c, T=T, C=C, q=q, r=r, half=half)
    for a in out.values():
        a.setflags(write=False)
    out["auc"] = EQ.auc_r_nx(r, k)
    return out


def same(a, b):
    """equal values, NaN in the same places"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def gaps(x):
    """the smallest relative gap between consecutive sorted distances of any row to all the others: above 1e-12, sklearn's
    dot-product distances and these difference-form distances sort alike"""
    worst = np.inf
    for s, _ in sorted_keys(x):
        dist = np.sqrt(s)
        worst = min(worst, float((np.diff(dist) / dist[1:]).min()))
    return worst


def random_idx(n, K, seed):
    """K distinct columns other than the row itself per row, in random order: int64 [n, K]"""
    g = np.random.default_rng(seed)
    return np.stack([g.permutation(np.delete(np.arange(n), i))[:K] for i in range(n)])


def two_rows():
    return np.array([[0.0, 0.0], [3.0, 4.0]]), np.array([[1], [0]])
