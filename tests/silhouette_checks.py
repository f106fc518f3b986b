"""numpy restatement of the silhouette (scrubvae_amd/eval/silhouette.py), used by test_silhouette_cpu.py (against sklearn) and
test_gpu_silhouette.py (against csrc/silhouette.hip), and the gate both hold a value to.

The gate is derived, not measured.  The truth is the np.longdouble evaluation of the same fp64 distances.  Any fp64 summation
order of the m_c <= n non-negative terms of S[i, c] is within (n - 1) 2^-53 S[i, c] of it, to first order; carried through the two
divisions, the minimum, the subtraction and the quotient this gives |s_i - truth_i| <= 2 (n + 4) u_i with
u_i = 2^-53 (a_i + b_i) / max(a_i, b_i) taken from the truth, a_i and b_i held to (n + 4) 2^-53 of themselves, and the score to the
mean of the per-row gates plus 4 * 2^-53.  The bound holds for every schedule, so it does not depend on the code under test."""
import functools
from collections import namedtuple

import numpy as np

from tests import mmd_checks as MC

EPS = 2.0 ** -53

#          n,   d,  K
SIZES = [(301, 3, 5),       # 16-column kernel, partial row and column tiles
         (130, 37, 3),      # partial feature chunk
         (131, 128, 7),     # rows not resident in LDS
         (1037, 1, 4),      # more than 16 row tiles, several column tiles per block, exact ties in one dimension
         (400, 5, 40),      # 64-column kernel
         (600, 8, 70),      # 256-column kernel
         (700, 4, 300)]     # two z chunks across the 255 / 256 boundary: 262 occupied clusters, 63 of them singletons

Parts = namedtuple("Parts", ["s", "a", "b", "nearest", "S", "uniq", "inv", "count"])
Gate = namedtuple("Gate", ["truth", "u", "tol_s", "tol_a", "tol_b", "score", "tol_score"])


def blobs(n, d, K, seed):
    """n rows around K centres, float32-representable; labels = the centre drawn (empty clusters do not occur among them)"""
    g = np.random.default_rng(seed)
    y = g.integers(0, K, n)
    mu = 2 * g.normal(size=(K, d))
    x = mu[y] + g.normal(size=(n, d))
    return x.astype(np.float32).astype(np.float64), y


def parts(x, labels, dtype=np.float64):
    """S [n, K], a, b, s in `dtype` from the fp64 distances; nearest (an index into uniq) from the values in `dtype` with the
    lowest cluster on a tie.  a = s = 0 for a row alone in its cluster, s = 0 where max(a, b) == 0."""
    uniq, inv, count = np.unique(np.asarray(labels), return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    n, K = len(inv), len(uniq)
    D = MC.pair_dist(x, x).astype(dtype)
    S = np.zeros((n, K), dtype=dtype)
    for c in range(K):
        S[:, c] = D[:, inv == c].sum(axis=1)
    rows = np.arange(n)
    m_own = count[inv]
    a = np.where(m_own > 1, S[rows, inv] / np.maximum(m_own - 1, 1).astype(dtype), dtype(0))
    other = S / count.astype(dtype)[None, :]
    other[rows, inv] = np.inf
    nearest = np.argmin(other, axis=1)  # the first minimum: the lowest c
    b = other[rows, nearest]
    mx = np.maximum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where((m_own > 1) & (mx > 0), (b - a) / np.where(mx > 0, mx, dtype(1)), dtype(0))
    return Parts(s, a, b, nearest, S, uniq, inv, count)


def gate(x, labels):
    """the long-double truth and the derived tolerances (module docstring), as fp64"""
    t = parts(x, labels, np.longdouble)
    n = len(t.s)
    mx = np.maximum(t.a, t.b)
    u = (EPS * np.where(mx > 0, (t.a + t.b) / np.where(mx > 0, mx, 1), 1)).astype(np.float64)
    tol_s = 2 * (n + 4) * u
    tol_a = ((n + 4) * EPS * t.a).astype(np.float64)
    tol_b = ((n + 4) * EPS * t.b).astype(np.float64)
    return Gate(t, u, tol_s, tol_a, tol_b, t.s.mean(), float(tol_s.mean() + 4 * EPS))


def err(got, truth):
    return np.abs((np.asarray(got).astype(np.longdouble) - truth).astype(np.float64))


def medoids(p):
    """per cluster of a Parts: the row with the smallest a, the lowest row on a tie"""
    out = np.empty(len(p.uniq), dtype=np.int64)
    for c in range(len(p.uniq)):
        rows = np.flatnonzero(p.inv == c)
        out[c] = rows[np.argmin(p.a[rows])]
    return out


@functools.lru_cache(maxsize=None)
def case(n, d, K):
    """one of SIZES: (x, labels, fp64 restatement, gate or None without a long double), computed once, read-only"""
    x, y = blobs(n, d, K, n + d)
    x.setflags(write=False)
    y.setflags(write=False)
    g = gate(x, y) if np.finfo(np.longdouble).nmant >= 63 else None
    return x, y, parts(x, y), g
