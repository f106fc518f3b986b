"""numpy restatement of placing new rows on a fitted t-SNE map (scrubvae_amd/eval/embed_transform.py, csrc/tsne.hip, csrc/knn.hip),
used by test_transform_cpu.py (against sklearn and a difference quotient) and test_gpu_transform.py (against the device), the
long-double truth of each sum and the gates both are held to.

The gates are derived as in the header of tsne_checks.py, not measured.  U = 2^-53; a sum of N terms is within (N - 1) U sum|terms|
of the exact sum of the rounded terms, to first order, and every term carries the roundings of its own operations:
  q = 1 / (1 + (d0 d0 + d1 d1)) carries 6 U.  rowq_i over the n map points: (n + 8) U rowq_i.
  q q d carries 15 U.  R_i: (n + 16) U sum_j |q q d|.
  P q d carries 9 U.  A_i over the k neighbours: (k + 10) U sum_e |P q d|.
  klrow_i = sum_e p log(p w) + log(rowq_i): the first part as tsne_checks' klpart with k entries, U sum p (7 + (k + 7) |log(p w)|);
      rowq is within (n + 8) U of itself, which moves its logarithm by (n + 8) U in absolute terms; the logarithm is allowed
      3 ulp = 6 U |log rowq|; the last addition U |klrow|.
  g_i = 2 (exag A_i - R_i / rowq_i): 2 (exag (tol_A + 2 U |A|) + (tol_R + (n + 11) U |R|) / rowq) + 2 U |g|: the quotient carries
      rowq's (n + 8) U, its own rounding and the product's.  When R and rowq are given as inputs (the place step alone) tol_R = 0
      and rowq is exact: 2 (exag (tol_A + 2 U |A|) + 3 U |R| / rowq) + 2 U |g|.
The cross kNN involves no gate: the key is strict, so indices and distances are equal or wrong."""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import silhouette_checks as SC
from tests import tsne_checks as TC

U, LD, HAVE_LD = TC.U, TC.LD, TC.HAVE_LD
DEFAULTS = dict(max_iter=250, learning_rate=0.1, momentum=0.8, exaggeration=1.0, max_grad_norm=0.25)

#           m,    n,  d,  k
KNN = [(1, 64, 2, 1),
       (63, 65, 3, 15),
       (65, 1037, 16, 90),
       (130, 40, 17, 40),       # k = n, one partial column tile
       (70, 300, 70, 30)]       # d > 64: the rows restaged per tile must come from the queries
KNN_WIDE = (40000, 200, 4, 5)   # a grid large enough for one column chunk
REPULSION = [(1, 1), (1, 1037), (255, 64), (257, 65), (300, 301)]
# the blob case: 300 reference and 60 held-out rows of 5 blobs.  Of the seeds 0..9, those whose held-out rows all have their nearest
# reference latent in their own blob (the blobs are separated) are 1, 2, 4, 5, 8; with sklearn's exact map and the default
# optimiser every one of them keeps all 60 objectives at or below their initial value, and all but seed 2 (one row) put every row
# next to a map point of its blob.  Seed 4 is the one used.
BLOB = dict(n=300, m=60, d=8, blobs=5, seed=4, perplexity=30.0)


def cross_sq_dist(q, x):
    """s [m, n]: the squared distances of the rows of q to the rows of x in the contract's arithmetic (knn_checks.sq_dist)"""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    s = np.zeros((len(q), len(x)))
    for j in range(x.shape[1]):
        e = q[:, j, None] - x[None, :, j]
        s = s + e * e
    return s


def cross_keys(q, x):
    """per query (s in key order, the reference indices in key order): the key is (s, j), strict"""
    s = cross_sq_dist(q, x)
    j = np.arange(s.shape[1])
    out = []
    for row in s:
        o = np.lexsort((j, row))
        out.append((row[o], o))
    return out


def cross_neighbors(q, x, k, rows=None):
    """(dist [m, k] float64, idx [m, k] int64) of the queries (or of the given rows of them) among the rows of x"""
    q = np.asarray(q, np.float64)
    keys = cross_keys(q if rows is None else q[rows], x)
    return np.sqrt(np.stack([s[:k] for s, _ in keys])), np.stack([j[:k] for _, j in keys]).astype(np.int64)


def cross_ties(q, x, k):
    """queries with two equal s among their first k + 1 keys: where there are none, any correct search returns the same lists"""
    return sum(int((np.diff(s[:k + 1]) == 0).any()) for s, _ in cross_keys(q, x))


def transfer_labels(idx, labels_ref):
    """majority label among labels_ref[idx [m, k]], a tie going to the smallest label"""
    out = []
    for row in np.asarray(labels_ref)[idx]:
        vals, count = np.unique(row, return_counts=True)
        out.append(vals[count.argmax()])          # the first maximum: the smallest label
    return np.array(out)


def cross_repulsion(Yq, Yref, dtype=np.float64):
    """(R [m, 2], rowq [m], sum_j |q q d| [m, 2]) of every query over all map points; in fp64 the sums run over j in ascending order"""
    Yq, Yref = np.asarray(Yq, np.float64).astype(dtype), np.asarray(Yref, np.float64).astype(dtype)
    d0, d1 = Yq[:, None, 0] - Yref[None, :, 0], Yq[:, None, 1] - Yref[None, :, 1]
    q = dtype(1) / (dtype(1) + (d0 * d0 + d1 * d1))
    t0, t1 = q * q * d0, q * q * d1
    if dtype is np.float64:
        R, rowq = np.zeros((len(Yq), 2)), np.zeros(len(Yq))
        for j in range(len(Yref)):
            R[:, 0], R[:, 1], rowq = R[:, 0] + t0[:, j], R[:, 1] + t1[:, j], rowq + q[:, j]
    else:
        R, rowq = np.stack([t0.sum(1), t1.sum(1)], 1), q.sum(1)
    return R, rowq, np.stack([np.abs(t0).sum(1), np.abs(t1).sum(1)], 1)


CrossGate = namedtuple("CrossGate", ["R", "rowq", "tol_R", "tol_rowq"])


def cross_repulsion_gate(Yq, Yref):
    n = len(Yref)
    R, rowq, absR = cross_repulsion(Yq, Yref, LD)
    return CrossGate(R, rowq, ((n + 16) * U * absR).astype(np.float64), ((n + 8) * U * rowq).astype(np.float64))


def place_terms(idx, P, exag, Yq, Yref, dtype=np.float64):
    """over each query's k entries in stored order: (A [m, 2], sum_e p log(p w) [m], sum |P q d| [m, 2],
    sum p (7 + (k + 7) |log(p w)|) [m]), p = exag P"""
    Yq, Yref = np.asarray(Yq, np.float64).astype(dtype), np.asarray(Yref, np.float64).astype(dtype)
    P = np.asarray(P, np.float64).astype(dtype)
    m, k = idx.shape
    A, absA, kl, klw = np.zeros((m, 2), dtype), np.zeros((m, 2), dtype), np.zeros(m, dtype), np.zeros(m, dtype)
    for e in range(k):
        j, v = idx[:, e], P[:, e]
        d0, d1 = Yq[:, 0] - Yref[j, 0], Yq[:, 1] - Yref[j, 1]
        w = dtype(1) + (d0 * d0 + d1 * d1)
        pq = v * (dtype(1) / w)
        p = dtype(exag) * v
        lg = np.log(np.where(p > 0, p * w, 1))     # an entry with p = 0 adds nothing, as its limit
        A[:, 0], A[:, 1], kl = A[:, 0] + pq * d0, A[:, 1] + pq * d1, kl + p * lg
        absA[:, 0], absA[:, 1] = absA[:, 0] + np.abs(pq * d0), absA[:, 1] + np.abs(pq * d1)
        klw = klw + p * (7 + (k + 7) * np.abs(lg))
    return A, kl, absA, klw


def place_gradient(A, R, rowq, exag):
    return 2.0 * (exag * A - R / rowq[:, None])


def place_values(idx, P, exag, Yq, Yref, R, rowq):
    """(klrow [m], g [m, 2]) in fp64 from given R and rowq"""
    A, kl, _, _ = place_terms(idx, P, exag, Yq, Yref)
    return kl + np.log(rowq), place_gradient(A, R, rowq, exag)


def clip(g, max_grad_norm):
    if max_grad_norm > 0.0:
        norm = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        with np.errstate(divide="ignore"):
            s = np.where(norm > max_grad_norm, max_grad_norm / norm, 1.0)
        g = np.where((norm > max_grad_norm)[:, None], g * s[:, None], g)
    return g


def place_step(idx, P, exag, Yq, Yref, R, rowq, update, gains, momentum, lr, max_grad_norm):
    """svae_tsne_place_step: (new Yq, update, gains, klrow, gradsq of the gained gradient, rows the clip bit)"""
    klrow, g = place_values(idx, P, exag, Yq, Yref, R, rowq)
    plain = g
    g = clip(g, max_grad_norm)
    bit = (g != plain).any(1)
    gains = np.where(update * g < 0.0, gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, 0.01)
    g = g * gains
    update = momentum * update - lr * g
    return Yq + update, update, gains, klrow, g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1], bit


PlaceGate = namedtuple("PlaceGate", ["A", "klrow", "g", "tol_A", "tol_klrow", "tol_g"])


def place_gate(idx, P, exag, Yq, Yref, R=None, rowq=None):
    """the long-double truth of A, klrow and g and their tolerances (module docstring).  R and rowq given: they are inputs, taken
    as exact; otherwise they are the cross repulsion's, with its gates."""
    n, k = len(Yref), idx.shape[1]
    A, kl, absA, klw = place_terms(idx, P, exag, Yq, Yref, LD)
    tol_A = ((k + 10) * U * absA).astype(np.float64)
    if R is None:
        rg = cross_repulsion_gate(Yq, Yref)
        R, rowq, tol_R, rel_q, rel_div = rg.R, rg.rowq, rg.tol_R, (n + 8) * U, (n + 11) * U
    else:
        R, rowq, tol_R, rel_q, rel_div = np.asarray(R).astype(LD), np.asarray(rowq).astype(LD), 0.0, 0.0, 3 * U
    klrow = kl + np.log(rowq)
    g = LD(2) * (LD(exag) * A - R / rowq[:, None])
    tol_kl = (U * klw + rel_q + 6 * U * np.abs(np.log(rowq)) + U * np.abs(klrow)).astype(np.float64)
    tol_g = (2 * (exag * (tol_A + 2 * U * np.abs(A)) + (tol_R + rel_div * np.abs(R)) / rowq[:, None]) + 2 * U * np.abs(g)).astype(np.float64)
    return PlaceGate(A, klrow, g, tol_A, tol_kl, tol_g)


def objective_ld(idx_row, P_row, y, Yref):
    """the objective of one query at y [2] in long double: sum_e p log(p w) + log(rowq)"""
    y, Yref, p = np.asarray(y).astype(LD), np.asarray(Yref, np.float64).astype(LD), np.asarray(P_row, np.float64).astype(LD)
    d = y[None, :] - Yref
    w = LD(1) + (d * d).sum(1)
    we = w[idx_row]
    return (np.where(p > 0, p * np.log(np.where(p > 0, p * we, 1)), 0)).sum() + np.log((LD(1) / w).sum())


def weighted_init(idx, P, Yref):
    """y_i = sum_e P_ie Yref[idx_ie], in neighbour order"""
    Y = np.zeros((len(idx), 2))
    for e in range(idx.shape[1]):
        Y = Y + P[:, e, None] * Yref[idx[:, e]]
    return Y


def affinities(x_ref, x_new, perplexity):
    """(idx [m, k], P [m, k], the restated Search): stages 1 and 2"""
    k = min(len(x_ref), int(math.floor(3.0 * perplexity)))
    dist, idx = cross_neighbors(x_new, x_ref, k)
    s = TC.search(dist * dist, perplexity)
    return idx, s.P, s


Placed = namedtuple("Placed", ["Y", "kl", "kl_init", "grad_norm", "idx", "P", "Y_init", "clipped"])


def transform(x_ref, Yref, x_new, perplexity=30.0, *, init="weighted", max_iter=250, learning_rate=0.1, momentum=0.8, exaggeration=1.0,
              max_grad_norm=0.25):
    """the whole loop: positions, the objective there and at the initial positions (exaggeration 1), |g| there, and how many
    (row, iteration) steps the clip bit"""
    Yref = np.asarray(Yref, np.float64)
    idx, P, _ = affinities(x_ref, x_new, perplexity)
    Y = weighted_init(idx, P, Yref) if isinstance(init, str) else np.array(init, dtype=np.float64)
    Y0 = Y
    R, rowq, _ = cross_repulsion(Y, Yref)
    kl_init, _ = place_values(idx, P, 1.0, Y, Yref, R, rowq)
    update, gains, clipped = np.zeros_like(Y), np.ones_like(Y), 0
    for _ in range(max_iter):
        R, rowq, _ = cross_repulsion(Y, Yref)
        Y, update, gains, _, _, bit = place_step(idx, P, exaggeration, Y, Yref, R, rowq, update, gains, momentum, learning_rate, max_grad_norm)
        clipped += int(bit.sum())
    R, rowq, _ = cross_repulsion(Y, Yref)
    kl, g = place_values(idx, P, 1.0, Y, Yref, R, rowq)
    return Placed(Y, kl, kl_init, np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]), idx, P, Y0, clipped)


def nearest_in_plane(Y, Yref):
    """the index of the nearest map point of every row of Y (the lowest on a tie)"""
    d = ((Y[:, None, :] - Yref[None, :, :]) ** 2).sum(2)
    return d.argmin(1)


@functools.lru_cache(maxsize=None)
def blob_case():
    """(reference rows, their blobs, held-out rows, their blobs), read-only: BLOB["n"] + BLOB["m"] rows of SC.blobs, the last m held out"""
    b = BLOB
    x, y = SC.blobs(b["n"] + b["m"], b["d"], b["blobs"], seed=b["seed"])
    out = x[:b["n"]], y[:b["n"]], x[b["n"]:], y[b["n"]:]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def knn_case(m, n, d, k):
    """(queries, reference rows) read-only, float32-representable blobs around the same centres"""
    x, _ = SC.blobs(m + n, d, 4, seed=m + n)
    q, r = x[:m], x[m:]
    q.setflags(write=False), r.setflags(write=False)
    return q, r
