"""numpy restatement of the t-SNE stages (scrubvae_amd/eval/embed.py, csrc/tsne.hip), used by test_tsne_cpu.py (against sklearn)
and test_gpu_tsne.py (against the device), the long-double truth of each sum and the gates both are held to.

The gates are derived, not measured.  U = 2^-53.  A sum of N terms added in any order is within (N - 1) U sum|terms| of the exact
sum of the rounded terms, to first order; every term carries the roundings of its own operations on top:
  q = 1 / (1 + (d0 d0 + d1 d1)), d = y_i - y_j: 6 U q (two differences and two squares: 3 U on each square, one more for their
      sum, at most that on 1 + s, one for the division).  rowq_i over `adds` terms: (adds + 8) U rowq_i.
  q q d: 15 U (two q, the difference, two products).  R_i: (adds + 16) U sum_j |q q d|.
  Z, a sum of sums: (2 adds + 8) U Z.
  val q d: 9 U.  A_i over the nnz_i entries of the row: (nnz_i + 10) U sum |val q d|.
  p log(p w): w and p w carry 7 U, which moves the logarithm by 7 U in absolute terms; the logarithm itself is allowed 3 ulp
      = 6 U of its value (OpenCL's bound for a double-precision log), the product one more: p (7 U + 7 U |log|).
      klpart_i: U sum p (7 + (nnz_i + 7) |log(p w)|).  KL = sum_i klpart_i + exag log Z with `adds` additions on the longest path:
      U sum p (7 + (adds + 7) |log(p w)|) + exag (2 adds + 8) U + 7 U |exag log Z| + U |KL|, plus |sum p - exag| |log Z| for a
      P whose sum is not exactly exag (a property of the input, where the other side normalises Q instead).
  grad = 4 (exag A - R / Z): 4 (exag (tol_A + 2 U |A|) + (tol_R + (2 adds + 11) U |R|) / Z) + 2 U |grad|.
  P of the search, exp(-d2 beta) / sum over k terms: an exp within 3 ulp = 6 U on both sides of the quotient, (k - 1) U for the
      sum, one for the division: (k + 12) U P.
`adds` is n for anything that adds a row's n terms and then the n rows (the restatement, the device with any chunking: a chain is
never longer), and the number of terms for a sum whose order is unknown (sklearn's np.dot over the condensed matrix)."""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import knn_checks as KC
from tests import silhouette_checks as SC

U = 2.0 ** -53
LD = np.longdouble
HAVE_LD = np.finfo(np.longdouble).nmant >= 63
STEPS, TOL = 100, 1e-5

#                n,   d,  k, seed    the search against sklearn (test_tsne_cpu.py).  sklearn keeps P in float32, so a row one of
# whose steps has |diff| within about 1e-7 of the 1e-5 tolerance can stop one step earlier or later there, which moves its P by
# 1e-5 of itself, a hundred float32 roundings (one such row each at seeds 200 and 203 of the second size).  The seeds below have none.
SEARCH_CPU = [(600, 16, 90, 600), (200, 3, 15, 202), (91, 2, 90, 91)]
#                n,  d,  k, seed     the search on the device (test_gpu_tsne.py)
SEARCH_GPU = [(2, 2, 1, 2), (63, 3, 15, 63), (65, 8, 64, 65), (301, 5, 90, 301)]
REPULSION_N = [2, 63, 64, 65, 129, 301, 1037]
FITS = [(400, 8, 5), (600, 16, 25)]   # n, d, blobs

Search = namedtuple("Search", ["P", "beta", "used", "near", "tiny", "steps"])


def search(d2, perplexity):
    """sklearn's _binary_search_perplexity in fp64 on d2 [n, k], the sums in neighbour order: P [n, k], beta [n] as the loop
    leaves it, `used` the beta of P, and over all steps of all rows the smallest | |diff| - 1e-5 | and the smallest |diff| whose
    sign decided a step"""
    d2 = np.asarray(d2, np.float64)
    n, k = d2.shape
    want = math.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    used, S = np.ones(n), np.ones(n)
    active = np.ones(n, dtype=bool)
    near = tiny = np.inf
    steps = np.zeros(n, dtype=np.int64)
    for _ in range(STEPS):
        at = np.flatnonzero(active)
        if len(at) == 0:
            break
        b, D = beta[at], d2[at]
        s, sdp = np.zeros(len(at)), np.zeros(len(at))
        with np.errstate(under="ignore"):
            for j in range(k):
                p = np.exp(-D[:, j] * b)
                s = s + p
                sdp = sdp + D[:, j] * p
        s = np.where(s == 0.0, 1e-8, s)
        diff = (np.log(s) + b * sdp / s) - want
        used[at], S[at] = b, s
        steps[at] += 1
        done = np.abs(diff) <= TOL
        near = min(near, float(np.abs(np.abs(diff) - TOL).min()))
        if not done.all():
            tiny = min(tiny, float(np.abs(diff[~done]).min()))   # the sign of diff is looked at only where the row goes on
        up = ~done & (diff > 0.0)
        dn = ~done & ~(diff > 0.0)
        iu, idn = at[up], at[dn]
        lo[iu] = beta[iu]
        beta[iu] = np.where(hi[iu] == np.inf, beta[iu] * 2.0, (beta[iu] + hi[iu]) / 2.0)
        hi[idn] = beta[idn]
        beta[idn] = np.where(lo[idn] == -np.inf, beta[idn] / 2.0, (beta[idn] + lo[idn]) / 2.0)
        active[at[done]] = False
    with np.errstate(under="ignore"):
        P = np.exp(-d2 * used[:, None]) / S[:, None]
    return Search(P, beta, used, near, tiny, steps)


def search_truth(d2, used):
    """P in long double at the given beta, from the fp64 product d2 * beta"""
    e = np.exp(-(np.asarray(d2, np.float64) * used[:, None]).astype(LD))
    return e / e.sum(1, keepdims=True)


def p_gate(truth):
    return ((truth.shape[1] + 12) * U * truth).astype(np.float64)


def entropy(P):
    """-sum p log p per row in long double"""
    P = np.asarray(P).astype(LD)
    return -np.where(P > 0, P * np.log(np.where(P > 0, P, 1)), 0).sum(1)


def search_perplexity(k):
    """the perplexity the kernel tests pair with k neighbours (the public path takes k = floor(3 perplexity))"""
    return max(1.0, k / 3.0)


@functools.lru_cache(maxsize=None)
def search_case(n, d, k, seed):
    """(d2 [n, k] read-only, the restated Search): the squared kNN distances of SC.blobs(n, d, 4, seed)"""
    x, _ = SC.blobs(n, d, 4, seed=seed)
    dist, _ = KC.neighbors(x, k)
    d2 = dist * dist
    d2.setflags(write=False)
    return d2, search(d2, search_perplexity(k))


def affinities(x, perplexity):
    """(P csr [n, n] summing to 1 with sorted columns, the restated Search, the unnormalised P + P^T): steps 1 to 3 on the host"""
    from scipy.sparse import csr_matrix
    n = len(x)
    k = min(n - 1, int(math.floor(3.0 * perplexity)))
    dist, idx = KC.neighbors(x, k)
    s = search(dist * dist, perplexity)
    C = csr_matrix((s.P.reshape(-1), idx.reshape(-1), np.arange(0, n * k + 1, k)), shape=(n, n))
    S = (C + C.T).tocsr()
    S.sort_indices()
    return S / S.data.sum(), s, S


def repulsion(Y, dtype=np.float64):
    """(R [n, 2], rowq [n], Z, sum_j |q q d| [n, 2]); in fp64 the row sums run over j in ascending order and Z over i"""
    Y = np.asarray(Y, np.float64).astype(dtype)
    n = len(Y)
    d0, d1 = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
    q = dtype(1) / (dtype(1) + (d0 * d0 + d1 * d1))
    q[np.arange(n), np.arange(n)] = 0
    t0, t1 = q * q * d0, q * q * d1
    if dtype is np.float64:
        R, rowq = np.zeros((n, 2)), np.zeros(n)
        for j in range(n):
            R[:, 0], R[:, 1], rowq = R[:, 0] + t0[:, j], R[:, 1] + t1[:, j], rowq + q[:, j]
        Z = 0.0
        for i in range(n):
            Z = Z + rowq[i]
    else:
        R, rowq = np.stack([t0.sum(1), t1.sum(1)], 1), q.sum(1)
        Z = rowq.sum()
    return R, rowq, Z, np.stack([np.abs(t0).sum(1), np.abs(t1).sum(1)], 1)


RepGate = namedtuple("RepGate", ["R", "rowq", "Z", "tol_R", "tol_rowq", "tol_Z"])


def repulsion_gate(Y, adds=None):
    n = len(Y)
    adds = n if adds is None else adds
    R, rowq, Z, absR = repulsion(Y, LD)
    return RepGate(R, rowq, Z, ((adds + 16) * U * absR).astype(np.float64), ((adds + 8) * U * rowq).astype(np.float64),
                   float((2 * adds + 8) * U * Z))


def err(got, truth):
    return np.abs((np.asarray(got).astype(LD) - truth).astype(np.float64))


def csr_rows(P):
    """(rowptr, col, val) of a scipy csr matrix as int32, int32, float64"""
    return P.indptr.astype(np.int32), P.indices.astype(np.int32), P.data.astype(np.float64)


def attraction(rowptr, col, val, exag, Y, dtype=np.float64):
    """(A [n, 2], klpart [n], sum |val q d| [n, 2], sum p (7 + (nnz_i + 7) |log(p w)|) [n], sum p |log(p w)| [n]) over each row's
    entries in stored order"""
    Y = np.asarray(Y, np.float64).astype(dtype)
    n = len(Y)
    A, absA, kl, klw, klabs = np.zeros((n, 2), dtype), np.zeros((n, 2), dtype), np.zeros(n, dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    for i in range(n):
        e = slice(rowptr[i], rowptr[i + 1])
        j, v = col[e], np.asarray(val[e]).astype(dtype)
        d0, d1 = Y[i, 0] - Y[j, 0], Y[i, 1] - Y[j, 1]
        w = dtype(1) + (d0 * d0 + d1 * d1)
        pq = v * (dtype(1) / w)
        p = dtype(exag) * v
        lg = np.log(np.where(p > 0, p * w, 1))   # an entry that underflowed to 0 adds nothing, as its limit
        t = np.stack([pq * d0, pq * d1, p * lg], 1)
        acc = np.zeros(3, dtype)
        for row in t:            # stored order
            acc = acc + row
        A[i], kl[i] = acc[:2], acc[2]
        absA[i] = np.abs(t[:, :2]).sum(0)
        klw[i] = (p * (7 + (len(j) + 7) * np.abs(lg))).sum()
        klabs[i] = (p * np.abs(lg)).sum()
    return A, kl, absA, klw, klabs


def gradient(A, R, Z, exag):
    return 4.0 * (exag * A - R / Z)


def step(rowptr, col, val, exag, Y, R, Z, update, gains, momentum, lr):
    """svae_tsne_step from the old Y: (new Y, update, gains, klpart, gradsq of the gained gradient)"""
    A, kl, _, _, _ = attraction(rowptr, col, val, exag, Y)
    g = gradient(A, R, Z, exag)
    gains = np.where(update * g < 0.0, gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, 0.01)
    g = g * gains
    update = momentum * update - lr * g
    return Y + update, update, gains, kl, g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]


Objective = namedtuple("Objective", ["kl", "grad", "tol_kl", "tol_grad", "klpart", "tol_klpart", "A", "tol_A"])


def objective(P, Y, exag=1.0, dtype=np.float64):
    """(KL, grad [n, 2]) of a scipy csr P (joint probabilities before the factor exag) at Y: the restatement in fp64"""
    rowptr, col, val = csr_rows(P)
    A, klpart, _, _, _ = attraction(rowptr, col, val, exag, Y, dtype)
    R, _, Z, _ = repulsion(Y, dtype)
    if dtype is np.float64:
        s = 0.0
        for v in klpart:
            s = s + v
    else:
        s = klpart.sum()
    return s + dtype(exag) * np.log(Z), dtype(4) * (dtype(exag) * A - R / Z)


def objective_gate(P, Y, exag=1.0, adds=None):
    """the long-double truth of KL and the gradient at Y and their tolerances (module docstring)"""
    rowptr, col, val = csr_rows(P)
    n = len(Y)
    adds = n if adds is None else adds
    A, klpart, absA, klw, klabs = attraction(rowptr, col, val, exag, Y, LD)
    nnz = np.diff(rowptr)
    rg = repulsion_gate(Y, adds)
    kl = klpart.sum() + LD(exag) * np.log(rg.Z)
    grad = LD(4) * (LD(exag) * A - rg.R / rg.Z)
    tol_A = ((nnz[:, None] + 10) * U * absA).astype(np.float64)
    # the per-row weights were taken with nnz_i additions; the whole sum has `adds` more on its longest path
    tol_klpart = (U * klw).astype(np.float64)
    off_sum = abs(float(LD(exag) * val.astype(LD).sum() - LD(exag))) * abs(float(np.log(rg.Z)))
    tol_kl = float(tol_klpart.sum() + U * adds * float(klabs.sum()) + exag * (2 * adds + 8) * U + 7 * U * abs(float(exag * np.log(rg.Z)))
                   + U * abs(float(kl)) + off_sum)
    tol_grad = (4 * (exag * (tol_A + 2 * U * np.abs(A)) + (rg.tol_R + (2 * adds + 11) * U * np.abs(rg.R)) / rg.Z)
                + 2 * U * np.abs(grad)).astype(np.float64)
    return Objective(kl, grad, tol_kl, tol_grad, klpart, tol_klpart, A, tol_A)


def schedule(n, *, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, n_iter_without_progress=300):
    """the arguments of sklearn's two _gradient_descent calls, the second one's `it` left open"""
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    return [dict(it=0, max_iter=250, momentum=0.5, learning_rate=lr, n_iter_without_progress=250, exag=float(early_exaggeration)),
            dict(it=None, max_iter=max_iter, momentum=0.8, learning_rate=lr, n_iter_without_progress=n_iter_without_progress, exag=1.0)]


def optimise(P, Y0, *, min_grad_norm=1e-7, **kw):
    """sklearn's TSNE._tsne loop with the restated exact objective on a csr P -> (Y, n_iter_, [(it at entry, it at exit)], checks)"""
    Y = np.array(Y0, dtype=np.float64)
    rowptr, col, val = csr_rows(P)
    it, spans, checks = -1, [], []
    for ph in schedule(len(Y), **kw):
        first = it + 1 if ph["it"] is None else ph["it"]
        it = first                # sklearn's _gradient_descent returns its `it` when the loop has nothing left to do
        update, gains = np.zeros_like(Y), np.ones_like(Y)
        best, best_iter = np.finfo(np.float64).max, first
        for i in range(first, ph["max_iter"]):
            it = i
            R, _, Z, _ = repulsion(Y)
            Y, update, gains, klpart, gradsq = step(rowptr, col, val, ph["exag"], Y, R, Z, update, gains, ph["momentum"], ph["learning_rate"])
            if (i + 1) % 50 == 0:
                kl = float(klpart.sum() + ph["exag"] * np.log(Z))
                checks.append((i, kl))
                if kl < best:
                    best, best_iter = kl, i
                elif i - best_iter > ph["n_iter_without_progress"]:
                    break
                if math.sqrt(gradsq.sum()) <= min_grad_norm:
                    break
        spans.append((first, it))
    return Y, it, spans, checks


def pca_init(x):
    """sklearn's init="pca" in fp64: PCA(2, svd_solver="full") scores, each component signed so that its largest-magnitude loading is
    positive, divided by the standard deviation of the first and multiplied by 1e-4"""
    xc = x - x.mean(0)
    _, _, Vt = np.linalg.svd(xc, full_matrices=False)
    V = Vt[:2]
    V = V * np.sign(V[np.arange(2), np.abs(V).argmax(1)])[:, None]
    Y = xc @ V.T
    return Y / np.std(Y[:, 0]) * 1e-4


@functools.lru_cache(maxsize=None)
def fit_case(n, d, blobs):
    x, y = SC.blobs(n, d, blobs, seed=1)
    x.setflags(write=False)
    return x, y
