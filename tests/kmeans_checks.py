"""fp64 numpy restatement of sklearn 1.7's KMeans(algorithm="lloyd") as scrubvae_amd.eval.KMeans states it, used by
test_kmeans_cpu.py (against sklearn) and test_gpu_kmeans.py (against csrc/kmeans.hip): the assignment under the strict key, one
Lloyd step, the relocation of empty clusters, the whole fit with its restarts, and the gates on re-ordered fp64 sums."""
import math

import numpy as np

from tests.gmm_checks import check_random_state, kmeans_pp  # noqa: F401  (the seeding the mixture's tests already check)

U = 2.0 ** -53


def sqdist(X, C):
    """s [n, K] = ((x0 - c0)^2 + (x1 - c1)^2) + ... in feature order, every operation rounded on its own"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    s = np.zeros((len(X), len(C)))
    for j in range(X.shape[1]):
        e = X[:, j:j + 1] - C[None, :, j]
        s = s + e * e
    return s


def assign(X, C):
    """(labels = the first nearest centre, dist = its s, gap = the second-smallest s minus the smallest, +inf for K = 1, s)"""
    s = sqdist(X, C)
    labels = s.argmin(1)  # the first minimum: equal s resolve to the lower centre index
    dist = s[np.arange(len(s)), labels]
    if s.shape[1] > 1:
        two = np.partition(s, 1, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
    else:
        gap = np.full(len(s), np.inf)
    return labels, dist, gap, s


def cluster_sums(X, labels, K):
    """sums [K, d + 1]: the rows of each cluster added up, and their count in the last column"""
    X = np.asarray(X, np.float64)
    sums = np.zeros((K, X.shape[1] + 1))
    for c in np.unique(labels):
        rows = X[labels == c]
        sums[c, :-1] = rows.sum(0)
        sums[c, -1] = len(rows)
    return sums


def relocation_rows(dist, n_empty):
    """the rows that found the empty clusters: by descending distance to their own centre, the lower index first on a tie"""
    return np.lexsort((np.arange(len(dist)), -np.asarray(dist)))[:n_empty]


def relocate(X, sums, labels, dist):
    """empty clusters in ascending order each take one far row out of its cluster's sum and count (sums is changed in place)"""
    empty = np.flatnonzero(sums[:, -1] == 0)
    for c, r in zip(empty, relocation_rows(dist, len(empty))):
        row = np.append(np.asarray(X[r], np.float64), 1.0)
        sums[labels[r]] -= row
        sums[c] = row
    return len(empty)


def finish(sums, C):
    """(C_new = sums / count, the old centre where the count is 0; shift = sum |C_new - C|^2)"""
    cnt = sums[:, -1]
    C_new = np.array(C, np.float64)
    live = cnt > 0
    C_new[live] = sums[live, :-1] / cnt[live, None]
    return C_new, float(((C_new - C) ** 2).sum())


def lloyd_step(X, C):
    """one iteration from the centres C -> dict(labels, dist, gap, sums, centers, shift, n_empty)"""
    labels, dist, gap, _ = assign(X, C)
    sums = cluster_sums(X, labels, len(C))
    n_empty = relocate(X, sums, labels, dist)
    C_new, shift = finish(sums, C)
    return dict(labels=labels, dist=dist, gap=gap, sums=sums, centers=C_new, shift=shift, n_empty=n_empty)


def lloyd(X, C, max_iter=300, tol_=0.0, trace=None):
    """sklearn's _kmeans_single_lloyd -> (labels, inertia, centers, n_iter); trace, a list, receives every step's dict"""
    C = np.array(C, np.float64)
    prev = np.full(len(X), -1)
    strict, it = False, 0
    for it in range(1, max_iter + 1):
        st = lloyd_step(X, C)
        if trace is not None:
            trace.append(dict(st, centers_in=C))
        C, labels, dist = st["centers"], st["labels"], st["dist"]
        if np.array_equal(labels, prev):
            strict = True
            break
        if st["shift"] <= tol_:
            break
        prev = labels
    if not strict:
        labels, dist, gap, _ = assign(X, C)
        if trace is not None:
            trace.append(dict(labels=labels, dist=dist, gap=gap, centers_in=C, final=True))
    return labels, float(dist.sum()), C, it


def is_same_clustering(l1, l2, K):
    m = np.full(K, -1)
    u, first = np.unique(l1, return_index=True)
    m[u] = l2[first]
    return bool((m[l1] == l2).all())


def tolerance(Xc, tol):
    """tol * the mean over columns of var(X) of centred rows: their sum of squares (distances to one zero centre) / (n d)"""
    n, d = Xc.shape
    return tol * float(assign(Xc, np.zeros((1, d)))[1].sum()) / (n * d)


def fit(X, K, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, random_state=None, centred=False, trace=None):
    """KMeans.fit -> dict(labels, inertia, centers, n_iter, mean); centred=True: X are centred rows already (the device's own A)
    and the centres, an init array included, are in that frame."""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    rs = check_random_state(random_state)
    mean = np.zeros(d) if centred else X.mean(0)
    Xc = X - mean
    tol_ = tolerance(Xc, tol)
    is_array = not isinstance(init, str)
    if n_init == "auto":
        n_init = 1 if is_array or init == "k-means++" else 10
    best = None
    for _ in range(n_init):
        if is_array:
            C0 = np.asarray(init, np.float64) - mean
        elif init == "k-means++":
            C0 = Xc[kmeans_pp(Xc, K, rs)]
        else:
            C0 = Xc[rs.choice(n, size=K, replace=False, p=np.ones(n) / n)]
        tr = [] if trace is not None else None
        labels, inertia, C, it = lloyd(Xc, C0, max_iter, tol_, tr)
        if best is None or (inertia < best["inertia"] and not is_same_clustering(labels, best["labels"], K)):
            best = dict(labels=labels, inertia=inertia, centers=C + mean, n_iter=it, mean=mean, tol_=tol_)
        if trace is not None:
            trace.extend(tr)  # every restart's steps, in order
    return best


# ---- gates: bounds on fp64 sums added in another order ----------------------------------------------------------------------------
def centre_gate(X):
    """|x|max n 2^-53 on a centre of rows X"""
    X = np.asarray(X)
    return float(np.abs(X).max()) * len(X) * U


def inertia_gate(n):
    """relative"""
    return n * U


def fsum_cluster_sums(X, labels, K):
    """exactly rounded sums [K, d + 1] and the bound (m_c - 1) 2^-53 sum |a_rf| on a plain fp64 sum of them in any order"""
    X = np.asarray(X, np.float64)
    d = X.shape[1]
    sums, bound = np.zeros((K, d + 1)), np.zeros((K, d + 1))
    for c in range(K):
        rows = X[labels == c]
        m = len(rows)
        sums[c, d] = m
        for f in range(d):
            sums[c, f] = math.fsum(rows[:, f])
            bound[c, f] = max(m - 1, 0) * U * math.fsum(np.abs(rows[:, f]))
    return sums, bound
