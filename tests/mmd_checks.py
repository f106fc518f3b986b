"""numpy restatements of the rest of the reference's eval/metrics.py (mmd_estimate, lda_rand_cv, hungarian_match), used by
test_mmd_cpu.py (against scipy, sklearn, pandas) and test_gpu_mmd.py (against csrc/mmd.hip and csrc/decode.hip)."""
import itertools
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def pair_dist(A, B):
    """euclidean distances [len(A), len(B)] in the contract's arithmetic: s = ((a0 - b0)^2 + (a1 - b1)^2) + ... in feature order,
    every operation rounded on its own (numpy never fuses), then the correctly rounded sqrt"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    s = np.zeros((len(A), len(B)))
    for j in range(A.shape[1]):
        e = A[:, j, None] - B[None, :, j]
        s = s + e * e
    return np.sqrt(s)


def upper(D):
    """the pairs i < j of a square matrix, row by row (scipy's pdist order)"""
    return D[np.triu_indices(len(D), 1)]


def bandwidth(X, Y):
    """h = med * med, med = np.median over the pairs i < j of Z = [X; Y]: rank M / 2 for odd M, the mean of ranks M / 2 - 1 and
    M / 2 for even M"""
    Z = np.vstack([np.asarray(X, np.float64), np.asarray(Y, np.float64)])
    v = np.sort(upper(pair_dist(Z, Z)))
    M = len(v)
    med = v[M // 2] if M % 2 else (v[M // 2 - 1] + v[M // 2]) / 2
    return med * med


def mmd_terms(X, Y, h, dtype=np.float64):
    """(kxx, kyy, kxy): means of exp(-(dist^2) / h) over the pairs inside X, inside Y and across; the distances and h are always
    the fp64 ones, exp, sums and means run in `dtype`"""
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for v in (upper(pair_dist(X, X)), upper(pair_dist(Y, Y)), pair_dist(X, Y).ravel()):
            v = v.astype(dtype)
            out.append(np.mean(np.exp(-(v ** 2) / dtype(h))))
    return out


def mmd(X, Y, h):
    """the reference's arithmetic in fp64"""
    kxx, kyy, kxy = mmd_terms(X, Y, h)
    return kxx + kyy - 2 * kxy


def mmd_truth(X, Y, h):
    """the same distances and h, exp, sums and means in np.longdouble"""
    kxx, kyy, kxy = mmd_terms(X, Y, h, np.longdouble)
    return kxx + kyy - 2 * kxy


def mmd_gate(X, Y, h):
    """(truth, tolerance, u): tolerance = 8 max(e_ref, u), e_ref = |fp64 restatement - truth|, u = 2^-53 (kxx + kyy + 2 kxy)"""
    kxx, kyy, kxy = mmd_terms(X, Y, h, np.longdouble)
    truth = kxx + kyy - 2 * kxy
    u = float(2.0 ** -53 * (kxx + kyy + 2 * kxy))
    e_ref = abs(float(np.longdouble(mmd(X, Y, h)) - truth))
    return truth, 8 * max(e_ref, u), u


def rank_counts(Z, med, block=1024, threads=16):
    """(pairs i < j with dist < med, with dist <= med) of the rows Z, block by block: proves the rank of med among the M
    distances without holding them"""
    Z = np.asarray(Z, np.float64)
    n = len(Z)
    starts = range(0, n, block)

    def one(a):
        lt = le = 0
        for b in range(a, n, block):
            D = pair_dist(Z[a: a + block], Z[b: b + block])
            if a == b:
                D = upper(D)
            lt += int((D < med).sum())
            le += int((D <= med).sum())
        return lt, le

    with ThreadPoolExecutor(threads) as ex:
        res = list(ex.map(one, starts))
    return sum(r[0] for r in res), sum(r[1] for r in res)


def lda_scores(xtr, ytr, xte, classes):
    """LinearDiscriminantAnalysis() decision scores [m, K] up to a per-row constant: -1/2 (x - mu_k)' S^-1 (x - mu_k) + log prior_k,
    S = the pooled within-class scatter / (n_train - K); directions in which S is numerically zero are left out"""
    xtr, xte = np.asarray(xtr, np.float64), np.asarray(xte, np.float64)
    mus, S = [], np.zeros((xtr.shape[1], xtr.shape[1]))
    for c in classes:
        xc = xtr[ytr == c]
        mus.append(xc.mean(0))
        S += (xc - mus[-1]).T @ (xc - mus[-1])
    S /= len(xtr) - len(classes)
    lam, V = np.linalg.eigh(S)
    keep = lam > 1e-10 * lam.max()
    W = V[:, keep] / np.sqrt(lam[keep])
    out = []
    for c, mu in zip(classes, mus):
        z = (xte - mu) @ W
        out.append(-0.5 * (z ** 2).sum(1) + np.log((ytr == c).sum() / len(xtr)))
    return np.stack(out, 1)


def crosstab(x1, x2):
    """(row labels, column labels, counts): the table pandas.crosstab(x1, x2) holds"""
    k1, i1 = np.unique(x1, return_inverse=True)
    k2, i2 = np.unique(x2, return_inverse=True)
    t = np.zeros((len(k1), len(k2)), dtype=np.int64)
    for a, b in zip(i1.ravel(), i2.ravel()):
        t[a, b] += 1
    return k1, k2, t


def assignments(table):
    """every assignment of min(rows, cols) pairs of a table up to 8 x 8 with its total: [(total, rows, cols)]"""
    t = np.asarray(table)
    assert max(t.shape) <= 8
    flip = t.shape[0] > t.shape[1]
    if flip:
        t = t.T
    r = np.arange(t.shape[0])
    out = []
    for p in itertools.permutations(range(t.shape[1]), t.shape[0]):
        p = np.array(p, dtype=np.int64)
        out.append((int(t[r, p].sum()), p, r) if flip else (int(t[r, p].sum()), r, p))
    return out


def assignment_total(table):
    """(the maximum total over all assignments, how many assignments reach it), by brute force"""
    totals = [a[0] for a in assignments(table)]
    return max(totals), totals.count(max(totals))


def two_sets(nx, ny, d, seed, shift=0.5):
    g = np.random.default_rng(seed)
    x = (g.normal(size=(nx, d)) * np.exp(0.3 * g.normal(size=d))).astype(np.float32)
    y = (g.normal(size=(ny, d)) * np.exp(0.3 * g.normal(size=d)) + shift).astype(np.float32)
    return x.astype(np.float64), y.astype(np.float64)


def class_rows(n, d, K, seed, degenerate):
    g = np.random.default_rng(seed)
    y = g.integers(0, K, n)
    mus = g.normal(size=(K, d)) * 0.35
    A = g.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
    x = mus[y] + g.normal(size=(n, d)) @ A
    if degenerate:
        x[:, 0] = 3.0          # a constant column
        x[:, 1] = x[:, 2]      # a duplicated column
    return x.astype(np.float32), y
