"""fp64 numpy restatement of sklearn 1.7's GaussianMixture (n_init=1, init_params="k-means++", covariance "full" / "diag") used by
test_gmm_cpu.py (against sklearn) and test_gpu_gmm.py (against csrc/gmm.hip): k-means++ with sklearn's RandomState draws and
direct squared distances, the EM loop with two-pass covariances, predict, predict_proba and score_samples."""
import numbers

import numpy as np

EPS10 = 10 * np.finfo(np.float64).eps


def check_random_state(seed):
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(seed)
    return seed


def kmeans_pp(X, K, rs):
    """sklearn.cluster._kmeans._kmeans_plusplus with unit weights and distances sum (x - c)^2 -> seed row indices"""
    X = np.asarray(X, np.float64)
    n = len(X)
    T = 2 + int(np.log(K))
    cid = rs.choice(n, p=np.ones(n) / n)
    idx = [cid]
    closest = ((X - X[cid]) ** 2).sum(1)
    pot = closest.sum()
    for _ in range(1, K):
        vals = rs.uniform(size=T) * pot
        cand = np.clip(np.searchsorted(np.cumsum(closest), vals), None, n - 1)
        d = np.stack([np.minimum(closest, ((X - X[c]) ** 2).sum(1)) for c in cand])
        pots = d.sum(1)
        b = int(np.argmin(pots))
        pot, closest = pots[b], d[b]
        idx.append(int(cand[b]))
    return np.array(idx)


def prec_chol(cov, diag):
    if diag:
        if (cov <= 0).any():
            raise ValueError("not positive definite")
        return 1.0 / np.sqrt(cov)
    out = np.empty_like(cov)
    for k, c in enumerate(cov):
        try:
            L = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            raise ValueError("not positive definite")
        out[k] = np.linalg.solve(L, np.eye(len(c))).T
    return out


def init_params(X, idx, reg, diag):
    X = np.asarray(X, np.float64)
    K, d = len(idx), X.shape[1]
    nk = 1.0 + EPS10
    means = X[idx] / nk
    weights = np.full(K, nk / len(X))
    cov = np.full((K, d), reg) if diag else np.broadcast_to(np.eye(d) * reg, (K, d, d)).copy()
    return weights, means, cov, prec_chol(cov, diag)


def weighted_log_prob(X, weights, means, P, diag):
    X = np.asarray(X, np.float64)
    K, d = means.shape
    out = np.empty((len(X), K))
    for k in range(K):
        if diag:
            q = (((X - means[k]) * P[k]) ** 2).sum(1)
            ld = np.log(P[k]).sum()
        else:
            q = (((X - means[k]) @ P[k]) ** 2).sum(1)
            ld = np.log(np.diag(P[k])).sum()
        out[:, k] = -0.5 * (d * np.log(2 * np.pi) + q) + ld + np.log(weights[k])
    return out


def estep(X, weights, means, P, diag):
    """(log_prob_norm [n], resp [n, K])"""
    w = weighted_log_prob(X, weights, means, P, diag)
    m = w.max(1)
    lpn = m + np.log(np.exp(w - m[:, None]).sum(1))
    return lpn, np.exp(w - lpn[:, None])


def mstep(X, resp, reg, diag):
    """(weights, means, covariances, precisions_cholesky): sums about the new means"""
    X = np.asarray(X, np.float64)
    nk = resp.sum(0) + EPS10
    means = resp.T @ X / nk[:, None]
    K, d = means.shape
    if diag:
        cov = np.stack([(resp[:, k:k + 1] * (X - means[k]) ** 2).sum(0) / nk[k] for k in range(K)]) + reg
    else:
        cov = np.empty((K, d, d))
        for k in range(K):
            diff = X - means[k]
            cov[k] = (resp[:, k] * diff.T) @ diff / nk[k] + reg * np.eye(d)
    return nk / nk.sum(), means, cov, prec_chol(cov, diag)


def fit(X, K, diag=False, tol=1e-3, reg=1e-6, max_iter=100, random_state=None):
    X = np.asarray(X, np.float64)
    rs = check_random_state(random_state)
    idx = kmeans_pp(X, K, rs)
    w, mu, cov, P = init_params(X, idx, reg, diag)
    lb, bounds, converged, it = -np.inf, [], False, 0
    for it in range(1, max_iter + 1):
        prev = lb
        lpn, resp = estep(X, w, mu, P, diag)
        w, mu, cov, P = mstep(X, resp, reg, diag)
        lb = lpn.mean()
        bounds.append(lb)
        if abs(lb - prev) < tol:
            converged = True
            break
    labels = weighted_log_prob(X, w, mu, P, diag).argmax(1)
    return dict(seeds=idx, weights=w, means=mu, covariances=cov, precisions_cholesky=P, n_iter=it, converged=converged,
                lower_bound=lb, lower_bounds=bounds, labels=labels)


def predict(X, f, diag):
    return weighted_log_prob(X, f["weights"], f["means"], f["precisions_cholesky"], diag).argmax(1)


def predict_proba(X, f, diag):
    return estep(X, f["weights"], f["means"], f["precisions_cholesky"], diag)[1]


def score_samples(X, f, diag):
    return estep(X, f["weights"], f["means"], f["precisions_cholesky"], diag)[0]


def top_gap(X, f, diag):
    w = np.sort(weighted_log_prob(X, f["weights"], f["means"], f["precisions_cholesky"], diag), 1)
    return w[:, -1] - w[:, -2]


def cluster_entropy_literal(k_preds0, k_preds1, n_components):
    """the inner loop of the reference's epoch_cluster_entropy (eval/metrics.py:133-147) as written there"""
    entropy = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n_components):
            hist = (np.histogram(k_preds0[k_preds1 == i], bins=np.arange(k_preds0.max() + 2) - 0.5)[0] / (k_preds1 == i).sum())
            entropy += np.nan_to_num(hist * np.log2(1 / hist)).sum()
    return entropy / n_components
