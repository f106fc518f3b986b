"""fp64 numpy / torch restatements of the decodability metrics (reference src/scrubvae/eval/metrics.py:231-329) used by
test_decodability_cpu.py (against sklearn) and test_gpu_decodability.py (against csrc/decode.hip)."""
import numpy as np
import torch


def kfold_split(n, folds):
    """KFold(n_splits=folds, shuffle=True, random_state=100).split: list of (train, test) index arrays."""
    if n < folds:
        raise ValueError("n < folds")
    idx = np.arange(n)
    np.random.RandomState(100).shuffle(idx)
    sizes = [n // folds + (1 if f < n % folds else 0) for f in range(folds)]
    out, s = [], 0
    for sz in sizes:
        test = np.sort(idx[s: s + sz])
        s += sz
        mask = np.ones(n, bool)
        mask[test] = False
        out.append((np.nonzero(mask)[0], test))
    return out


def r2(y, p):
    """r2_score(multioutput="uniform_average") with force_finite"""
    y, p = y.reshape(len(y), -1), p.reshape(len(p), -1)
    res = ((y - p) ** 2).sum(0)
    tot = ((y - y.mean(0)) ** 2).sum(0)
    out = np.where(tot > 0, 1 - res / np.where(tot > 0, tot, 1), np.where(res == 0, 1.0, 0.0))
    return float(out.mean())


def linear_r2(xtr, ytr, xte, yte):
    """least squares with intercept by centred minimum-norm lstsq, then R^2 on the test rows"""
    xtr, ytr, xte, yte = (np.asarray(a, np.float64) for a in (xtr, ytr, xte, yte))
    ytr, yte = ytr.reshape(len(ytr), -1), yte.reshape(len(yte), -1)
    mx, my = xtr.mean(0), ytr.mean(0)
    beta = np.linalg.lstsq(xtr - mx, ytr - my, rcond=None)[0]
    return r2(yte, (xte - mx) @ beta + my)


def qda_scores(xtr, ytr, xte, classes):
    """QuadraticDiscriminantAnalysis(reg_param=0) decision scores [m, K]: -1/2 (logdet S_c + maha^2) + log prior_c"""
    xtr, xte = np.asarray(xtr, np.float64), np.asarray(xte, np.float64)
    out = []
    for c in classes:
        xc = xtr[ytr == c]
        mu = xc.mean(0)
        S = np.cov(xc, rowvar=False, ddof=1)
        L = np.linalg.cholesky(S)
        z = np.linalg.solve(L, (xte - mu).T)
        out.append(-0.5 * (2 * np.log(np.diag(L)).sum() + (z ** 2).sum(0)) + np.log(len(xc) / len(xtr)))
    return np.stack(out, 1)


def _softplus(t):
    return np.logaddexp(0.0, t)


def _sigmoid(t):
    return 0.5 * (1 + np.tanh(0.5 * t))


def logreg_grad(X, s, w, b, C=1.0, rho=0.5):
    """gradient of the smooth part of C sum log(1 + exp(-s (Xw + b))) + (1-rho)/2 |w|^2 (w part, intercept part)"""
    u = X @ w + b
    coef = -C * s * _sigmoid(-s * u)
    return X.T @ coef + (1 - rho) * w, coef.sum()


def kkt_residual(X, s, w, b, C=1.0, rho=0.5):
    """max violation of the optimality conditions of the elastic-net logistic problem"""
    g, gb = logreg_grad(X, s, w, b, C, rho)
    e = np.where(w > 0, np.abs(g + rho), np.where(w < 0, np.abs(g - rho), np.maximum(np.abs(g) - rho, 0)))
    return max(float(e.max()), abs(float(gb)))


def logreg_fit(X, s, C=1.0, rho=0.5, tol=1e-11, max_iter=100):
    """fp64 proximal Newton + cyclic coordinate descent for min C sum softplus(-s (Xw + b)) + (1-rho)/2 |w|^2 + rho |w|_1"""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    mx = X.mean(0)
    A = np.hstack([X - mx, np.ones((n, 1))])
    alpha = 1 - rho
    v = np.zeros(d + 1)

    def F(v):
        return C * _softplus(-s * (A @ v)).sum() + 0.5 * alpha * (v[:d] ** 2).sum() + rho * np.abs(v[:d]).sum()

    g0 = None
    for _ in range(max_iter):
        u = A @ v
        g = A.T @ (-C * s * _sigmoid(-s * u))
        g[:d] += alpha * v[:d]
        e = np.where(v[:d] > 0, np.abs(g[:d] + rho), np.where(v[:d] < 0, np.abs(g[:d] - rho), np.maximum(np.abs(g[:d]) - rho, 0)))
        res = max(e.max(), abs(g[d]))
        g0 = np.abs(g).max() if g0 is None else g0
        if res <= tol * g0:
            break
        q = _sigmoid(u)
        H = (A * (C * q * (1 - q))[:, None]).T @ A
        H[np.arange(d), np.arange(d)] += alpha
        nv, hd = v.copy(), np.zeros(d + 1)
        for _sw in range(2000):
            big = 0.0
            for j in range(d + 1):
                bq = g[j] + hd[j] - H[j, j] * (nv[j] - v[j])
                if j == d:
                    t = v[j] - bq / H[j, j]
                else:
                    z = H[j, j] * v[j] - bq
                    t = np.sign(z) * max(abs(z) - rho, 0.0) / H[j, j]
                dl = t - nv[j]
                if dl != 0.0:
                    hd += H[:, j] * dl
                    nv[j] = t
                    big = max(big, abs(dl))
            if big <= 1e-14 * max(np.abs(nv).max(), 1e-300):
                break
        dirn = nv - v
        f0 = F(v)
        delta = g @ dirn + rho * (np.abs(nv[:d]).sum() - np.abs(v[:d]).sum())
        t = 1.0
        while t > 1e-6 and F(v + t * dirn) > f0 + 1e-4 * t * delta + 1e-15 * abs(f0):
            t *= 0.5
        v = v + t * dirn
    w = v[:d]
    return w, v[d] - w @ mx


def mlp_predict(xtr, ytr, xte, init, dtype=torch.float64, steps=200):
    """train_MLP (metrics.py:307-329) on the CPU in `dtype` from the given initial weights [(W, b)] * 3, then predict xte"""
    lins = [torch.nn.Linear(W.shape[1], W.shape[0]).to(dtype) for W, _ in init]
    with torch.no_grad():
        for l, (W, b) in zip(lins, init):
            l.weight.copy_(W.to(dtype))
            l.bias.copy_(b.to(dtype))
    model = torch.nn.Sequential(lins[0], torch.nn.ReLU(), lins[1], torch.nn.ReLU(), lins[2])
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    x = torch.as_tensor(np.asarray(xtr), dtype=dtype)
    y = torch.as_tensor(np.asarray(ytr).reshape(len(xtr), -1), dtype=dtype)
    for _ in range(steps):
        opt.zero_grad()
        loss = torch.nn.MSELoss(reduction="sum")(model(x), y)
        loss.backward()
        opt.step()
    with torch.no_grad():
        return model(torch.as_tensor(np.asarray(xte), dtype=dtype)).numpy()
