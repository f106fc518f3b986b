"""Cost of train()'s decodability metrics: each scrubvae_amd.eval.metrics function on the device at 4 096 and 20 000 downsampled
rows, z in {32, 128}, 4 classes / 3 regression targets, 5 folds; next to it the reference's own path when sklearn imports: sklearn
on the host CPUs (at most 16 threads) for linear / logistic / QDA, and train_MLP's torch recipe on the GPU for the MLP, as the
reference runs it (metrics.py:307-329: model.cuda(), z.cuda()).  Prints one JSON line: {"device": {...}, "reference": {...}} in
seconds per call (device: median of 3 after a warm-up call; reference: one call after one warm-up MLP fold).

    python tools/bench_decodability.py [--no-reference]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scrubvae_amd.eval import metrics as M

THREADS = 16
SIZES, ZS, K, NY = (4096, 20000), (32, 128), 4, 3


def data(n, d, seed=0):
    g = np.random.default_rng(seed)
    y = g.integers(0, K, n)
    x = (g.normal(size=(K, d))[y] + g.normal(size=(n, d))).astype(np.float32)
    t = (x @ g.normal(size=(d, NY)) * 0.1 + g.normal(size=(n, NY))).astype(np.float32)
    return x, y, t


def device_time(fn, *args):
    fn(*args)
    ts = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(*args)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def host_funcs():
    import warnings

    from sklearn.discriminant_analysis import QuadraticDiscriminantAnalysis
    from sklearn.linear_model import LinearRegression, LogisticRegression
    from sklearn.metrics import r2_score
    from sklearn.model_selection import KFold

    def cv(func):
        def run(z, y):
            return [func(z[tr], y[tr], z[te], y[te]) for tr, te in KFold(5, shuffle=True, random_state=100).split(z)]
        return run

    def lin(a, b, c, d):
        return r2_score(d, LinearRegression().fit(a, b).predict(c))

    def log(a, b, c, d):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            clf = LogisticRegression(l1_ratio=0.5, penalty="elasticnet", multi_class="ovr", solver="saga", max_iter=300).fit(a, b)
        return (clf.predict(c) == d).mean()

    def qda(a, b, c, d):
        return (QuadraticDiscriminantAnalysis().fit(a, b).predict(c) == d).mean()

    def mlp(a, b, c, d):  # train_MLP as the reference runs it: fp32 torch on the GPU
        dd = a.shape[1]
        net = torch.nn.Sequential(torch.nn.Linear(dd, dd), torch.nn.ReLU(), torch.nn.Linear(dd, dd), torch.nn.ReLU(),
                                  torch.nn.Linear(dd, b.shape[1])).cuda()
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
        xa, ya = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        for _ in range(200):
            opt.zero_grad()
            torch.nn.MSELoss(reduction="sum")(net(xa), ya).backward()
            opt.step()
        with torch.no_grad():
            return r2_score(d, net(torch.from_numpy(c).cuda()).cpu().numpy())

    return {"linear": cv(lin), "mlp": cv(mlp), "log_class": cv(log), "qda": cv(qda)}


def main():
    host = "--no-reference" not in sys.argv
    torch.set_num_threads(THREADS)
    os.environ.setdefault("OMP_NUM_THREADS", str(THREADS))
    dev_res, host_res = {}, {}
    hf = None
    if host:
        try:
            hf = host_funcs()
        except ImportError:
            hf = None
    if hf is not None:  # warm the reference MLP's torch kernels once
        x, _, t = data(512, 32)
        hf["mlp"](x, t)
    for n in SIZES:
        for d in ZS:
            x, y, t = data(n, d)
            xd = torch.from_numpy(x).cuda()
            tag = f"n{n}_z{d}"
            for name, fn, tgt in (("linear", M.linear_rand_cv, t), ("mlp", M.mlp_rand_cv, t), ("log_class", M.log_class_rand_cv, y),
                                  ("qda", M.qda_rand_cv, y)):
                dev_res[f"{name}_{tag}"] = round(device_time(fn, xd, tgt, 1, 5), 4)
                if hf is not None:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    hf[name](x, tgt)
                    torch.cuda.synchronize()
                    host_res[f"{name}_{tag}"] = round(time.perf_counter() - t0, 3)
    print(json.dumps({"device": dev_res, "reference": host_res if hf is not None else None,
                      "reference_path": "sklearn on %d host threads; mlp: torch on the GPU" % THREADS, "folds": 5,
                      "classes": K, "targets": NY}))


if __name__ == "__main__":
    main()
