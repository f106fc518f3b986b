"""Cost of the entropic optimal transport (scrubvae_amd/eval/transport.py, csrc/ot.hip) between two blobs of z features.

  pass      one svae_ot_softmin pass (with and without cbar, both costs) at --pass-size rows on each side: synchronised host clock
            over 5 windows of --reps launches after a warm-up (the median, and (max - min) / median as its spread), as pairs per
            second, next to svae_knn_cross (k = 15) on the same rows and svae_tsne_cross_repulsion on as many 2-D points: the two
            other all-pairs walks over a rectangle.
  solve     sinkhorn and sinkhorn_divergence at --solve-size rows on each side, whole calls (inputs on the device, the median
            epsilon included), with the sweeps they ran.  With --reference, the dense numpy restatement of one sweep (the cost
            matrix stored, the two log-sum-exp passes over it in row blocks on 16 host threads) timed over --ref-sweeps sweeps;
            dense_solve_s_estimated = that time per sweep x the device's sweep count, an estimate and named so.
  large     sinkhorn at --large-size rows on each side, where no dense baseline fits (80 GB of cost): seconds per sweep and the
            sweep count, at most --large-iter sweeps.
Prints one JSON line.

    python tools/bench_ot.py [--z 32] [--pass-size 32768] [--solve-size 10000] [--large-size 100000] [--reference]"""
import argparse
import json
import os
import sys
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd import _lib, ops
from scrubvae_amd._lib import check
from scrubvae_amd.eval import sinkhorn, sinkhorn_divergence, transport as T
from scrubvae_amd.eval._device import _clock

THREADS = 16
WINDOWS = 5   # timed windows of --reps launches each: the median is reported, the spread next to it


def blobs(nx, ny, d, seed=0, shift=1.5):
    g = np.random.default_rng(seed)
    x = g.normal(size=(nx, d)).astype(np.float32)
    y = g.normal(size=(ny, d)).astype(np.float32)
    y[:, 0] += shift
    return x, y


def timed(fn, reps, dev):
    """(median, (max - min) / median) of the seconds per launch over WINDOWS windows of `reps` launches, after a warm-up launch"""
    fn()
    per = []
    for _ in range(WINDOWS):
        t0 = _clock(dev)
        for _ in range(reps):
            fn()
        per.append((_clock(dev) - t0) / reps)
    med = float(np.median(per))
    return med, (max(per) - min(per)) / med


def bench_pass(n, d, reps):
    x, y = blobs(n, n, d)
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.lib()
    st = ops._stream()
    out = dict(n=n, d=d, reps=reps, windows=WINDOWS)
    w = np.full(n, 1.0 / n)
    off = torch.from_numpy(np.random.default_rng(1).uniform(-3, 3, n)).to(dev)
    for kind, name in ((0, "sqeuclidean"), (1, "euclidean")):
        S = T._Sets(x.astype(np.float64), y.astype(np.float64), w, w, kind)
        eps = float(S.X.var(dim=0).sum()) * (0.1 if kind == 0 else 0.1 / np.sqrt(d))
        for cbar in (False, True):
            t, spread = timed(lambda: S.softmin(S.X, S.Y, off, eps, cbar), reps, dev)
            key = f"softmin_{name}{'_cbar' if cbar else ''}"
            out.update({key + "_s": round(t, 6), key + "_spread": round(spread, 4), key + "_gpairs_per_s": round(float(n) * n / t / 1e9, 1)})
    X, Y = S.X, S.Y
    k = 15
    work = torch.empty(lib.svae_knn_cross_work(n, n, k), dtype=torch.uint8, device=dev)
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    dist = torch.empty((n, k), dtype=torch.float64, device=dev)
    t, spread = timed(lambda: check(lib.svae_knn_cross(X.data_ptr(), d, n, Y.data_ptr(), d, n, d, k, work.data_ptr(), idx.data_ptr(), dist.data_ptr(), st),
                            "knn_cross"), reps, dev)
    out.update(knn_cross_k15_s=round(t, 6), knn_cross_k15_spread=round(spread, 4), knn_cross_k15_gpairs_per_s=round(float(n) * n / t / 1e9, 1))
    Yq, Yr = X[:, :2].contiguous(), Y[:, :2].contiguous()
    rwork = torch.empty(lib.svae_tsne_cross_repulsion_work(n, n, 0), dtype=torch.float64, device=dev)
    R = torch.empty((n, 2), dtype=torch.float64, device=dev)
    rowq = torch.empty(n, dtype=torch.float64, device=dev)
    t, spread = timed(lambda: check(lib.svae_tsne_cross_repulsion(Yq.data_ptr(), n, Yr.data_ptr(), n, 0, rwork.data_ptr(), R.data_ptr(), rowq.data_ptr(), st),
                            "tsne_cross_repulsion"), reps, dev)
    out.update(tsne_cross_repulsion_2d_s=round(t, 6), tsne_cross_repulsion_2d_spread=round(spread, 4), tsne_cross_repulsion_2d_gpairs_per_s=round(float(n) * n / t / 1e9, 1))
    return out


def whole(fn, dev):
    """(result, seconds, softmin passes) of one whole call"""
    before = T._OT_CALLS["softmin"]
    t0 = _clock(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", T.ConvergenceWarning)
        res = fn()
    return res, _clock(dev) - t0, T._OT_CALLS["softmin"] - before


def dense_sweep_seconds(x, y, eps, sweeps):
    """seconds per sweep of the dense numpy restatement: C stored, both log-sum-exp passes over it in row blocks on THREADS threads"""
    x, y = x.astype(np.float64), y.astype(np.float64)
    nx, ny = len(x), len(y)
    t0 = time.perf_counter()
    C = np.zeros((nx, ny))
    for j in range(x.shape[1]):
        e = x[:, j, None] - y[None, :, j]
        C += e * e
    build_s = time.perf_counter() - t0
    inv = 1.0 / eps
    loga, logb = np.full(nx, -np.log(nx)), np.full(ny, -np.log(ny))
    f, g = np.zeros(nx), np.zeros(ny)
    step = 256

    def rows_pass(off, out):
        def one(i0):
            v = off[None, :] - C[i0:i0 + step] * inv
            M = v.max(axis=1)
            out[i0:i0 + step] = -eps * (M + np.log(np.exp(v - M[:, None]).sum(axis=1)))
        list(ex.map(one, range(0, len(out), step)))

    def cols_pass(off, out):
        def one(j0):
            v = off[:, None] - C[:, j0:j0 + step] * inv
            M = v.max(axis=0)
            out[j0:j0 + step] = -eps * (M + np.log(np.exp(v - M[None, :]).sum(axis=0)))
        list(ex.map(one, range(0, len(out), step)))

    with ThreadPoolExecutor(THREADS) as ex:
        t0 = time.perf_counter()
        for _ in range(sweeps):
            rows_pass(g * inv + logb, f)
            cols_pass(f * inv + loga, g)
        return (time.perf_counter() - t0) / sweeps, build_s


def bench_solve(n, d, reference, ref_sweeps, max_iter):
    x, y = blobs(n, n, d)
    dev = torch.device("cuda", torch.cuda.current_device())
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    sinkhorn(xd[:512], yd[:512], max_iter=20, tol=0.0)                      # warm-up: code objects, torch kernels
    sinkhorn_divergence(xd[:512], yd[:512], max_iter=20, tol=0.0)
    res, t, passes = whole(lambda: sinkhorn(xd, yd, max_iter=max_iter), dev)
    out = dict(n=n, d=d, epsilon=res.epsilon, sinkhorn_s=round(t, 4), sweeps=res.n_iter, converged=res.converged, softmin_passes=passes,
               s_per_sweep=round(t / res.n_iter, 5), value=res.value, transport_cost=res.transport_cost, marginal_error=res.marginal_error)
    div, t, passes = whole(lambda: sinkhorn_divergence(xd, yd, max_iter=max_iter), dev)
    out.update(divergence_s=round(t, 4), divergence_softmin_passes=passes, divergence=div.value)
    if reference:
        per, build = dense_sweep_seconds(x, y, res.epsilon, ref_sweeps)
        out.update(dense_numpy_threads=THREADS, dense_s_per_sweep=round(per, 3), dense_cost_matrix_s=round(build, 3),
                   dense_sweeps_timed=ref_sweeps, dense_solve_s_estimated=round(per * res.n_iter + build, 1),
                   speedup_estimated=round((per * res.n_iter + build) / out["sinkhorn_s"], 1))
    return out


def bench_large(n, d, max_iter):
    x, y = blobs(n, n, d)
    dev = torch.device("cuda", torch.cuda.current_device())
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    res, t, passes = whole(lambda: sinkhorn(xd, yd, max_iter=max_iter), dev)
    return dict(n=n, d=d, epsilon=res.epsilon, sinkhorn_s=round(t, 3), sweeps=res.n_iter, converged=res.converged, softmin_passes=passes,
                s_per_sweep=round(t / res.n_iter, 4), gpairs_per_s_whole_call=round(float(n) * n * passes / t / 1e9, 1), value=res.value,
                marginal_error=res.marginal_error)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--z", type=int, default=32)
    ap.add_argument("--pass-size", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--solve-size", type=int, default=10000)
    ap.add_argument("--solve-iter", type=int, default=1000)
    ap.add_argument("--large-size", type=int, default=100000)
    ap.add_argument("--large-iter", type=int, default=200)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-sweeps", type=int, default=2)
    a = ap.parse_args()
    torch.set_num_threads(THREADS)
    out = dict(device=torch.cuda.get_device_name(0))
    for name, fn in (("pass", lambda: bench_pass(a.pass_size, a.z, a.reps)),
                     ("solve", lambda: bench_solve(a.solve_size, a.z, a.reference, a.ref_sweeps, a.solve_iter)),
                     ("large", lambda: bench_large(a.large_size, a.z, a.large_iter))):
        if getattr(a, f"{name}_size") > 0:
            out[name] = fn()
            print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
