"""Cost of the density map (scrubvae_amd/eval/density.py, csrc/density.hip) on n points of a 2-D embedding (25 blobs) and a G x G
grid, points already on the device, synchronised host clock, after a warm-up call at the smallest size:

  density_map   the whole call with one bandwidth ("scott") and with a bandwidth per point (given as a device array): argument
                checks, the launches and the copy of the grid to the host; and the launches alone (svae_density_grid), the best
                and the median of --repeat runs, with the rate of the product in TFLOP/s (2 n G^2 flops) and of the exponentials
                the kernel evaluates (256 per point and 128 x 128 tile).
  host          on the same points with at most 16 host threads: the separable numpy product (two exp arrays and a dgemm per
                block of rows: the strong baseline), at every size; sklearn.neighbors.KernelDensity(rtol=0, atol=0).score_samples
                on the grid at the sizes in --sklearn-sizes (n x G), where it ends in reasonable time.  With each the largest
                difference from the device grid relative to the grid's maximum.

Prints one JSON line.

    python tools/bench_density.py [--sizes 10000,100000,1000000] [--grids 256,512] [--sklearn-sizes 10000x256] [--repeat 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd.eval import density as DM

THREADS = 16


def points(n, seed=0):
    g = np.random.default_rng(seed)
    mu = 12.0 * g.normal(size=(25, 2))
    return mu[g.integers(0, 25, n)] + g.normal(size=(n, 2))


def separable(y, h, xs, ys, block=50000):
    """D = B^T A / n on the host, block rows at a time"""
    s = 1.0 / (2.0 * h * h)
    D = np.zeros((len(ys), len(xs)))
    for i in range(0, len(y), block):
        p = y[i:i + block]
        A = np.exp(-(xs[None, :] - p[:, :1]) ** 2 * s)
        B = np.exp(-(ys[None, :] - p[:, 1:]) ** 2 * s)
        D += B.T @ A
    return D * (s / np.pi) / len(y)


def one(n, G, repeat, with_sklearn):
    y = points(n)
    Y = torch.from_numpy(y).cuda()
    dev = Y.device
    t0 = DM._device._clock(dev)
    g = DM.density_map(Y, grid_size=G)
    whole_s = DM._device._clock(dev) - t0
    h = g.bandwidth
    rows = torch.from_numpy(h * (0.5 + np.random.default_rng(1).random(n))).cuda()
    t0 = DM._device._clock(dev)
    DM.density_map(Y, bandwidth=rows, grid_size=G)
    whole_rows_s = DM._device._clock(dev) - t0
    dx, dy = (g.xs[-1] - g.xs[0]) / (G - 1), (g.ys[-1] - g.ys[0]) / (G - 1)
    launch = {"one": [], "rows": []}
    for _ in range(repeat):
        for kind, (hh, hr) in (("one", (h, None)), ("rows", (None, rows))):
            info = {}
            DM._density_device(Y, hh, hr, float(g.xs[0]), dx, G, float(g.ys[0]), dy, G, info=info)
            launch[kind].append(info["density_s"])
    tiles = (-(-G // 128)) ** 2
    best = min(launch["one"])
    row = dict(n=n, grid=G, bandwidth=round(h, 5), density_map_s=round(whole_s, 5), density_map_rows_s=round(whole_rows_s, 5),
               launch_best_s=round(best, 6), launch_median_s=round(float(np.median(launch["one"])), 6),
               launch_rows_best_s=round(min(launch["rows"]), 6), launch_rows_median_s=round(float(np.median(launch["rows"])), 6),
               work_mb=round(DM._DENSITY_LAST["work"] / 2 ** 20, 1), product_tflops=round(2.0 * n * G * G / best / 1e12, 2),
               gexp_per_s=round(256.0 * n * tiles / best / 1e9, 1))
    t0 = time.perf_counter()
    ref = separable(y, h, g.xs, g.ys)
    host_s = time.perf_counter() - t0
    row.update(numpy_separable_s=round(host_s, 3), speedup_vs_numpy=round(host_s / whole_s, 1),
               numpy_max_difference=float(np.abs(ref - g.density).max() / g.density.max()))
    if with_sklearn:
        from sklearn.neighbors import KernelDensity
        X, Yg = np.meshgrid(g.xs, g.ys)
        t0 = time.perf_counter()
        S = np.exp(KernelDensity(bandwidth=h, rtol=0, atol=0).fit(y).score_samples(np.stack([X.ravel(), Yg.ravel()], axis=1))).reshape(G, G)
        sk_s = time.perf_counter() - t0
        row.update(sklearn_s=round(sk_s, 2), speedup_vs_sklearn=round(sk_s / whole_s, 1),
                   sklearn_max_difference=float(np.abs(S - g.density).max() / g.density.max()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--sklearn-sizes", default="10000x256")
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    torch.set_num_threads(min(torch.get_num_threads(), THREADS))
    sizes = [int(s) for s in a.sizes.split(",") if s]
    grids = [int(s) for s in a.grids.split(",") if s]
    DM.density_map(torch.from_numpy(points(min(sizes))).cuda(), grid_size=min(grids))     # warm-up: code objects, torch kernels
    DM.density_map(torch.from_numpy(points(min(sizes))).cuda(), bandwidth=torch.ones(min(sizes), dtype=torch.float64).cuda(), grid_size=min(grids))
    out = dict(device=torch.cuda.get_device_name(0), host_threads=THREADS, rows=[])
    for n in sizes:
        for G in grids:
            row = one(n, G, a.repeat, f"{n}x{G}" in a.sklearn_sizes.split(","))
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
