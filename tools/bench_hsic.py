"""Cost of hsic_permutation_test (scrubvae_amd/eval/independence.py, csrc/hsic.hip) on n rows of d latent features against a
dependent variable: real of width q in --qs, and integer labels (q = 0 in the output) with 4 classes.  Per size, after a warm-up
call at the smallest size and with the inputs already on the device: the synchronised host-clock time of the whole test at P
permutations and of its parts (the bandwidth selects, the moments, the svae_hsic_cross launches, the permuted dot products), the
rate in (pair, permutation) evaluations per second of the cross launches (pairs i < j; `executed` counts the whole 64 x 64 tiles
and chunks of 16 permutations the kernel runs), and the ratio to the only other route to the null: P calls of hsic() on permuted
rows, one call timed and scaled to P.  With --host-sizes, the numpy recipe on the host (kernel matrices once, then a gather, a
product and a sum per permutation) at those sizes: --host-perms permutations timed and scaled to P.  Prints one JSON line.

    python tools/bench_hsic.py [--sizes 2000,10000,50000] [--d 32] [--qs 1,3] [--no-labels] [--permutations 1000] [--host-sizes 2000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd.eval import independence as IN


def rows(n, d, q, seed=0):
    """z [n, d] and y: q >= 1 real columns that carry a little of z, q = 0 four classes cut from such a column"""
    g = np.random.default_rng(seed)
    z = g.standard_normal(size=(n, d)).astype(np.float32)
    y = (0.2 * z[:, :max(q, 1)] + g.standard_normal(size=(n, max(q, 1)))).astype(np.float32)
    if q == 0:
        return z, np.searchsorted(np.quantile(y[:, 0], [0.25, 0.5, 0.75]), y[:, 0]).astype(np.int64)
    return z, y


def device_call(z, y, P, seed=0):
    """z, y on the device"""
    n = z.shape[0]
    info = {}
    checked = IN._hsic_check(z, y, None, None, "biased")
    r = IN._hsic_run(checked, None, None, "biased", None, P, seed, info)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one = IN.hsic(z, y)
    torch.cuda.synchronize()
    one_s = time.perf_counter() - t0
    total = sum(info.values())
    nt, chunks = (n + 63) // 64, (P + 15) // 16 + 1  # the observed pairing is a launch of its own
    useful = (n * (n - 1) // 2) * float(P + 1)
    executed = 4096.0 * (nt * (nt + 1) // 2) * chunks * 16
    null = r["values"][1:]
    return dict(permutations=P, total_s=round(total, 5), **{k: round(v, 5) for k, v in info.items()},
                pair_perms_per_s=float(f"{useful / info['cross_s']:.4g}"), executed_per_s=float(f"{executed / info['cross_s']:.4g}"),
                one_call_s=round(one_s, 5), loop_s=round(one_s * P, 3), speedup=round(one_s * P / total, 1),
                statistic=float(r["values"][0]), pvalue=(1 + int((null >= r["values"][0]).sum())) / (1 + P), normalized=r["normalized"],
                same_statistic=bool(np.float64(one).tobytes() == np.float64(r["values"][0]).tobytes()))


def host_call(z, y, P, timed, seed=0):
    """the numpy recipe, fp64, at most the threads numpy takes by itself"""
    z, y = np.asarray(z, np.float64), np.asarray(y)
    n = len(z)
    g = np.random.default_rng(seed)

    def sq(a):
        a = a.reshape(n, -1)
        s = (a * a).sum(1)
        return np.maximum(s[:, None] + s[None, :] - 2.0 * a @ a.T, 0.0)

    def med2(s):
        return np.median(np.sqrt(s[np.triu_indices(n, 1)])) ** 2

    t0 = time.perf_counter()
    s = sq(z)
    K = np.exp(-s / med2(s))
    if y.dtype.kind in "iu":
        L = (y[:, None] == y[None, :]).astype(np.float64)
    else:
        t = sq(y.astype(np.float64))
        L = np.exp(-t / med2(t))
    k, l, C, D = K.sum(1), L.sum(1), K.sum(), L.sum()

    def stat(perm):
        return np.sum(K * L[np.ix_(perm, perm)]) / n ** 2 - 2.0 * np.sum(k * l[perm]) / n ** 3 + C * D / n ** 4

    t1 = time.perf_counter()
    stat(np.arange(n))
    for _ in range(timed):
        stat(g.permutation(n))
    per = (time.perf_counter() - t1) / (timed + 1)
    return dict(host_setup_s=round(t1 - t0, 3), host_per_permutation_s=round(per, 5), host_s=round(t1 - t0 + per * (P + 1), 2),
                host_perms_timed=timed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000,50000")
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--qs", default="1,3")
    ap.add_argument("--no-labels", action="store_true")
    ap.add_argument("--permutations", type=int, default=1000)
    ap.add_argument("--host-sizes", default="2000")
    ap.add_argument("--host-perms", type=int, default=8)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    host_sizes = [int(s) for s in a.host_sizes.split(",") if s]
    qs = [int(q) for q in a.qs.split(",") if q] + ([] if a.no_labels else [0])
    for q in qs:  # warm-up: code objects, torch kernels
        device_call(*(torch.from_numpy(t).cuda() for t in rows(256, a.d, q)), 16)
    out = dict(device=torch.cuda.get_device_name(0), calls=[])
    for n in sizes:
        for q in qs:
            z, y = rows(n, a.d, q)
            row = dict(n=n, d=a.d, q=q, **device_call(torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda(), a.permutations))
            if n in host_sizes:
                row.update(host_call(z, y, a.permutations, a.host_perms))
                row["host_speedup"] = round(row["host_s"] / row["total_s"], 1)
            out["calls"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
