"""Cost of silhouette_samples (scrubvae_amd/eval/silhouette.py, csrc/silhouette.hip) on n rows of z features around K centres: the
device time of the svae_silhouette launches (synchronised host clock, after a warm-up call at the smallest size, inputs already on
the device) at n in --sizes for K in --ks, with two rates taken over that one time: the distances (n^2 pairs per call and chunk of
256 clusters, the full square) and the fp64 label products on the matrix cores (2 flops per pair and cluster; `executed` counts the
whole 64 x 64 tiles and the 16, 64 or 256 cluster columns a block runs).  With --reference, sklearn.metrics.silhouette_samples on at
most 16 host threads at the sizes in --ref-sizes, in a child process ended after --ref-cap seconds; the sizes left out are listed.
Prints one JSON line.

    python tools/bench_silhouette.py [--reference] [--ref-sizes 8192,32768] [--ref-cap 75] [--sizes 8192,32768,131072] [--z 32] [--ks 25,256]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd.eval import silhouette as SM

THREADS = 16


def blobs(n, d, K, seed=0):
    g = np.random.default_rng(seed)
    y = g.integers(0, K, n)
    mu = 2 * g.normal(size=(K, d))
    return (mu[y] + g.normal(size=(n, d))).astype(np.float32), y


def device_call(x, y):
    """x on the device"""
    rows, lab, count, _, _, _ = SM._sil_check(x, y, None)
    info = {}
    s = SM._sil_device(rows, lab, count, info)[0]
    n, K = rows.shape[0], len(count)
    nc = 16 if K <= 16 else 64 if K <= 64 else 256
    chunks = (K + nc - 1) // nc
    nt = (n + 63) // 64
    t = info["sil_s"]
    return dict(clusters=K, columns_per_block=nc, launches=SM._SIL_LAST["ranges"], sil_s=round(t, 5),
                gpairs_per_s=round(float(n) * n * chunks / t / 1e9, 1), tflops_useful=round(2.0 * n * n * K / t / 1e12, 2),
                tflops_executed=round(2.0 * 4096 * nt * nt * chunks * nc / t / 1e12, 2), score=float(s.mean()))


REF = """
import sys, time
import numpy as np
sys.path.insert(0, {root!r})
from tools.bench_silhouette import blobs
from sklearn.metrics import silhouette_samples
x, y = blobs({n}, {d}, {K})
x = x.astype(np.float64)
t0 = time.perf_counter()
s = silhouette_samples(x, y)
print(time.perf_counter() - t0, s.mean())
"""


def reference_call(n, d, K, cap):
    env = dict(os.environ, OMP_NUM_THREADS=str(THREADS), OPENBLAS_NUM_THREADS=str(THREADS), MKL_NUM_THREADS=str(THREADS))
    try:
        r = subprocess.run([sys.executable, "-c", REF.format(root=ROOT, n=n, d=d, K=K)], capture_output=True, text=True, timeout=cap, env=env)
    except subprocess.TimeoutExpired:
        return None
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    t, v = r.stdout.strip().splitlines()[-1].split()
    return float(t), float(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,32768,131072")
    ap.add_argument("--z", type=int, default=32)
    ap.add_argument("--ks", default="25,256")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-sizes", default="8192,32768")
    ap.add_argument("--ref-cap", type=float, default=75.0)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    ks = [int(k) for k in a.ks.split(",") if k]
    ref_sizes = [int(s) for s in a.ref_sizes.split(",") if s] if a.reference else []
    for K in ks:  # warm-up: code objects of each instantiation, torch kernels
        x, y = blobs(min(sizes), a.z, K)
        device_call(torch.from_numpy(x).cuda(), y)
    out = dict(device=torch.cuda.get_device_name(0), z=a.z, calls=[],
               reference_left_out=[n for n in sizes if n not in ref_sizes] if a.reference else sizes)
    for n in sizes:
        for K in ks:
            x, y = blobs(n, a.z, K)
            row = dict(n=n, **device_call(torch.from_numpy(x).cuda(), y))
            if n in ref_sizes:
                ref = reference_call(n, a.z, K, a.ref_cap)
                row["sklearn_s"] = None if ref is None else round(ref[0], 3)
                if ref is not None:
                    row["speedup"] = round(ref[0] / row["sil_s"], 1)
                    row["score_diff"] = abs(ref[1] - row["score"])
            out["calls"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
