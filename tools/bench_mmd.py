"""Cost of mmd_estimate (scrubvae_amd/eval/metrics.py, csrc/mmd.hip) on two shifted Gaussian sets of nx = ny rows and z features:
the device time (synchronised host clock, after a warm-up call at the smallest size, inputs already on the device) split into the
bandwidth select and the kernel sums, at nx in --sizes for z in --zs.  With --reference, the reference's recipe (scipy pdist /
cdist, np.median, np.exp) on at most 16 host threads at the sizes in --ref-sizes, in a child process ended after --ref-cap
seconds.  Prints one JSON line.

With --permutations P[,P...], the permutation null of mmd_permutation_test (csrc/mmd_null.hip) instead, with h given: the device
time of the svae_mmd_null launches and of the label bit-packing at each size, the fp64 rate of the label products (2 flops per
pair i < j and permutation; `executed` counts the whole 64 x 64 tiles and 256-column chunks the matrix cores run), and the ratio
to the only other route to the null, P calls of mmd_estimate(Zp[:nx], Zp[nx:], h) on relabelled rows: at most 16 of them are
timed and scaled to P.

    python tools/bench_mmd.py [--reference] [--ref-sizes 4096,8192] [--ref-cap 600] [--sizes 4096,...,65536] [--zs 32,128]
    python tools/bench_mmd.py --permutations 256,1024 --sizes 4096,16384 --zs 32"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd.eval import metrics as M

THREADS = 16


def two_sets(n, d, seed=0):
    g = np.random.default_rng(seed)
    return g.standard_normal(size=(n, d)).astype(np.float32), (g.standard_normal(size=(n, d)) + 0.25).astype(np.float32)


def device_call(x, y):
    info = {}
    h, terms = M._mmd_device(x, y, None, False, info)
    return dict(select_s=round(info["select_s"], 5), sums_s=round(info["sums_s"], 5),
                total_s=round(info["select_s"] + info["sums_s"], 5), h=h, mmd=float(terms[3]))


LOOP_CALLS = 16


def null_call(x, y, P, seed=0):
    """x, y on the device, nx = ny rows"""
    nx, n = x.shape[0], x.shape[0] + y.shape[0]
    keep = {}
    h, _ = M._mmd_device(x, y, None, False, keep=keep)
    Z, hm = keep["Z"], keep["hm"]
    perms = M.mmd_permutations(n, P, seed, x.device)
    M._mmd_null_device(Z, hm, nx, perms[:1])  # this size's first launch
    info = {}
    null = M._mmd_null_device(Z, hm, nx, perms, info)
    calls = min(LOOP_CALLS, P)
    loop = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in range(calls):
        Zp = Z[perms[p]]
        loop.append(M.mmd_estimate(Zp[:nx], Zp[nx:], h))
    torch.cuda.synchronize()
    loop_s = (time.perf_counter() - t0) / calls * P
    nt, chunks = (n + 63) // 64, (P + 255) // 256
    useful = 2.0 * (n * (n - 1) // 2) * P
    executed = 2.0 * 4096 * (nt * (nt + 1) // 2) * chunks * 256
    null_h = null[:calls].cpu().numpy()
    return dict(permutations=P, null_s=round(info["null_s"], 5), pack_s=round(info["pack_s"], 5),
                tflops_useful=round(useful / info["null_s"] / 1e12, 2), tflops_executed=round(executed / info["null_s"] / 1e12, 2),
                loop_s=round(loop_s, 4), loop_calls_timed=calls, speedup=round(loop_s / (info["null_s"] + info["pack_s"]), 1),
                max_diff_to_loop=float(np.abs(null_h - np.array(loop)).max()), h=h)


REF = """
import sys, time
import numpy as np
sys.path.insert(0, {root!r})
from tools.bench_mmd import two_sets
from scipy.spatial.distance import cdist, pdist
X, Y = (a.astype(np.float64) for a in two_sets({n}, {d}))
t0 = time.perf_counter()
xd, yd, xyd = pdist(X), pdist(Y), cdist(X, Y).ravel()
h = np.median(np.concatenate((xd, yd, xyd))) ** 2
v = np.mean(np.exp(-(xd ** 2) / h)) + np.mean(np.exp(-(yd ** 2) / h)) - 2 * np.mean(np.exp(-(xyd ** 2) / h))
print(time.perf_counter() - t0, h, v)
"""


def reference_call(n, d, cap):
    env = dict(os.environ, OMP_NUM_THREADS=str(THREADS), OPENBLAS_NUM_THREADS=str(THREADS), MKL_NUM_THREADS=str(THREADS))
    try:
        r = subprocess.run([sys.executable, "-c", REF.format(root=ROOT, n=n, d=d)], capture_output=True, text=True, timeout=cap, env=env)
    except subprocess.TimeoutExpired:
        return None
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    t, h, v = r.stdout.strip().splitlines()[-1].split()
    return float(t), float(h), float(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192,16384,32768,65536")
    ap.add_argument("--zs", default="32,128")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-sizes", default="4096,8192")
    ap.add_argument("--ref-cap", type=float, default=600.0)
    ap.add_argument("--permutations", default="", help="time the permutation null at these permutation counts instead")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    zs = [int(z) for z in a.zs.split(",") if z]
    ref_sizes = [int(s) for s in a.ref_sizes.split(",") if s] if a.reference else []
    if a.permutations:
        counts = [int(p) for p in a.permutations.split(",") if p]
        null_call(*(torch.from_numpy(t).cuda() for t in two_sets(256, zs[0])), 16)  # warm-up: code objects, torch kernels
        out = dict(device=torch.cuda.get_device_name(0), calls=[])
        for z in zs:
            for n in sizes:
                x, y = (torch.from_numpy(t).cuda() for t in two_sets(n, z))
                for P in counts:
                    row = dict(nx=n, ny=n, z=z, **null_call(x, y, P))
                    out["calls"].append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
        print(json.dumps(out))
        return
    device_call(*(torch.from_numpy(t).cuda() for t in two_sets(min(sizes), zs[0])))  # warm-up: code objects, torch kernels
    out = dict(device=torch.cuda.get_device_name(0), calls=[])
    for z in zs:
        for n in sizes:
            x, y = (torch.from_numpy(t).cuda() for t in two_sets(n, z))
            row = dict(nx=n, ny=n, z=z, **device_call(x, y))
            if n in ref_sizes:
                ref = reference_call(n, z, a.ref_cap)
                row["reference_s"] = None if ref is None else round(ref[0], 3)
                if ref is not None:
                    row["speedup"] = round(ref[0] / row["total_s"], 1)
                    row["h_equal"] = ref[1] == row["h"]
                    row["mmd_diff"] = abs(ref[2] - row["mmd"])
            out["calls"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
