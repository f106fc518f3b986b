"""Cost of HDBSCAN fits (scrubvae_amd/eval/hdbscan.py, csrc/hdbscan.hip) with min_cluster_size=500 on planted blobs (25 blobs,
z features): the device fit time (synchronised host clock, after a warm-up fit at the smallest size) split into core distances,
Boruvka rounds (and their count) and the host tree, at n in --sizes for z in --zs, plus --big rows at z = 32.  With --reference,
sklearn's HDBSCAN (default algorithm) at the same settings on at most 16 host threads, in a child process ended after --ref-cap
seconds (the size is then reported as not finished and larger ones are skipped).  Prints one JSON line.

    python tools/bench_hdbscan.py [--reference] [--ref-cap 600] [--sizes 32768,65536,131072] [--zs 32,128] [--big 1048576]"""
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

from scrubvae_amd.eval import HDBSCAN

THREADS, BLOBS, MCS = 16, 25, 500


def planted(n, d, seed=0):
    g = np.random.default_rng(seed)
    centers = g.uniform(-6.0, 6.0, size=(BLOBS, d))
    lab = g.integers(0, BLOBS, n)
    return (centers[lab] + 0.5 * g.standard_normal(size=(n, d))).astype(np.float32)


def device_fit(x):
    m = HDBSCAN(min_cluster_size=MCS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.fit(x)
    t = time.perf_counter() - t0
    tm = m._timings_
    return dict(fit_s=round(t, 4), core_s=round(tm["core_s"], 4), boruvka_s=round(tm["boruvka_s"], 4), rounds=tm["rounds"],
                tree_s=round(tm["tree_s"], 4), clusters=int(m.labels_.max()) + 1, noise=float((m.labels_ < 0).mean()))


REF = """
import os, sys, time
import numpy as np
sys.path.insert(0, {root!r})
from tools.bench_hdbscan import planted
from sklearn.cluster import HDBSCAN
x = planted({n}, {d}).astype(np.float64)
t0 = time.perf_counter()
HDBSCAN(min_cluster_size={mcs}).fit(x)
print(time.perf_counter() - t0)
"""


def reference_fit(n, d, cap):
    env = dict(os.environ, OMP_NUM_THREADS=str(THREADS), OPENBLAS_NUM_THREADS=str(THREADS), MKL_NUM_THREADS=str(THREADS))
    try:
        r = subprocess.run([sys.executable, "-c", REF.format(root=ROOT, n=n, d=d, mcs=MCS)], capture_output=True, text=True,
                           timeout=cap, env=env)
    except subprocess.TimeoutExpired:
        return None
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return float(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32768,65536,131072")
    ap.add_argument("--zs", default="32,128")
    ap.add_argument("--big", default="1048576", help="extra sizes at z = 32 ('' for none)")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-cap", type=float, default=600.0)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    zs = [int(z) for z in a.zs.split(",") if z]
    runs = [(n, z) for z in zs for n in sizes] + [(int(s), 32) for s in a.big.split(",") if s]
    device_fit(torch.from_numpy(planted(min(sizes), zs[0])).cuda())  # warm-up: code objects, torch kernels
    out = dict(device=torch.cuda.get_device_name(0), min_cluster_size=MCS, fits=[])
    ref_done = {}
    for n, z in runs:
        x = torch.from_numpy(planted(n, z)).cuda()
        row = dict(n=n, z=z, **device_fit(x))
        if a.reference and z == 32 and ref_done.get(z, True):
            t = reference_fit(n, z, a.ref_cap)
            row["sklearn_s"] = None if t is None else round(t, 2)
            if t is None:
                ref_done[z] = False
            else:
                row["speedup"] = round(t / row["fit_s"], 1)
        out["fits"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
