"""Cost of kneighbors (scrubvae_amd/eval/neighbors.py, csrc/knn.hip) on n rows of d features around 25 centres: the device time of
the svae_knn call (synchronised host clock, after a warm-up call at the smallest size, inputs already on the device) at n in
--sizes, d in --dims, k in --ks, with the rate of distances it stands for (n^2 pairs per call).  Next to it, on the same rows,
svae_hdb_core at k + 1: the project's other selection kernel, which finds the k-th distance alone in up to 8 passes over the
distances.  With --reference, sklearn.neighbors.NearestNeighbors with kd_tree and with brute on at most 16 host threads at the sizes
in --ref-sizes, each in a child process ended after --ref-cap seconds; what was left out or cut off is listed.  Prints one JSON line.

    python tools/bench_knn.py [--reference] [--ref-sizes 20000] [--ref-cap 60] [--sizes 20000,100000] [--dims 32,128] [--ks 15,64]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd import _lib, ops
from scrubvae_amd.eval import neighbors as NB
from scrubvae_amd.eval._device import _clock

THREADS = 16


def blobs(n, d, seed=0):
    g = np.random.default_rng(seed)
    y = g.integers(0, 25, n)
    mu = 2 * g.normal(size=(25, d))
    return (mu[y] + g.normal(size=(n, d))).astype(np.float32)


def device_call(x, k):
    """x on the device"""
    rows, k, _ = NB._knn_check(x, k)
    info = {}
    dist, idx = NB._knn_device(rows, k, None, info)
    n, d = rows.shape
    t = info["knn_s"]
    # svae_hdb_core at k + 1 (the row itself is its first neighbour there)
    core = torch.empty(n, dtype=torch.float64, device=rows.device)
    t0 = _clock(rows.device)
    _lib.check(_lib.lib().svae_hdb_core(rows.data_ptr(), d, d, n, k + 1, core.data_ptr(), ops._stream()), "hdb_core")
    t_core = _clock(rows.device) - t0
    return dict(chunks=NB._KNN_LAST["chunks"], knn_s=round(t, 5), gpairs_per_s=round(float(n) * n / t / 1e9, 1),
                hdb_core_s=round(t_core, 5), hdb_core_over_knn=round(t_core / t, 2),
                kth_equal=bool(torch.equal(dist[:, k - 1], core)), checksum=int(idx.sum()))


REF = """
import sys, time
import numpy as np
sys.path.insert(0, {root!r})
from tools.bench_knn import blobs
from sklearn.neighbors import NearestNeighbors
x = blobs({n}, {d}).astype(np.float64)
t0 = time.perf_counter()
dist, idx = NearestNeighbors(n_neighbors={k}, algorithm={algo!r}, n_jobs={threads}).fit(x).kneighbors()
print(time.perf_counter() - t0, int(idx.sum()))
"""


def reference_call(n, d, k, algo, cap):
    env = dict(os.environ, OMP_NUM_THREADS=str(THREADS), OPENBLAS_NUM_THREADS=str(THREADS), MKL_NUM_THREADS=str(THREADS))
    try:
        r = subprocess.run([sys.executable, "-c", REF.format(root=ROOT, n=n, d=d, k=k, algo=algo, threads=THREADS)], capture_output=True,
                           text=True, timeout=cap, env=env)
    except subprocess.TimeoutExpired:
        return None
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    t, v = r.stdout.strip().splitlines()[-1].split()
    return float(t), int(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--dims", default="32,128")
    ap.add_argument("--ks", default="15,64")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-sizes", default="20000")
    ap.add_argument("--ref-cap", type=float, default=60.0)
    a = ap.parse_args()
    sizes, dims, ks = ([int(v) for v in s.split(",") if v] for s in (a.sizes, a.dims, a.ks))
    ref_sizes = [int(s) for s in a.ref_sizes.split(",") if s] if a.reference else []
    device_call(torch.from_numpy(blobs(min(sizes), min(dims))).cuda(), min(ks))  # warm-up: code objects, torch kernels
    out = dict(device=torch.cuda.get_device_name(0), calls=[], reference_cap_s=a.ref_cap if a.reference else None,
               reference_left_out=[n for n in sizes if n not in ref_sizes])
    for n in sizes:
        for d in dims:
            x = torch.from_numpy(blobs(n, d)).cuda()
            for k in ks:
                row = dict(n=n, d=d, k=k, **device_call(x, k))
                if n in ref_sizes:
                    for algo in ("kd_tree", "brute"):
                        ref = reference_call(n, d, k, algo, a.ref_cap)
                        row[f"sklearn_{algo}_s"] = None if ref is None else round(ref[0], 3)   # None: ended at the cap
                        if ref is not None:
                            row[f"speedup_{algo}"] = round(ref[0] / row["knn_s"], 1)
                            row[f"same_indices_{algo}"] = ref[1] == row["checksum"]   # brute's GEMM distances may order near-ties differently
                out["calls"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
