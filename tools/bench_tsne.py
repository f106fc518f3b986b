"""Cost of TSNE (scrubvae_amd/eval/embed.py, csrc/tsne.hip) on the Gaussian blobs of tools/bench_knn.py (n rows of d features
around 25 centres): the time of one fit at n in --sizes with --max-iter iterations, split into graph + search (kNN, perplexity
search, symmetrisation), repulsion and step (synchronised host clock around every launch, after a warm-up fit at 2 000 rows, rows
already on the device), the time per iteration, the rate of pairs the repulsion stands for (n^2 per iteration), and the time of an
untimed fit (no synchronisation inside the loop), which is what a user waits for.  With --reference, at the sizes in --ref-sizes,
sklearn.manifold.TSNE(method="barnes_hut", n_jobs=16) with the same max_iter in a child process ended after --ref-cap seconds, and
sklearn's trustworthiness (5 neighbours) of both embeddings on a subsample of --trust-rows rows.  Prints one JSON line.

    python tools/bench_tsne.py [--reference] [--ref-sizes 20000] [--ref-cap 400] [--sizes 20000,100000] [--d 32] [--max-iter 1000]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd.eval import embed
from tools.bench_knn import blobs

THREADS = 16


def device_fit(x, max_iter):
    """x on the device -> (row of timings, embedding)"""
    info = {}
    est = embed.TSNE(max_iter=max_iter)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    est.fit(x, info=info)
    timed = time.perf_counter() - t0
    n, its = x.shape[0], info["iterations"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plain = embed.TSNE(max_iter=max_iter).fit(x)
    fit_s = time.perf_counter() - t0
    row = dict(iterations=its, chunks=embed._TSNE_LAST["chunks"], graph_s=round(info["graph_s"], 4), repulsion_s=round(info["repulsion_s"], 4),
               step_s=round(info["step_s"], 4), fit_timed_s=round(timed, 4), fit_s=round(fit_s, 4),
               repulsion_ms_per_iter=round(1e3 * info["repulsion_s"] / its, 4), step_ms_per_iter=round(1e3 * info["step_s"] / its, 4),
               gpairs_per_s=round(float(n) * n * its / info["repulsion_s"] / 1e9, 1), kl=round(plain.kl_divergence_, 5),
               same_bytes=bool(np.array_equal(plain.embedding_, est.embedding_)))
    return row, plain.embedding_


REF = """
import sys, time
import numpy as np
sys.path.insert(0, {root!r})
from tools.bench_knn import blobs
from sklearn.manifold import TSNE
x = blobs({n}, {d}).astype(np.float64)
t0 = time.perf_counter()
est = TSNE(method="barnes_hut", n_jobs={threads}, max_iter={max_iter}, random_state=0)
emb = est.fit_transform(x)
print(time.perf_counter() - t0, est.kl_divergence_, est.n_iter_)
np.save({out!r}, emb)
"""


def reference_fit(n, d, max_iter, cap):
    env = dict(os.environ, OMP_NUM_THREADS=str(THREADS), OPENBLAS_NUM_THREADS=str(THREADS), MKL_NUM_THREADS=str(THREADS))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "emb.npy")
        try:
            r = subprocess.run([sys.executable, "-c", REF.format(root=ROOT, n=n, d=d, threads=THREADS, max_iter=max_iter, out=out)],
                               capture_output=True, text=True, timeout=cap, env=env)
        except subprocess.TimeoutExpired:
            return None
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        t, kl, its = r.stdout.strip().splitlines()[-1].split()
        return float(t), float(kl), int(its), np.load(out)


def trust(x, emb, rows):
    from sklearn.manifold import trustworthiness
    pick = np.random.default_rng(0).choice(len(x), size=min(rows, len(x)), replace=False)
    return round(float(trustworthiness(x[pick], emb[pick], n_neighbors=5)), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-sizes", default="20000")
    ap.add_argument("--ref-cap", type=float, default=400.0)
    ap.add_argument("--trust-rows", type=int, default=5000)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    ref_sizes = [int(s) for s in a.ref_sizes.split(",") if s] if a.reference else []
    torch.set_num_threads(THREADS)
    device_fit(torch.from_numpy(blobs(2000, a.d)).cuda(), 250)  # warm-up: code objects, torch kernels
    out = dict(device=torch.cuda.get_device_name(0), d=a.d, max_iter=a.max_iter, fits=[], reference_cap_s=a.ref_cap if a.reference else None,
               reference_left_out=[n for n in sizes if n not in ref_sizes])
    for n in sizes:
        x = blobs(n, a.d)
        row, emb = device_fit(torch.from_numpy(x).cuda(), a.max_iter)
        row = dict(n=n, **row)
        if n in ref_sizes:
            row["trust_device"] = trust(x.astype(np.float64), emb, a.trust_rows)
            ref = reference_fit(n, a.d, a.max_iter, a.ref_cap)
            row["sklearn_barnes_hut_s"] = None if ref is None else round(ref[0], 2)   # None: ended at the cap
            if ref is not None:
                row.update(sklearn_kl=round(ref[1], 5), sklearn_n_iter=ref[2], speedup=round(ref[0] / row["fit_s"], 1),
                           trust_sklearn=trust(x.astype(np.float64), ref[3], a.trust_rows))
        out["fits"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
