"""Cost of KMeans fits (scrubvae_amd/eval/cluster.py, csrc/kmeans.hip) against sklearn.cluster.KMeans(algorithm="lloyd", n_init=1)
from the same init array (rows of the data drawn once), at n in {10^5, 10^6}, d = 32, K in {25, 100}, on planted data.  The device
times are a synchronised host clock after a warm-up fit; seconds per Lloyd iteration are the difference of two fits with
different max_iter (tol = 0) over the difference of their n_iter_, which leaves out the centring and the final assignment.  An
iteration reads the centred fp64 rows A [n][pad16(d + 1)] twice (assignment, update); that is set against the HBM streaming rate
(--hbm-tbs, 6.3 TB/s as measured with a float4 copy).  sklearn runs on at most 16 host threads on the same rows as fp64 (the
device's arithmetic); labels and n_iter_ are compared.  Prints one JSON line.

    python tools/bench_kmeans.py [--sizes 100000,1000000] [--ks 25,100] [--no-reference] [--hbm-tbs 6.3]"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scrubvae_amd import ops
from scrubvae_amd.eval import KMeans

THREADS, D = 16, 32


def planted(n, d, K, seed=0):
    g = np.random.default_rng(seed)
    lab = g.integers(0, K, n)
    x = g.normal(size=(K, d))[lab] * 3.0 + g.standard_normal(size=(n, d), dtype=np.float32) + 20.0
    return x.astype(np.float32)


def device_fit(x, init, max_iter, tol):
    m = KMeans(len(init), init=init, n_init=1, max_iter=max_iter, tol=tol)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(x)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--ks", default="25,100")
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    args = ap.parse_args()
    out = {"d": D, "device": {}, "reference": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        for K in (int(s) for s in args.ks.split(",")):
            key = f"n{n}_K{K}"
            x_host = planted(n, D, K)
            init = x_host[np.random.default_rng(1).choice(n, K, replace=False)].astype(np.float64)
            x = torch.from_numpy(x_host).cuda()
            device_fit(x, init, 2, 0.0)  # warm-up
            t, m = device_fit(x, init, 300, 1e-4)
            t_a, m_a = device_fit(x, init, 2, 0.0)
            t_b, m_b = device_fit(x, init, 12, 0.0)
            row = {"fit_s": round(t, 4), "n_iter": m.n_iter_, "inertia": m.inertia_}
            if m_b.n_iter_ > m_a.n_iter_:
                per = (t_b - t_a) / (m_b.n_iter_ - m_a.n_iter_)
                a_bytes = 2 * n * ops.pad16(D + 1) * 8
                row.update(s_per_iter=round(per, 6), a_bytes_per_iter=a_bytes, a_tbs=round(a_bytes / per / 1e12, 3),
                           hbm_fraction=round(a_bytes / per / 1e12 / args.hbm_tbs, 3))
            out["device"][key] = row
            print(key, row, file=sys.stderr, flush=True)
            if not args.no_reference:
                from sklearn.cluster import KMeans as SkKMeans
                from threadpoolctl import threadpool_limits
                with threadpool_limits(THREADS):
                    t0 = time.perf_counter()
                    ref = SkKMeans(K, init=init, n_init=1, algorithm="lloyd").fit(x_host.astype(np.float64))
                    t_ref = time.perf_counter() - t0
                same = bool(np.array_equal(ref.labels_, m.labels_))
                out["reference"][key] = {"fit_s": round(t_ref, 3), "n_iter": int(ref.n_iter_), "s_per_iter": round(t_ref / ref.n_iter_, 4),
                                         "labels_equal": same, "rows_differing": int((ref.labels_ != m.labels_).sum()),
                                         "n_iter_equal": bool(ref.n_iter_ == m.n_iter_)}
                print(key, out["reference"][key], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
