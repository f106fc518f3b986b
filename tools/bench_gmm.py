"""Cost of GaussianMixture fits (scrubvae_amd/eval/cluster.py, csrc/gmm.hip): the device fit time (synchronised host clock, after
a warm-up fit) and seconds per EM iteration at n in {2^17, 10^6}, z in {32, 128}, K = 25, full and diag covariance, on planted
data.  With --reference, sklearn's GaussianMixture at the same settings on at most 16 host threads, with max_iter capped
(--ref-iters, tol = 0) and reported per iteration; --ref-max-rows skips sizes above it.  Prints one JSON line.

    python tools/bench_gmm.py [--reference] [--ref-iters 3] [--ref-max-rows 1000000] [--sizes 131072,1000000] [--zs 32,128]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scrubvae_amd.eval import GaussianMixture

THREADS, K = 16, 25


def planted(n, d, seed=0):
    g = np.random.default_rng(seed)
    lab = g.integers(0, K, n)
    x = g.normal(size=(K, d))[lab] * 3.0 + g.standard_normal(size=(n, d), dtype=np.float32) + 20.0
    return x.astype(np.float32)


def device_fit(x, cov, max_iter):
    m = GaussianMixture(K, covariance_type=cov, max_iter=max_iter, random_state=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(x)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, m.n_iter_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-iters", type=int, default=3)
    ap.add_argument("--ref-max-rows", type=int, default=1_000_000)
    ap.add_argument("--sizes", default="131072,1000000")
    ap.add_argument("--zs", default="32,128")
    ap.add_argument("--max-iter", type=int, default=100)
    args = ap.parse_args()
    out = {"K": K, "device": {}, "reference": {}}
    sizes = [int(s) for s in args.sizes.split(",")]
    zs = [int(s) for s in args.zs.split(",")]
    for n in sizes:
        for d in zs:
            x = torch.from_numpy(planted(n, d)).cuda()
            for cov in ("full", "diag"):
                device_fit(x, cov, 2)  # warm-up
                t, it = device_fit(x, cov, args.max_iter)
                t1, _ = device_fit(x, cov, 1)  # seeding + one iteration + the final labels
                t2, _ = device_fit(x, cov, 2)
                key = f"n{n}_z{d}_{cov}"
                out["device"][key] = {"fit_s": round(t, 4), "n_iter": it, "s_per_iter": round(t2 - t1, 5),
                                      "s_seed_and_labels": round(2 * t1 - t2, 4)}
                print(key, out["device"][key], file=sys.stderr, flush=True)
    if args.reference:
        from threadpoolctl import threadpool_limits
        from sklearn.mixture import GaussianMixture as SkGM
        with threadpool_limits(THREADS):
            for n in sizes:
                if n > args.ref_max_rows:
                    continue
                for d in zs:
                    x = planted(n, d)
                    for cov in ("full", "diag"):
                        m = SkGM(K, covariance_type=cov, max_iter=args.ref_iters, tol=0.0, init_params="k-means++", random_state=0)
                        import warnings
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            t0 = time.perf_counter()
                            m.fit(x)
                            t = time.perf_counter() - t0
                        key = f"n{n}_z{d}_{cov}"
                        out["reference"][key] = {"s_per_iter_incl_init": round(t / args.ref_iters, 3), "iters": args.ref_iters}
                        print(key, out["reference"][key], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
