"""Cost of placing new rows on a fitted t-SNE map (scrubvae_amd/eval/embed_transform.py, csrc/tsne.hip, csrc/knn.hip) on the
Gaussian blobs of tools/bench_knn.py (rows of d features around 25 centres).

1. The pair rate of svae_tsne_cross_repulsion, in Gpairs/s, at the (m, n) of --pairs, and of svae_tsne_repulsion (the square kernel
   it was made from) at --square rows, in the same run: --reps launches each after a warm-up, synchronised host clock around them.
2. The whole transform at the (m, n) of --sizes: a map fitted on n rows with --map-iter iterations, then m other rows placed with
   the default optimiser; the time split into kNN, search, repulsion and step (synchronised host clock around every launch), and
   the time of an untimed call, which is what a user waits for.
3. Quality: sklearn's trustworthiness (5 neighbours) of the reference rows and the placed rows together on a subsample of
   --trust-rows rows, next to that of the reference rows alone, and the share of placed rows whose DensityMap region equals that of
   their nearest reference latent.
4. With --reference: the numpy restatement of tests/transform_checks.py at --ref-size (m, n), with 16 host threads.
Prints one JSON line.

    python tools/bench_transform.py [--reference] [--pairs 100000x20000,1000000x20000,100000x100000] [--sizes 100000x20000,1000000x20000,100000x100000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd import _lib
from scrubvae_amd.eval import DensityMap, embed, embed_transform, neighbors
from tools.bench_knn import blobs

THREADS = 16


def pairs_of(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def cross_rate(m, n, reps):
    g = torch.Generator(device="cuda").manual_seed(m + n)
    Yref = 30.0 * torch.randn(n, 2, dtype=torch.float64, device="cuda", generator=g)
    Yq = 30.0 * torch.randn(m, 2, dtype=torch.float64, device="cuda", generator=g)
    rep = embed_transform._CrossRepulsion(m, Yref)
    s = timed(lambda: rep(Yq), reps)
    return dict(m=m, n=n, chunks=embed_transform._PLACE_LAST["chunks"], ms=round(1e3 * s, 4), gpairs_per_s=round(float(m) * n / s / 1e9, 1))


def square_rate(n, reps):
    g = torch.Generator(device="cuda").manual_seed(n)
    Y = 30.0 * torch.randn(n, 2, dtype=torch.float64, device="cuda", generator=g)
    rep = embed._Repulsion(n, Y.device)
    s = timed(lambda: rep(Y), reps)
    return dict(n=n, chunks=embed._TSNE_LAST["chunks"], ms=round(1e3 * s, 4), gpairs_per_s=round(float(n) * n / s / 1e9, 1))


def trust(x, emb, rows):
    from sklearn.manifold import trustworthiness
    pick = np.random.default_rng(0).choice(len(x), size=min(rows, len(x)), replace=False)
    return round(float(trustworthiness(x[pick], emb[pick], n_neighbors=5)), 5)


def whole(m, n, d, map_iter, trust_rows, maps):
    x = blobs(n + m, d)
    ref, new = torch.from_numpy(x[:n]).cuda(), torch.from_numpy(x[n:]).cuda()
    if n not in maps:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        maps[n] = (embed.TSNE(max_iter=map_iter).fit(ref).embedding_, time.perf_counter() - t0)
    emb, fit_s = maps[n]
    tmap = embed_transform.TSNEMap(ref, emb)
    info = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Yt = tmap.transform(new, info=info)
    timed_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Y = tmap.transform(new)
    plain_s = time.perf_counter() - t0
    its = info["iterations"]
    row = dict(m=m, n=n, map_fit_s=round(fit_s, 3), batches=info["batches"], knn_s=round(info["knn_s"], 4), search_s=round(info["search_s"], 4),
               repulsion_s=round(info["repulsion_s"], 4), step_s=round(info["step_s"], 4), transform_timed_s=round(timed_s, 4),
               transform_s=round(plain_s, 4), repulsion_gpairs_per_s=round(float(m) * n * its / info["repulsion_s"] / 1e9, 1),
               same_bytes=bool(np.array_equal(Y, Yt)), kl_mean=round(float(tmap.kl_rows_.mean()), 5),
               grad_norm_max=float(tmap.grad_norm_rows_.max()))
    # quality: the placed rows among the reference rows, and the density regions they fall in
    xs = x.astype(np.float64)
    pick = np.random.default_rng(1).choice(m, size=min(m, n), replace=False)       # as many placed rows as reference rows at most
    both_x, both_y = np.concatenate([xs[:n], xs[n:][pick]]), np.concatenate([emb, Y[pick]])
    row.update(trust_reference=trust(xs[:n], emb, trust_rows), trust_reference_and_placed=trust(both_x, both_y, trust_rows))
    dm = DensityMap().fit(emb)
    nearest = neighbors.kneighbors_cross(ref, new, 1, return_distance=False)[:, 0]
    placed = dm.predict(Y)
    row.update(regions=int(len(dm.region_counts_)), same_region_as_nearest_reference=round(float((placed == dm.labels_[nearest]).mean()), 5),
               placed_in_no_region=round(float((placed < 0).mean()), 5))
    return row


def reference(m, n, d):
    from tests import transform_checks as XC
    x = blobs(n + m, d).astype(np.float64)
    emb = embed.TSNE(max_iter=500).fit(x[:n]).embedding_
    t0 = time.perf_counter()
    out = XC.transform(x[:n], emb, x[n:], 30.0, **XC.DEFAULTS)
    host_s = time.perf_counter() - t0
    tmap = embed_transform.TSNEMap(x[:n], emb)
    tmap.transform(x[n:])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Y = tmap.transform(x[n:])
    dev_s = time.perf_counter() - t0
    return dict(m=m, n=n, numpy_s=round(host_s, 3), device_s=round(dev_s, 4), ratio=round(host_s / dev_s, 1),
                max_abs_difference=float(np.abs(Y - out.Y).max()), kl_mean_numpy=round(float(out.kl.mean()), 6),
                kl_mean_device=round(float(tmap.kl_rows_.mean()), 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="100000x20000,1000000x20000,100000x100000")
    ap.add_argument("--square", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="100000x20000,1000000x20000,100000x100000")
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--map-iter", type=int, default=500)
    ap.add_argument("--trust-rows", type=int, default=5000)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--ref-size", default="2000x2000")
    a = ap.parse_args()
    torch.set_num_threads(THREADS)
    _lib.lib()
    out = dict(device=torch.cuda.get_device_name(0), d=a.d, reps=a.reps, square=None, cross=[], transforms=[], reference=None)
    if a.square:
        square_rate(2000, 2)                                  # warm-up: code objects
        out["square"] = square_rate(a.square, a.reps)
        print(json.dumps(out["square"]), file=sys.stderr, flush=True)
    for m, n in pairs_of(a.pairs):
        out["cross"].append(cross_rate(m, n, a.reps))
        print(json.dumps(out["cross"][-1]), file=sys.stderr, flush=True)
    if a.square:
        again = square_rate(a.square, a.reps)                 # once more after the cross launches: the spread of one box
        out["square"]["gpairs_per_s_again"] = again["gpairs_per_s"]
    maps = {}
    for m, n in pairs_of(a.sizes):
        out["transforms"].append(whole(m, n, a.d, a.map_iter, a.trust_rows, maps))
        print(json.dumps(out["transforms"][-1]), file=sys.stderr, flush=True)
    if a.reference:
        out["reference"] = reference(*pairs_of(a.ref_size)[0], a.d)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
