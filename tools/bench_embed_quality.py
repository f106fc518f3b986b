"""Cost of the embedding scores (scrubvae_amd/eval/embed_quality.py, csrc/rank.hip) on n rows of d features around 25 centres
(tools/bench_knn.py's blobs) and a 2-D embedding of them, inputs already on the device, synchronised host clock, after a warm-up
call at the smallest size:

  scores     trustworthiness(X, Y, n_neighbors=5) and embedding_quality(X, Y, max_neighbors=30): the whole calls, and of the
             second one kNN search, one rank pass and one curve pass, each timed in a run of its own.  Y is X's first two
             features plus noise (a well-ordered embedding: most candidates lie above a row's largest threshold and cost no LDS
             traffic) and, as the worst case, a Y drawn on its own (most candidates fall below it: a binary search and an LDS atomic
             each).  At the sizes in --ref-sizes also sklearn.manifold.trustworthiness on the same host arrays (at most 16 host
             threads), with the difference of the two values; sklearn stores n x n distances and their argsort, so it is left out
             beyond those sizes.
  tsne       (--tsne N) the quality curves of eval.TSNE (exact gradient) next to sklearn's Barnes-Hut TSNE on the same N rows,
             both with --max-iter iterations.

Prints one JSON line.

    python tools/bench_embed_quality.py [--sizes 2000,10000,20000,100000] [--ref-sizes 2000,10000] [--d 32] [--tsne 5000]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd.eval import embed_quality as EQ
from scrubvae_amd.eval._device import _clock
from scrubvae_amd.eval.neighbors import _knn_device
from tools.bench_knn import blobs

THREADS = 16
K_ONE, K_MAX = 5, 30


def timed(dev, fn):
    t0 = _clock(dev)
    out = fn()
    return out, _clock(dev) - t0


def scores(x, y, name, reference):
    """x [n, d], y [n, 2] float64 numpy -> one row of timings"""
    X, Y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    dev, n = X.device, len(x)
    t, trust_s = timed(dev, lambda: EQ.trustworthiness(X, Y, n_neighbors=K_ONE))
    q, quality_s = timed(dev, lambda: EQ.embedding_quality(X, Y, max_neighbors=K_MAX))
    (_, idx), knn_s = timed(dev, lambda: _knn_device(Y, K_MAX, None))
    rank, ranks_s = timed(dev, lambda: EQ._ranks_device(X, idx))
    _, curves_s = timed(dev, lambda: EQ._curves_device(rank))
    row = dict(n=n, embedding=name, trustworthiness_s=round(trust_s, 5), embedding_quality_s=round(quality_s, 5), knn_2d_s=round(knn_s, 5),
               rank_pass_s=round(ranks_s, 5), curve_pass_s=round(curves_s, 5), rank_gpairs_per_s=round(float(n) * n / ranks_s / 1e9, 1),
               chunks=EQ._RANK_LAST["chunks"], trustworthiness=t, continuity=float(q.continuity[K_ONE - 1]),
               q_nx_30=round(float(q.q_nx[-1]), 5), auc_r_nx=round(q.auc_r_nx, 5), same_value=bool(q.trustworthiness[K_ONE - 1] == t))
    if reference:
        from sklearn.manifold import trustworthiness
        t0 = time.perf_counter()
        want = trustworthiness(x, y, n_neighbors=K_ONE)
        ref = time.perf_counter() - t0
        row.update(sklearn_s=round(ref, 3), speedup=round(ref / trust_s, 1), difference=float(t - want))
    return row


def curves(q):
    pick = [k for k in (1, 5, 10, 30) if k <= len(q.k)]
    return dict(trustworthiness={k: round(float(q.trustworthiness[k - 1]), 5) for k in pick},
                continuity={k: round(float(q.continuity[k - 1]), 5) for k in pick},
                q_nx={k: round(float(q.q_nx[k - 1]), 5) for k in pick}, r_nx={k: round(float(q.r_nx[k - 1]), 5) for k in pick},
                auc_r_nx=round(q.auc_r_nx, 5))


def tsne_pair(n, d, max_iter):
    """the same rows through eval.TSNE and sklearn's Barnes-Hut TSNE, scored alike"""
    from sklearn.manifold import TSNE as Theirs

    from scrubvae_amd.eval import TSNE
    x = blobs(n, d).astype(np.float64)
    t0 = time.perf_counter()
    ours = TSNE(max_iter=max_iter, random_state=0).fit_transform(x)
    ours_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    theirs = Theirs(method="barnes_hut", n_jobs=THREADS, max_iter=max_iter, random_state=0).fit_transform(x)
    theirs_s = time.perf_counter() - t0
    return dict(n=n, d=d, max_iter=max_iter, exact_gradient=dict(fit_s=round(ours_s, 2), **curves(EQ.embedding_quality(x, ours, max_neighbors=K_MAX))),
                barnes_hut=dict(fit_s=round(theirs_s, 2), **curves(EQ.embedding_quality(x, theirs.astype(np.float64), max_neighbors=K_MAX))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000,20000,100000")
    ap.add_argument("--ref-sizes", default="2000,10000")
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--tsne", type=int, default=0)
    ap.add_argument("--max-iter", type=int, default=1000)
    a = ap.parse_args()
    torch.set_num_threads(min(torch.get_num_threads(), THREADS))
    sizes = [int(s) for s in a.sizes.split(",") if s]
    ref_sizes = [int(s) for s in a.ref_sizes.split(",") if s]
    x = blobs(min(sizes), a.d).astype(np.float64)
    EQ.embedding_quality(x, x[:, :2].copy(), max_neighbors=K_MAX, rows_at=K_ONE)     # warm-up: code objects, torch kernels
    EQ.trustworthiness(x, x[:, :2].copy(), n_neighbors=K_ONE)
    out = dict(device=torch.cuda.get_device_name(0), d=a.d, n_neighbors=K_ONE, max_neighbors=K_MAX, scores=[])
    for n in sizes:
        x = blobs(n, a.d).astype(np.float64)
        g = np.random.default_rng(n)
        for name, y in (("first two features + noise", x[:, :2] + 0.5 * g.standard_normal((n, 2))), ("random", g.standard_normal((n, 2)))):
            row = scores(x, y, name, n in ref_sizes)
            out["scores"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    if a.tsne:
        out["tsne"] = tsne_pair(a.tsne, a.d, a.max_iter)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
