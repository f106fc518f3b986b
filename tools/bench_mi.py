"""Cost of the kNN mutual-information estimate (scrubvae_amd/eval/mutual_info.py, csrc/mi.hip) on n rows of d features around 25
centres, k = 3, inputs already on the device, synchronised host clock, after a warm-up call at the smallest size:

  estimate     mutual_information(z, y) with a real y of q = 3 columns and with the 25 centre labels: the whole call, and of it
               the radius pass, the count pass and the psi sums, each timed in a second run with a synchronisation between them
  scores       latent_mi_scores(z, y) against sklearn's mutual_info_regression / mutual_info_classif on the same host arrays
               (--reference; sklearn on at most 16 host threads), with the largest difference of a score
  permutation  mutual_information_permutation_test at P = --perms against one mutual_information call timed and scaled by P
  buffer       (host, numpy, --buffer) the share of a row tile's candidates that reach the LDS buffer of mi_radius_kernel, over
               the first 4 column tiles and over the rest, by replaying the kernel's append and cut rule on rows 0..63

Prints one JSON line.

    python tools/bench_mi.py [--sizes 5000,20000,50000] [--dim 32] [--perms 200] [--reference] [--buffer]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from scrubvae_amd.eval import mutual_info as MI
from scrubvae_amd.eval._device import _clock

THREADS = 16
K = 3


def rows(n, d, seed=0):
    """(z [n, d] float32 around 25 centres, y [n, 3] depending on z's first columns, the centre labels [n])"""
    g = np.random.default_rng(seed)
    lab = g.integers(0, 25, n)
    mu = 2 * g.normal(size=(25, d))
    z = (mu[lab] + g.normal(size=(n, d))).astype(np.float32)
    y = (0.8 * z[:, :3] + 0.6 * g.normal(size=(n, 3))).astype(np.float32)
    return z, y, lab.astype(np.int64)


def estimate(z, y):
    """z on the device -> the times of one estimate"""
    dev = z.device
    t0 = _clock(dev)
    value = MI.mutual_information(z, y, n_neighbors=K)
    whole = _clock(dev) - t0
    c = MI._mi_check(z, y, K)
    with torch.cuda.device(dev):
        run = MI._MiRun(c, dev)
        out = torch.zeros(2, dtype=torch.float64, device=dev)
        lib, st = run.lib, run.st
        yp, lp, kp = (None if t is None else t.data_ptr() for t in (run.Y, run.lab, run.kk))
        nyp = None if run.ny is None else run.ny.data_ptr()
        t0 = _clock(dev)
        MI.check(lib.svae_mi_radius(run.Z.data_ptr(), run.ld, run.ld, run.n, yp, run.q, lp, kp, K, run.work.data_ptr(), run.rho2.data_ptr(), st))
        t1 = _clock(dev)
        MI.check(lib.svae_mi_counts(run.Z.data_ptr(), run.ld, run.ld, run.n, yp, run.q, run.rho2.data_ptr(), run.nz.data_ptr(), nyp, st))
        t2 = _clock(dev)
        MI.check(lib.svae_mi_psi_sums(run.nz.data_ptr(), nyp, run.n, out.data_ptr(), st))
        t3 = _clock(dev)
        again = float(run.close(out.cpu().numpy()))
    n = run.n
    return dict(value=round(value, 6), same_bits=again == value, whole_s=round(whole, 5), radius_s=round(t1 - t0, 5),
                counts_s=round(t2 - t1, 5), psi_sums_s=round(t3 - t2, 6), radius_gpairs_per_s=round(float(n) * n / (t1 - t0) / 1e9, 1),
                counts_gpairs_per_s=round(float(n) * n / (t2 - t1) / 1e9, 1))


def scores(z, y, discrete, reference):
    zd = torch.from_numpy(z).cuda()
    t0 = _clock(zd.device)
    got = MI.latent_mi_scores(zd, y, discrete_target=discrete, n_neighbors=K, random_state=0)
    row = dict(scores_s=round(_clock(zd.device) - t0, 4), largest_score=round(float(got.max()), 4))
    if reference:
        from sklearn.feature_selection import mutual_info_classif, mutual_info_regression
        theirs = mutual_info_classif if discrete else mutual_info_regression
        t0 = time.perf_counter()
        want = theirs(z.astype(np.float64), y, n_neighbors=K, random_state=0, n_jobs=THREADS)
        t = time.perf_counter() - t0
        row.update(sklearn_s=round(t, 3), speedup=round(t / row["scores_s"], 1), largest_difference=float(np.abs(got - want).max()))
    return row


def permutation(z, y, P):
    dev = z.device
    t0 = _clock(dev)
    r = MI.mutual_information_permutation_test(z, y, n_neighbors=K, n_permutations=P, seed=0)
    whole = _clock(dev) - t0
    t0 = _clock(dev)
    MI.mutual_information(z, y, n_neighbors=K)
    one = _clock(dev) - t0
    return dict(P=P, test_s=round(whole, 4), per_permutation_s=round(whole / (P + 1), 5), single_call_s=round(one, 5),
                P_single_calls_s=round(P * one, 3), ratio=round(P * one / whole, 2), pvalue=r.pvalue)


def buffer_share(z, y, k, cap=128, first=4):
    """the append and cut rule of mi_radius_kernel on rows 0..63 against all columns in one chunk, on the host"""
    z, y = z.astype(np.float64), y.astype(np.float64)
    n = len(z)
    sq = lambda a, b: ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    key = np.maximum(sq(z[:64], z), sq(y[:64], y))
    key[np.arange(64), np.arange(64)] = np.inf
    thr = np.full(64, np.inf)
    held = [np.zeros(0) for _ in range(64)]
    seen = {True: [0, 0], False: [0, 0]}   # early tiles / the rest -> [appended, candidates]
    cuts = 0
    for t, c0 in enumerate(range(0, n, 64)):
        tile = key[:, c0:c0 + 64]
        take = tile < thr[:, None]
        seen[t < first][0] += int(take.sum())
        seen[t < first][1] += tile.size
        held = [np.concatenate([h, tile[r][take[r]]]) for r, h in enumerate(held)]
        if max(len(h) for h in held) > cap - 64:
            cuts += 1
            for r, h in enumerate(held):
                if len(h) > k:
                    held[r] = np.sort(h)[:k]
                    thr[r] = held[r][-1]
    return dict(first_tiles=first, share_first=round(seen[True][0] / seen[True][1], 4), share_rest=round(seen[False][0] / max(1, seen[False][1]), 5),
                cuts=cuts, tiles=t + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000,50000")
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--perms", type=int, default=200)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--buffer", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    z, y, lab = rows(min(sizes), a.dim)
    MI.mutual_information(torch.from_numpy(z).cuda(), y, n_neighbors=K)          # warm-up: code objects, torch kernels
    MI.mutual_information(torch.from_numpy(z).cuda(), lab, n_neighbors=K)
    MI.latent_mi_scores(z[:500], y[:500, 0], n_neighbors=K, random_state=0)
    out = dict(device=torch.cuda.get_device_name(0), d=a.dim, k=K, estimate=[], scores=[], permutation=[])
    for n in sizes:
        z, y, lab = rows(n, a.dim)
        zd = torch.from_numpy(z).cuda()
        for name, target in (("q = 3", y), ("labels", lab)):
            row = dict(n=n, y=name, **estimate(zd, target))
            out["estimate"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        for name, target, discrete in (("real", y[:, 0].astype(np.float64), False), ("labels", lab, True)):
            row = dict(n=n, y=name, **scores(z, target, discrete, a.reference))
            out["scores"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        for name, target in (("q = 3", y), ("labels", lab)):
            row = dict(n=n, y=name, **permutation(zd, target, a.perms))
            out["permutation"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    if a.buffer:
        z, y, _ = rows(min(sizes), a.dim)
        out["buffer"] = dict(n=min(sizes), **buffer_share(z, y, K))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
