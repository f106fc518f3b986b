"""Cost of the kNN mutual-information estimate (scrubvae_amd/eval/mutual_info.py, csrc/mi.hip) on n rows of d features around 25
centres, k = 3, inputs already on the device, synchronised host clock, after a warm-up call at the smallest size:

  estimate     mutual_information(z, y) with a real y of q = 3 columns and with the 25 centre labels: the whole call, and of it
               the radius pass, the count pass and the psi sums, each timed in a second run with a synchronisation between them
  scores       latent_mi_scores(z, y) against sklearn's mutual_info_regression / mutual_info_classif on the same host arrays
               (--reference; sklearn on at most 16 host threads), with the largest difference of a score
  permutation  mutual_information_permutation_test at P = --perms against one mutual_information call timed and scaled by P
  buffer       (host, numpy, --buffer) the share of a row tile's candidates that reach the LDS buffer of mi_radius_kernel, over
               the first 4 column tiles and over the rest, by replaying the kernel's append and cut rule on rows 0..63

  conditional  (--conditional, instead of the above) the radius and count passes of conditional_mutual_information with a real c
               next to those of mutual_information at the same n, d, k and y (the four passes timed in turn, 9 times each; the
               median, and the largest (max - min) / median of the four), the whole conditional call, and
               conditional_permutations for 64 permutations of --draw-rows rows at 8 donors

Prints one JSON line.

    python tools/bench_mi.py [--sizes 5000,20000,50000] [--dim 32] [--perms 200] [--reference] [--buffer]
    python tools/bench_mi.py --conditional [--sizes 5000,20000,50000] [--dim 32] [--draw-rows 20000]"""
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


def conditional(z, y, c, repeats=9):
    """z on the device, y [n, 3] and c [n] real -> the radius and count passes of conditional_mutual_information next to those of
    mutual_information on the same z, y and k (the median of `repeats` synchronised host-clock timings each, after one untimed
    call, the four in turn) and the whole conditional call"""
    from scrubvae_amd.eval import conditional_mi as CM
    dev = z.device
    with torch.cuda.device(dev):
        cr = CM._CmiRun(CM._cmi_check(z, y, c, K), dev)
        mr = MI._MiRun(MI._mi_check(z, y, K), dev)
        lib, st = cr.lib, cr.st
        same = (cr.Z.data_ptr(), cr.ld, cr.ld, cr.n, cr.Y.data_ptr(), cr.q)   # z and y are one set of rows for the four passes
        calls = dict(
            cmi_radius=lambda: lib.svae_cmi_radius(*same, cr.C.data_ptr(), cr.p, None, K, cr.work.data_ptr(), cr.rho2.data_ptr(), st),
            cmi_counts=lambda: lib.svae_cmi_counts(*same, cr.C.data_ptr(), cr.p, None, cr.rho2.data_ptr(), cr.nzc.data_ptr(),
                                                   cr.nyc.data_ptr(), cr.nc.data_ptr(), st),
            mi_radius=lambda: lib.svae_mi_radius(*same, None, None, K, mr.work.data_ptr(), mr.rho2.data_ptr(), st),
            mi_counts=lambda: lib.svae_mi_counts(*same, mr.rho2.data_ptr(), mr.nz.data_ptr(), mr.ny.data_ptr(), st))
        took = {name: [] for name in calls}
        for name, call in calls.items():
            MI.check(call())
        for _ in range(repeats):                      # the four passes in turn, so that a busy host touches all of them alike
            for name, call in calls.items():
                t0 = _clock(dev)
                MI.check(call())
                took[name].append(_clock(dev) - t0)
        times = {name: float(np.median(t)) for name, t in took.items()}
        spread = max((max(t) - min(t)) / np.median(t) for t in took.values())
        t0 = _clock(dev)
        value = CM.conditional_mutual_information(z, y, c, n_neighbors=K)
        whole = _clock(dev) - t0
    row = {f"{name}_s": round(t, 5) for name, t in times.items()}
    row.update(value=round(value, 6), whole_s=round(whole, 5), radius_ratio=round(times["cmi_radius"] / times["mi_radius"], 3),
               counts_ratio=round(times["cmi_counts"] / times["mi_counts"], 3), largest_spread=round(float(spread), 3))
    return row


def local_draw(c, P=64, donors=8, repeats=5):
    """conditional_permutations(c, P) of a real c [n] on the device: the median of `repeats` timings after one untimed call, and
    the share of the drawn entries whose donor had served already"""
    from scrubvae_amd.eval import conditional_mi as CM
    cd = torch.as_tensor(c).cuda()
    CM.conditional_permutations(cd, P, n_donors=donors, seed=0)      # untimed: torch's sort and random kernels, svae_knn
    took = []
    for r in range(repeats):
        t0 = _clock(cd.device)
        perms = CM.conditional_permutations(cd, P, n_donors=donors, seed=r)
        took.append(_clock(cd.device) - t0)
    repeated = float((perms.sort(dim=1).values.diff(dim=1) == 0).sum()) / perms.numel()
    return dict(n=len(cd), P=P, n_donors=donors, draw_s=round(float(np.median(took)), 4), slowest_s=round(max(took), 4),
                repeated_share=round(repeated, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000,50000")
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--perms", type=int, default=200)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--buffer", action="store_true")
    ap.add_argument("--conditional", action="store_true")
    ap.add_argument("--draw-rows", type=int, default=20000)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    if a.conditional:
        out = dict(device=torch.cuda.get_device_name(0), d=a.dim, k=K, conditional=[])
        condition = lambda z, n: (0.7 * z[:, 0] + 0.7 * np.random.default_rng(1).normal(size=n)).astype(np.float32)
        z, y, _ = rows(min(sizes), a.dim)
        conditional(torch.from_numpy(z).cuda(), y, condition(z, len(z)), repeats=1)   # warm-up: code objects, torch kernels
        for n in sizes:
            z, y, _ = rows(n, a.dim)
            row = dict(n=n, **conditional(torch.from_numpy(z).cuda(), y, condition(z, n)))
            out["conditional"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        z = rows(a.draw_rows, a.dim)[0]
        out["local_draw"] = local_draw(condition(z, a.draw_rows))
        print(json.dumps(out))
        return
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
