"""Cost of the Gaussian HMM on the device (scrubvae_amd/eval/hmm.py, csrc/hmm.hip) at d = 32, n in {10^5, 10^6}, K in {8, 25, 64},
as one sequence and as 100 equal sequences, inputs on the device:

  - the forward-backward pass by phase (transfer, carry, fill) and whole, at the library's segment length and at --segments L,...
    (the choice of L); the transfer kernel's 2 n KP^3 flops are set against the fp64 matrix rate (--matrix-tflops, 78.6 by the
    spec sheet): a whole-kernel figure, not a counter reading
  - the same fill kernels run with one segment per sequence: the frame-by-frame pass on the same GPU
  - one EM iteration (E-step, pass, M-step, chain update, the host's record) and a whole fit of --fit-iters iterations (tol = 0)
    including the mixture initialisation
  - Viterbi, per frame
  - the plain scaled recursion in numpy on at most 16 host threads, on --host-frames frames of the same inputs, per frame

Times are a synchronised host clock: after a warm-up call of the same shape, the calls per window are set so that a window lasts
at least --window-ms (one call where a call is longer), and the median of 5 windows is reported with (max - min) / median as its
spread (key + "_spread").  The frame-by-frame fill, seconds long, is timed once.  Viterbi is the library call alone, its inputs
and outputs on the device.  Prints one JSON line.

    python tools/bench_hmm.py [--sizes 100000,1000000] [--ks 8,25,64] [--seqs 1,100] [--segments 64,128,256,512,1024]
                              [--fit-iters 10] [--host-frames 100000] [--no-fit] [--no-host] [--no-serial]"""
import argparse
import importlib
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

H = importlib.import_module("scrubvae_amd.eval.hmm")
THREADS, D = 16, 32


WINDOWS = 5      # timed windows: the median is reported, the spread next to it
WINDOW_S = 0.05  # least length of a window (--window-ms)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def timed(fn):
    """(median, (max - min) / median) of the seconds per call over WINDOWS windows of at least WINDOW_S, after a warm-up call"""
    fn()
    t = window(fn, 1)
    reps = max(1, min(100000, int(np.ceil(WINDOW_S / max(t, 1e-7)))))
    per = [window(fn, reps) for _ in range(WINDOWS)]
    med = float(np.median(per))
    return med, (max(per) - min(per)) / med


def ms(row, key, fn):
    t, spread = timed(fn)
    row[key + "_ms"], row[key + "_spread"] = round(1e3 * t, 4), round(spread, 3)


def inputs(n, K, seed=0):
    """scaled emissions of overlapping states along a sticky chain, made on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn(K, n, generator=g, device="cuda", dtype=torch.float64) * 1.5
    B = torch.softmax(logits, 0).contiguous()
    lpn = torch.randn(n, generator=g, device="cuda", dtype=torch.float64) - 40.0
    A = torch.rand(K, K, generator=g, device="cuda", dtype=torch.float64) + 1e-3
    A = 0.1 * A / A.sum(1, keepdim=True) + 0.9 * torch.eye(K, device="cuda", dtype=torch.float64)
    pi = torch.full((K,), 1.0 / K, device="cuda", dtype=torch.float64)
    return B, lpn, pi, A.contiguous()


def plain_numpy(B, pi, A):
    """the plain scaled recursion of one sequence, as tests/hmm_checks.py::plain without the outputs nobody reads here"""
    K, n = B.shape
    alpha, c = np.empty((K, n)), np.empty(n)
    for t in range(n):
        u = (pi if t == 0 else alpha[:, t - 1] @ A) * B[:, t]
        c[t] = u.sum()
        alpha[:, t] = u / c[t]
    beta, Xi = np.ones(K), np.zeros((K, K))
    for t in range(n - 1, 0, -1):
        y = B[:, t] * beta
        Xi += alpha[:, t - 1][:, None] * A * y[None, :] / c[t]
        beta = (A @ y) / c[t]
    return np.log(c).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--ks", default="8,25,64")
    ap.add_argument("--seqs", default="1,100")
    ap.add_argument("--segments", default="64,128,256,512,1024")
    ap.add_argument("--fit-iters", type=int, default=10)
    ap.add_argument("--host-frames", type=int, default=100000)
    ap.add_argument("--matrix-tflops", type=float, default=78.6)
    ap.add_argument("--window-ms", type=float, default=50.0)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-serial", action="store_true")
    args = ap.parse_args()
    global WINDOW_S
    WINDOW_S = args.window_ms * 1e-3
    torch.set_num_threads(min(torch.get_num_threads(), THREADS))
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"d": D, "pass": {}, "segment_choice": {}, "serial": {}, "em": {}, "viterbi": {}, "host": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        for K in (int(s) for s in args.ks.split(",")):
            B, lpn, pi, A = inputs(n, K)
            KP = H.padded_states(K)
            for nseq in (int(s) for s in args.seqs.split(",")):
                key = f"n{n}_K{K}_seq{nseq}"
                lengths = np.full(nseq, n // nseq, np.int64)
                lengths[-1] += n - int(lengths.sum())
                for L in [None] + ([int(s) for s in args.segments.split(",")] if nseq == 1 else []):
                    p = H._Pass(n, K, lengths, dev, L=L)
                    p.run(B, lpn, pi, A)
                    row = {"L": p.L}
                    ms(row, "transfer", lambda: p.transfer(B, A))
                    ms(row, "carry", lambda: p.carry(pi))
                    ms(row, "fill", lambda: p.fill(B, lpn, A))
                    ms(row, "pass", lambda: p.run(B, lpn, pi, A))
                    row["transfer_share_of_matrix_rate"] = round(2.0 * n * KP ** 3 / (row["transfer_ms"] * 1e-3) / (args.matrix_tflops * 1e12), 4)
                    (out["pass"] if L is None else out["segment_choice"])[key if L is None else f"{key}_L{L}"] = row
                    print(key, row, file=sys.stderr, flush=True)
                    del p
                if not args.no_serial:
                    p = H._Pass(n, K, lengths, dev, L=int(lengths.max()))  # one segment per sequence: frame by frame
                    p.carry(pi)
                    torch.cuda.synchronize()  # the kernels are warm from the pass above; one call is seconds long
                    t0 = time.perf_counter()
                    p.fill(B, lpn, A)
                    torch.cuda.synchronize()
                    out["serial"][key] = {"fill_ms": round(1e3 * (time.perf_counter() - t0), 3)}
                    print(key, "serial", out["serial"][key], file=sys.stderr, flush=True)
                    del p
                _, seq = H.segment_table(lengths, 1 << 30)
                seq_d = torch.from_numpy(seq).to(dev)
                logB = torch.log(B).add_(lpn[None, :])
                lpi, lA = torch.log(pi), torch.log(A)
                row = {}
                ms(row, "viterbi", lambda: H._viterbi_device(logB, lpi, lA, seq_d))
                row["us_per_frame_of_the_longest_sequence"] = round(1e3 * row["viterbi_ms"] / int(lengths.max()), 4)
                out["viterbi"][key] = row
                print(key, "viterbi", out["viterbi"][key], file=sys.stderr, flush=True)
                del logB
                if not args.no_fit:
                    g = np.random.default_rng(0)
                    x = torch.randn(n, D, device=dev) + torch.from_numpy(g.normal(size=(K, D)).astype(np.float32) * 0.6).to(dev)[
                        torch.from_numpy(np.repeat(g.integers(0, K, n // 50 + 1), 50)[:n]).to(dev)]
                    R = H._Rows(x, K, False, dev)
                    R.set_params(np.ones(K), g.normal(size=(K, D)) * 0.6, np.stack([np.eye(D)] * K))
                    em = H._HmmEM(R, lengths, 1e-6, 1.0, 1.0)
                    em.set_chain(pi.cpu().numpy(), A.cpu().numpy())
                    row = {}
                    ms(row, "em_iteration", em.iterate)
                    del em, R
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        m = H.GaussianHMM(K, n_iter=args.fit_iters, tol=0.0, random_state=0)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        m.fit(x, lengths)
                        torch.cuda.synchronize()
                    row.update(fit_s=round(time.perf_counter() - t0, 3), fit_iters=m.n_iter_)
                    out["em"][key] = row
                    print(key, "em", row, file=sys.stderr, flush=True)
                    del x
            if not args.no_host:
                from threadpoolctl import threadpool_limits
                m = min(n, args.host_frames)
                Bh, pih, Ah = B[:, :m].cpu().numpy(), pi.cpu().numpy(), A.cpu().numpy()
                with threadpool_limits(THREADS):
                    t0 = time.perf_counter()
                    plain_numpy(Bh, pih, Ah)
                    t = time.perf_counter() - t0
                out["host"][f"K{K}"] = {"frames": m, "s": round(t, 3), "us_per_frame": round(1e6 * t / m, 3)}
                print(f"K{K} host", out["host"][f"K{K}"], file=sys.stderr, flush=True)
            del B, lpn
    print(json.dumps(out))


if __name__ == "__main__":
    main()
