"""Same-process A/B of the split gather kernels' two epilogue paths (ops.set_epilogue_wide: dword / 16-byte) per layer, tile code and
epilogue mode: data gradient plain, accumulating, and with the fused BatchNorm + PReLU backward sums; forward with statistics.
Every timed launch follows a 1 GiB write (the operands come from HBM as inside a training step); the two paths alternate.
    B=4096 LAYERS=mid python tools/time_epilogue.py 8128128 29128128"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from scrubvae_amd import ops, _lib

B = int(os.environ.get("B", 4096))
SETS = {
    "deep": [("enc3.c3", 4, 512, 1024, 5, 1, 2, False), ("dec0.sk", 8, 1024, 512, 6, 1, 2, False), ("dec0.t1", 4, 1024, 512, 5, 1, 2, True)],
    "mid": [("dec1.sk", 14, 512, 256, 6, 1, 2, False), ("dec1.t1", 7, 512, 256, 5, 1, 2, True), ("enc2.c3", 8, 256, 512, 5, 1, 2, False)],
    "skinny": [("dec2.sk", 26, 256, 128, 6, 1, 2, False), ("dec2.t1", 13, 256, 128, 5, 1, 2, True), ("dec3.sk", 50, 128, 64, 6, 1, 2, False),
               ("enc1.c3", 16, 128, 256, 5, 1, 2, False)],
    "s2": [("enc3.c0", 8, 512, 512, 5, 2, 2, False), ("enc1.sk", 32, 128, 256, 5, 2, 2, False), ("dec1.t2", 7, 256, 256, 5, 2, 2, True)],
}
REPS = int(os.environ.get("REPS", 6))
_flush = torch.empty(1 << 28, dtype=torch.float32, device="cuda")


def cold_time(fn):
    tot = 0.0
    for _ in range(REPS):
        _flush.add_(1.0)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); torch.cuda.synchronize()
        tot += s.elapsed_time(e)
    return tot / REPS * 1e3


def main():
    codes = [int(c) for c in sys.argv[1:]] or [8128128, 9128128, 29128128]
    for set_name in os.environ.get("LAYERS", "deep,mid,skinny,s2").split(","):
        for name, l_in, cin, cout, k, s, p, tr in SETS[set_name]:
            for code in codes:
                cv = ops.Conv(B, l_in, cin, cout, k, s, p, 1, tr, pieces=3)
                cv.__dict__["_tuned"] = {"fwd", "dgrad", "wgrad"}
                cv._set_choice("fwd", 22, code)
                cv._set_choice("dgrad", 2, code)
                x = torch.randn(B * l_in, cv.c_in_p, device="cuda")
                w = torch.randn(*cv.weight_shape, device="cuda") * 0.05
                y = torch.randn(B * cv.l_out, cv.c_out_p, device="cuda")
                ops.bump_weight_epoch()
                try:
                    cv.fwd(x, w, None, y)
                    cv.dgrad(y, w, x)
                except RuntimeError:
                    print(f"{name:8s} {code}: n/a")
                    continue
                n, cb = cv.dgrad_stats_tiles()
                keep = [torch.randn(B * l_in, cv.c_in_p, device="cuda")] + [torch.rand(cv.c_in_p, device="cuda") + 0.5 for _ in range(4)]
                keep += [torch.tensor([0.25], device="cuda"), torch.empty(n * 2 * cv.c_in_p, device="cuda"), torch.empty(2 * n * cb, device="cuda")]
                fuse = _lib.BnBwdFuse()
                fuse.x, fuse.scale, fuse.shift, fuse.mean, fuse.rstd, fuse.alpha, fuse.part, fuse.dalpha_part = (t.data_ptr() for t in keep)
                part = torch.empty(cv.stats_tiles() * 2 * cv.c_out_p, device="cuda")
                dx = torch.empty_like(x)
                modes = {"dgrad plain": lambda: cv.dgrad(y, w, dx), "dgrad acc": lambda: cv.dgrad(y, w, dx, accumulate=True),
                         "dgrad bn": lambda: cv.dgrad(y, w, dx, fuse=fuse), "fwd stats": lambda: cv.fwd(x, w, None, y, stats=part)}
                for mode, fn in modes.items():
                    for _ in range(2):
                        fn()
                    t = []
                    for wide in (0, 1, 0, 1):
                        ops.set_epilogue_wide(wide)
                        t.append(cold_time(fn))
                    ops.set_epilogue_wide(True)
                    off, on = (t[0] + t[2]) / 2, (t[1] + t[3]) / 2
                    print(f"{name:8s} {code:9d} {mode:12s} dword {t[0]:7.1f} {t[2]:7.1f}  16-byte {t[1]:7.1f} {t[3]:7.1f} us   {(off / on - 1) * 100:+5.1f} %")


if __name__ == "__main__":
    main()
