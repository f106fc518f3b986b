"""In-kernel s_memtime stamps around the epilogue of the 8-wave halo kernel (library built with --ablation): what part of a tile's
life its output movement is, with the dword path and with the 16-byte path (ops.set_epilogue_wide).

Per wave of the workgroup in the middle of the grid: entry | stage loop done | epilogue issued | stores drained.  Prints, per launch,
the median over the waves of the loop's and the epilogue's cycles and the epilogue's share of the tile.  Launches: a deep data
gradient (enc3.c3, 256 x 256 tiles), a shallow one (dec2.t1, 128 x 128 tiles, 160-row image), each plain, accumulating and with
the fused BatchNorm + PReLU backward sums.  Stamps are diagnostic only: the build is never shipped and no output depends on them."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scrubvae_amd import ops, _lib

B = int(os.environ.get("B", 4096))
LAYERS = {"enc3.c3": ((4, 512, 1024, 5, 1, 2, False), 29128128), "dec2.t1": ((13, 256, 128, 5, 1, 2, True), 8128128),
          "dec3.sk": ((50, 128, 64, 6, 1, 2, False), 8128128)}


def run(name, mode):
    (l_in, cin, cout, k, s, p, tr), code = LAYERS[name]
    cv = ops.Conv(B, l_in, cin, cout, k, s, p, 1, tr, pieces=3)
    cv.__dict__["_tuned"] = {"fwd", "dgrad", "wgrad"}
    cv._set_choice("dgrad", 2, code)
    dx = torch.randn(B * l_in, cv.c_in_p, device="cuda")
    w = torch.randn(*cv.weight_shape, device="cuda") * 0.05
    dy = torch.randn(B * cv.l_out, cv.c_out_p, device="cuda")
    ops.bump_weight_epoch()
    fuse = None
    if mode == "bn":
        n, cb = cv.dgrad_stats_tiles()
        keep = [torch.randn(B * l_in, cv.c_in_p, device="cuda")] + [torch.rand(cv.c_in_p, device="cuda") + 0.5 for _ in range(4)]
        keep += [torch.tensor([0.25], device="cuda"), torch.empty(n * 2 * cv.c_in_p, device="cuda"), torch.empty(2 * n * cb, device="cuda")]
        fuse = _lib.BnBwdFuse()
        fuse.x, fuse.scale, fuse.shift, fuse.mean, fuse.rstd, fuse.alpha, fuse.part, fuse.dalpha_part = (t.data_ptr() for t in keep)
    fn = lambda: cv.dgrad(dy, w, dx, accumulate=mode == "acc", fuse=fuse)
    l = _lib.lib()
    l.svae_debug_epilogue_stamp_buffer.argtypes = [C.c_void_p]
    l.svae_debug_epilogue_stamp_buffer.restype = C.c_int
    buf = torch.zeros(32, dtype=torch.int64, device="cuda")
    for wide in (False, True, False, True):
        ops.set_epilogue_wide(wide)
        assert l.svae_debug_epilogue_stamp_buffer(None) == 0
        for _ in range(10):  # warm clocks / caches
            fn()
        torch.cuda.synchronize()
        assert l.svae_debug_epilogue_stamp_buffer(C.c_void_p(buf.data_ptr())) == 0
        fn()
        torch.cuda.synchronize()
        assert l.svae_debug_epilogue_stamp_buffer(None) == 0
        t = buf.cpu().numpy().astype(np.int64).reshape(8, 4)
        d = np.diff(t, axis=1)
        loop, issue, drain = (int(np.median(d[:, i])) for i in range(3))
        last = int((t[:, 3].max() - t[:, 0].min()))
        print(f"{name:8s} {cv.kernel_name('dgrad'):60s} {mode:5s} wide={int(wide)}: entry..loop end {loop:7d}  epilogue issued {issue:6d}  "
              f"drained +{drain:5d}  tile {last:7d}  epilogue share {(issue + drain) / max(loop + issue + drain, 1) * 100:5.1f} %")
    ops.set_epilogue_wide(True)


if __name__ == "__main__":
    for name in os.environ.get("LAYER", "enc3.c3,dec2.t1,dec3.sk").split(","):
        for mode in ("plain", "acc", "bn"):
            run(name, mode)
