"""One training batch of 4096 x 64 x 18 built three ways, random kept windows of a synthetic recording of 2^20 frames:

  (a) DeviceWindowLoader's build from the resident recording (svae_window_batch + svae_window_speed_parts + pose-tail FK),
  (b) the same batch by the older means on the device: pose[window_inds] gather, inv_kin_windows, get_speed_parts, fwd_kin_cont6d,
  (c) the host path for one batch: 4096 random rows of a pinned host dict of preprocessed windows gathered into pinned staging
      buffers, then copied to the device.  This runs in ONE process (torch's intra-op threads do the gather); a DataLoader with
      collate workers adds inter-process copies on top, so (c) is the host path's best case, not a model of it.  The host set is
      `--host-windows` windows (default 32768 = 1.8 GB), not the whole 29 GB a recording of this length preprocesses to.

    python tools/bench_recording.py [--batch 4096] [--reps 20] [--host-windows 32768]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from scrubvae_amd.data import preprocess as PP
from scrubvae_amd.data import recording as R
from scrubvae_amd.data import synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-windows", type=int, default=32768)
args = ap.parse_args()
B, W, J, FRAMES, STRIDE = args.batch, 64, 18, 1 << 20, 2
KEYS = ["x6d", "root", "offsets", "target_pose", "avg_speed_3d", "heading", "ids"]
tree, offset = synthetic.skeleton(J)
skel = {"KINEMATIC_TREE": tree, "OFFSET": offset}

# a smooth synthetic recording: slowly turning joints on a random-walk root, 16 animals
g = torch.Generator().manual_seed(0)
t = torch.linspace(0, 400.0, FRAMES)[:, None, None]
x6d = (torch.randn(1, J, 6, generator=g) + 0.7 * torch.sin(t * torch.rand(1, J, 6, generator=g) + 6.28 * torch.rand(1, J, 6, generator=g))).cuda()
seg = ((0.5 + torch.rand(J, generator=g))[:, None] * torch.tensor(offset, dtype=torch.float32)).cuda()
pose = synthetic.fwd_kin_cont6d(x6d, tree, seg[None].expand(FRAMES, J, 3).contiguous())
pose = pose + torch.cumsum(0.05 * torch.randn(FRAMES, 1, 3, generator=g), dim=0).cuda()
del x6d
ids = np.repeat(np.arange(16), FRAMES // 16)
sample = pose[(torch.arange(0, FRAMES - W, 257, device="cuda")[:, None] + torch.arange(W, device="cuda"))]
thr = float(torch.sqrt((torch.diff(sample, dim=-3) ** 2).sum(-1)).mean(dim=(-1, -2)).quantile(0.9))
del sample


def timeit(fn, reps=args.reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


torch.cuda.synchronize()
t0 = time.perf_counter()
ds = R.DeviceRecording(pose.cpu().numpy(), ids, skel, W, STRIDE, data_keys=KEYS, speed_threshold=thr)
torch.cuda.synchronize()
print(f"recording {FRAMES} frames x {J} joints = {pose.numel() * 4 / 1e6:.0f} MB resident; {len(ds)} windows kept at stride {STRIDE} "
      f"(threshold {thr:.3f}); set up in {time.perf_counter() - t0:.2f} s (upload + outlier pass)")
index = torch.randperm(len(ds), generator=g)[:B].cuda()
starts = ds.starts[index]
frame = torch.arange(W, device="cuda")

# (a)
t_a_ik = timeit(lambda: ds._window_batch(starts, index, W, ("offsets", "root", "heading")))
t_a_sp = timeit(lambda: ds._build("avg_speed_3d", starts, index, {}))


# (b)
def composed():
    win = ds.pose[starts[:, None] + frame]
    x6d, offsets, root, heading = PP.inv_kin_windows(win, tree, offset, "midfwd")
    return {"x6d": x6d, "root": root, "offsets": offsets, "target_pose": synthetic.fwd_kin_cont6d(x6d, tree, offsets),
            "avg_speed_3d": PP.get_speed_parts(win), "heading": heading, "ids": ds.window_labels["ids"][index]}


rounds = [(timeit(lambda: ds.batch(index)), timeit(composed)) for _ in range(5)]  # alternating, for the spread
t_a, t_b = (sorted(r[i] for r in rounds)[2] for i in (0, 1))
spread = lambda i: "{:.3f}-{:.3f}".format(min(r[i] for r in rounds) * 1e3, max(r[i] for r in rounds) * 1e3)
t_b_gather = timeit(lambda: ds.pose[starts[:, None] + frame])
win = ds.pose[starts[:, None] + frame]
t_b_ik = timeit(lambda: PP.inv_kin_windows(win, tree, offset, "midfwd"))
t_b_sp = timeit(lambda: PP.get_speed_parts(win))
a, b = ds.batch(index), composed()
x6, offs = a["x6d"], a["offsets"]
t_fk = timeit(lambda: synthetic.fwd_kin_cont6d(x6, tree, offs))
zero_row = (index == 0)  # the identity quirk sits elsewhere in (b): leave that row out of the comparison
same = all(torch.equal(a[k][~zero_row][1:], b[k][~zero_row][1:]) for k in KEYS)
moved = B * W * (3 * J + 6 * J + 3 * J + 3) * 4  # pose in; x6d, offsets, root out
print(f"batch {B} x {W} x {J}: {B * W * (6 * J + 3 * J + 3 * J + 3) * 4 / 1e6:.0f} MB of x6d, offsets, target_pose and root")
print(f"(a) fused build      {t_a * 1e3:7.3f} ms (median of 5 alternating rounds, {spread(0)})  = window_batch {t_a_ik * 1e3:.3f} ({moved / t_a_ik / 1e9:.0f} GB/s algorithmic) + speed {t_a_sp * 1e3:.3f} "
      f"+ FK {t_fk * 1e3:.3f} + indexing")
print(f"(b) gather + parent  {t_b * 1e3:7.3f} ms (median of 5, {spread(1)})  = gather {t_b_gather * 1e3:.3f} + inv_kin {t_b_ik * 1e3:.3f} + speed {t_b_sp * 1e3:.3f} "
      f"+ FK {t_fk * 1e3:.3f}   (rows other than window 0's / batch row 0 bit-equal: {same})")

# (c)
n_host = min(args.host_windows, len(ds))
host = {k: v.cpu().pin_memory() for k, v in ds[:n_host].items()}
stage = {k: torch.empty((B,) + v.shape[1:], dtype=v.dtype).pin_memory() for k, v in host.items()}
dev = {k: torch.empty((B,) + v.shape[1:], dtype=v.dtype, device="cuda") for k, v in host.items()}
t_gather = t_copy = 0.0
for rep in range(args.reps + 1):
    idx = torch.randint(0, n_host, (B,), generator=g)
    t0 = time.perf_counter()
    for k, v in host.items():
        torch.index_select(v, 0, idx, out=stage[k])
    t1 = time.perf_counter()
    for k in host:
        dev[k].copy_(stage[k], non_blocking=True)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if rep:  # the first pass warms the pages
        t_gather += (t1 - t0) / args.reps
        t_copy += (t2 - t1) / args.reps
nbytes = sum(v.numel() * v.element_size() for v in stage.values())
print(f"(c) host path        {(t_gather + t_copy) * 1e3:7.3f} ms  = gather of {B} rows out of {n_host} pinned windows {t_gather * 1e3:.2f} "
      f"({nbytes / t_gather / 1e9:.1f} GB/s, {torch.get_num_threads()} threads, one process) + H2D {t_copy * 1e3:.2f} ({nbytes / t_copy / 1e9:.1f} GB/s)")
print(f"(a) / (b) = {t_a / t_b:.2f};  (a) builds {B / t_a / 1e3:.0f} k windows/s")
