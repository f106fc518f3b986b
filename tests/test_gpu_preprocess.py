"""On-device pose preprocessing (csrc/preprocess.hip: inv_kin_kernel, speed_parts_kernel; data/preprocess.py; the pose-tail
kernel's forward kinematics behind target_pose) against the fp64 restatement of tests/preprocess_checks.py.

Inputs are drawn in fp64 and rounded to fp32 once.  x6d and target_pose have to meet, in every kappa bucket,

    max |kernel - fp64|  <=  max(8 max |fp32 restatement - fp64|, 8 2^-24)

(absolute for x6d, in units of the truth's max-norm for target_pose); root, heading, avg_speed_3d and the float-OFFSET offsets
meet latent_checks.gate as it is; the integer-OFFSET (truncated) offsets are exact wherever the fp64 length is clear of a
truncation step.  The fairness of the inputs (bucket shares, truncation share, threshold clearance) is asserted in
test_preprocess_cpu.py.  Each gate prints its figures (run with -s).

The cases are chosen by what they make the 64-frame-tile kernel do:
    4096 x 64 x 18  midfwd int    the benchmark size, tile == window
    1000 x 51 x 18  midfwd float  windows straddle tiles, the middle frame lies in another tile, 51,000 % 64 = 56 leaves a partial
                                  last tile, the heading is written from lanes other than 0
    257 x 256 x 23  x360 float    a window of four tiles, W > 64 in the speed kernel's lane loop, 70,912 B of dynamic LDS
                                  (more than 64 KiB), the padded-input branch of fwd_kin_cont6d (6 J % 4 != 0)
    300 x 64 x 23   midfwd int    J = 23 with truncated lengths
    3 x 2 x 23      None int      W = 2: 6 frames in one partial tile, no centring and no rotation
    70 x 33 x 8     midfwd float  one chain of SVAE_MAX_CHAIN_LEN joints: the second wave idles; one speed part: limbs = 0"""
import ctypes as C

import pytest
import torch

from tests import preprocess_checks as PC
from tests.preprocess_checks import SENTINEL, gate

pytestmark = pytest.mark.gpu

GUARD = 3  # sentinel rows behind every output buffer of the direct C ABI calls


@pytest.fixture(scope="module")
def PP():
    from scrubvae_amd.data import preprocess as _pp
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _pp


def run_kernels(PP, pose, tree, offset, direction, parts):
    from scrubvae_amd.data import synthetic
    dev = pose.float().cuda()
    x6d, offsets, root, heading = PP.inv_kin_windows(dev, tree, offset, direction)
    out = dict(x6d=x6d, offsets=offsets, root=root, heading=heading, avg_speed_3d=PP.get_speed_parts(dev, parts),
               target_pose=synthetic.fwd_kin_cont6d(x6d, tree, offsets))
    torch.cuda.synchronize()
    assert out["x6d"].shape == pose.shape[:3] + (6,) and out["target_pose"].shape == pose.shape
    return out


def truths(pose, tree, offset, direction, parts):
    return tuple(PC.restate(pose, tree, offset, PC.ALL_KEYS, direction, parts, dt) for dt in (torch.float64, torch.float32))


@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_id)
def test_kernels_vs_fp64(PP, case):
    N, W, J, direction, kind, parts = case
    name = PC.case_id(case)
    tree, offset = PC.skeleton(J, kind)
    pose = PC.make_pose(N, W, J)
    t64, t32 = truths(pose, tree, offset, direction, parts)
    assert all(bool(torch.isfinite(v).all()) for v in t64.values())
    got = run_kernels(PP, pose, tree, offset, direction, parts)
    PC.gate_all(name, got, pose, tree, offset, direction, parts, t64, t32)
    # frame 0 of the flattened array carries the identity root quaternion, under "midfwd" turned by the window's yaw
    x0, yaw = got["x6d"][0, 0, 0].cpu().double(), t64["yaw"]
    if direction == "midfwd":
        c, s = float(torch.cos(yaw[0, 0])), float(torch.sin(yaw[0, 0]))
        gate(name + " frame 0", x0, torch.tensor([c, s, 0.0, -s, c, 0.0], dtype=torch.float64), t32["x6d"][0, 0, 0], denom=1.0)
    else:
        assert torch.equal(x0, torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64))
    gate(name + " heading vs yaw", got["heading"], torch.cat([torch.sin(yaw), torch.cos(yaw)], dim=-1), t32["heading"])


# ------------------------------------------------------------------------------------------------ the C ABI, called directly
def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def only_sentinel(t):
    return t.numel() == 0 or bool((t == SENTINEL).all())


def uoff(offset):
    flat = [float(v) for row in offset for v in row]
    return (C.c_float * len(flat))(*flat)


def abi_inv_kin(pose, tree_struct, uo, W, J, direction, truncate, frames=None, want=("offsets", "root", "heading")):
    """svae_inv_kin into sentinel-filled buffers with GUARD rows behind the `frames` (heading: windows) the call may write;
    -> status, buffers"""
    from scrubvae_amd import _lib
    frames = pose.shape[0] * pose.shape[1] if frames is None else frames
    n_win = frames // W
    buf = dict(x6d=sentinel(frames + GUARD, J, 6), offsets=sentinel(frames + GUARD, J, 3), root=sentinel(frames + GUARD, 3),
               heading=sentinel(n_win + GUARD, 2))
    p = lambda k: buf[k].data_ptr() if k == "x6d" or k in want else None
    st = _lib.lib().svae_inv_kin(pose.data_ptr(), uo, C.byref(tree_struct), W, int(direction == "midfwd"),
                                 int(direction in ("midfwd", "x360")), truncate, p("x6d"), p("offsets"), p("root"), p("heading"),
                                 frames, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, buf


def abi_speed(pose, parts, W, J, windows):
    from scrubvae_amd import _lib
    flat = [j for part in parts for j in part]
    out = sentinel(windows + GUARD, 3)
    st = _lib.lib().svae_speed_parts(pose.data_ptr(), (C.c_int * len(flat))(*flat), (C.c_int * len(parts))(*[len(q) for q in parts]),
                                     len(parts), W, J, out.data_ptr(), windows, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, out


def test_buffer_discipline(PP):
    """51,000 frames end in a partial tile: nothing is written behind the last frame / window, and a null output pointer changes
    no other output"""
    from scrubvae_amd import _lib
    N, W, J, direction, kind, parts = PC.CASES[1]
    tree, offset = PC.skeleton(J, kind)
    pose = PC.make_pose(N, W, J).float().cuda()
    ts, uo, frames = _lib.make_tree(J, tree), uoff(offset), N * W
    st, full = abi_inv_kin(pose, ts, uo, W, J, direction, 0)
    assert st == 0, _lib.last_error()
    rows = dict(x6d=frames, offsets=frames, root=frames, heading=N)
    for k, n in rows.items():
        assert only_sentinel(full[k][n:]), k
        assert not bool((full[k][:n] == SENTINEL).any()), k
    for want in (("root", "heading"), ("offsets", "heading"), ("offsets", "root"), ()):
        st, part = abi_inv_kin(pose, ts, uo, W, J, direction, 0, want=want)
        assert st == 0, _lib.last_error()
        for k in rows:
            if k == "x6d" or k in want:
                assert torch.equal(part[k], full[k]), (want, k)
            else:
                assert only_sentinel(part[k]), (want, k)
    st, spd = abi_speed(pose, parts, W, J, N)
    assert st == 0 and only_sentinel(spd[N:]) and not bool((spd[:N] == SENTINEL).any())
    # the Python entry point's switches
    x6d, offsets, root, heading = PP.inv_kin_windows(pose, tree, offset, direction, want_offsets=False, want_root=False)
    torch.cuda.synchronize()
    assert offsets is None and root is None
    assert torch.equal(x6d.reshape(frames, J, 6), full["x6d"][:frames]) and torch.equal(heading, full["heading"][:N])


def test_bit_reproducible(PP):
    N, W, J, direction, kind, parts = PC.CASES[1]
    tree, offset = PC.skeleton(J, kind)
    pose = PC.make_pose(N, W, J)
    a, b = (run_kernels(PP, pose, tree, offset, direction, parts) for _ in range(2))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_preprocess_pose_end_to_end(PP):
    """window 51 / stride 3 over three id runs (one shorter than the window) with a speed threshold that drops some windows"""
    pose, ids, win, spd, thr = PC.e2e_inputs()
    tree, offset = PC.skeleton(PC.E2E["J"], "float")
    skel = {"KINEMATIC_TREE": tree, "OFFSET": offset}
    keys = list(PC.ALL_KEYS) + ["ids"]
    out = PP.preprocess_pose(pose.numpy(), ids, skel, PC.E2E["window"], PC.E2E["stride"], data_keys=keys, speed_threshold=thr,
                             direction_process="midfwd")
    torch.cuda.synchronize()
    keep = spd <= thr
    kept = pose[win][keep]
    assert 0 < int(keep.sum()) < len(win)
    assert set(out) == set(keys) | {"raw_pose"}
    assert out["raw_pose"].shape[0] == int(keep.sum()) and torch.equal(out["raw_pose"].cpu().double(), kept)
    want_ids = torch.from_numpy(ids)[win[:, PC.E2E["window"] // 2]][keep]
    assert out["ids"].dtype == torch.int16 and torch.equal(out["ids"].cpu().long(), want_ids.long())
    assert len(set(want_ids.tolist())) == 2  # both long runs survive
    PC.gate_all("preprocess_pose", {k: out[k] for k in PC.ALL_KEYS}, kept, tree, offset, "midfwd", PC.SPEED_PARTS)
    only = PP.preprocess_pose(pose.numpy(), ids, skel, PC.E2E["window"], PC.E2E["stride"], data_keys=["avg_speed_3d", "ids"],
                              speed_threshold=thr, direction_process="midfwd")
    assert set(only) == {"raw_pose", "avg_speed_3d", "ids"}
    assert torch.equal(only["avg_speed_3d"], out["avg_speed_3d"]) and torch.equal(only["ids"], out["ids"])


def test_degenerate_poses(PP):
    """A bone exactly against its unit offset, two coincident keypoints, a root forward vector exactly along -x, and a middle
    frame without a forward vector: the reference's arithmetic yields 0 / 0 there (test_preprocess_cpu.py spells out where).  The
    kernel's non-finite entries are exactly the restatement's, `offsets` stays finite, and every other frame and chain -- those
    of the same tiles included -- still meets the gate."""
    d = PC.DEGENERATE
    tree, offset = PC.skeleton(d["J"], "float")
    pose = PC.degenerate_pose()
    t64, t32 = truths(pose, tree, offset, "midfwd", PC.SPEED_PARTS)
    assert int((~torch.isfinite(t64["x6d"])).sum()) > 0
    got = run_kernels(PP, pose, tree, offset, "midfwd", PC.SPEED_PARTS)
    assert bool(torch.isfinite(got["offsets"]).all()) and bool(torch.isfinite(got["avg_speed_3d"]).all())
    PC.gate_all("degenerate", got, pose, tree, offset, "midfwd", PC.SPEED_PARTS, t64, t32)


def test_rejections(PP):
    """bad shapes return SVAE_ERR_SHAPE with a message and launch nothing"""
    from scrubvae_amd import _lib
    J, W = 18, 64
    tree, offset = PC.skeleton(J, "float")
    pose = PC.make_pose(2, W, J).float().cuda()
    good = lambda: _lib.make_tree(J, tree)

    def rejected(st, bufs, text):
        assert st == _lib.ERR_SHAPE, (st, text)
        assert text in _lib.last_error(), (_lib.last_error(), text)
        assert all(only_sentinel(b) for b in bufs), text

    st, buf = abi_inv_kin(pose, good(), uoff(offset), W, J, "midfwd", 0, frames=W + 1)
    rejected(st, buf.values(), "not a multiple of window")
    t = good()
    t.n_joints = 33
    st, buf = abi_inv_kin(pose, t, uoff(offset + [[1.0, 0.0, 0.0]] * 15), W, J, "midfwd", 0)
    rejected(st, buf.values(), "33 joints")
    t = good()
    t.n_chains = 9
    st, buf = abi_inv_kin(pose, t, uoff(offset), W, J, "midfwd", 0)
    rejected(st, buf.values(), "bad chain count")
    t = good()
    t.chain[0][1] = J
    st, buf = abi_inv_kin(pose, t, uoff(offset), W, J, "midfwd", 0)
    rejected(st, buf.values(), "joint index out of range")
    st, out = abi_speed(pose, PC.SPEED_PARTS, 1, J, 2)
    rejected(st, [out], "speed_parts: bad shape")
    st, out = abi_speed(pose, ([0, 1, J],), W, J, 2)
    rejected(st, [out], "speed_parts: joint index out of range")
    st, out = abi_speed(pose, ([0, 1], [0, 2], [0, 3], [0, 4]), W, J, 2)
    rejected(st, [out], "speed_parts: bad shape")
    # and the same arguments, valid, still run
    st, buf = abi_inv_kin(pose, good(), uoff(offset), W, J, "midfwd", 0)
    assert st == 0 and not bool((buf["x6d"][:2 * W] == SENTINEL).any())
