"""Plain-torch restatement of the pose preprocessing (csrc/preprocess.hip, data/preprocess.py), used by test_preprocess_cpu.py
(against oracle/preprocess_oracle.py and the reference's recorded outputs) and test_gpu_preprocess.py (against the kernels).

`restate` follows oracle.preprocess_oracle.preprocess_windows step by step, but the quaternion helpers run in the dtype `dt` they
are given: on float64 it is the truth, on float32 the yardstick e32 -- the error the reference's own fp32 arithmetic makes on
these inputs.  The pose differences, norms, yaw and speeds stay in float64 on both sides, as the reference's numpy does.  The
input generator draws in fp64 and rounds to fp32 once, so truth, yardstick and kernel see the same numbers.

The bound for x6d / target_pose is bucketed by the conditioning `kappa` of each (frame, joint) entry: qbetween computes
w = |u||v| + u.v, which cancels when a bone points against its unit offset, and a quaternion's error carries down its chain.
FACTOR and FLOOR are latent_checks' (the project's margin of an fp32 kernel over an fp32 yardstick)."""
import math

import numpy as np
import torch

from oracle import preprocess_oracle as P
from oracle import scvae_oracle as O
from tests.latent_checks import FACTOR, FLOOR, SENTINEL, gate, r32  # noqa: F401  (re-exported for the tests)

SPEED_PARTS = P.SPEED_PARTS
IK_KEYS = ("x6d", "root", "offsets", "heading", "target_pose")
ALL_KEYS = IK_KEYS + ("avg_speed_3d",)
EDGES = (0.0, 10.0, 30.0, 100.0, 1000.0, math.inf)  # a partition of kappa, not a tolerance
TRUNC_CLEAR = 1e-5  # an integer-OFFSET length this close (relative) to a truncation step may round either way in fp32
TRUNC_SHARE = 1e-4  # at most this share of the entries may be that close
THRESH_CLEAR = 1e-4  # no window's mean speed may be this close (relative) to the speed threshold

# (windows, W, J, direction_process, OFFSET kind, speed parts): what each reaches is in test_gpu_preprocess.py
CASES = [
    (4096, 64, 18, "midfwd", "int", SPEED_PARTS),
    (1000, 51, 18, "midfwd", "float", SPEED_PARTS),
    (257, 256, 23, "x360", "float", SPEED_PARTS),
    (300, 64, 23, "midfwd", "int", SPEED_PARTS),
    (3, 2, 23, None, "int", SPEED_PARTS),
    (70, 33, 8, "midfwd", "float", ([0, 1, 2, 3, 4, 5, 6, 7],)),
]


def case_id(case):
    return "{}x{}x{}-{}-{}".format(*case[:5])


def skeleton(J, kind):
    """KINEMATIC_TREE and OFFSET (a list of ints or of floats, which decides the truncation) of the J-joint skeleton"""
    conv = float if kind == "float" else int
    return O.skeleton_tree(J), [[conv(c) for c in row] for row in O.skeleton_offsets(J)]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def make_pose(N, W, J, seed=0):
    """[N, W, J, 3] fp64 holding fp32 values: forward kinematics of random 6-D rotations with per-joint segment lengths in
    [0.5, 1.5), plus a random-walk root per window (tools/bench_preprocess.py, oracle.synthetic_raw_pose)"""
    g = _gen(N, W, J, seed, 17)
    tree, offs = O.skeleton_tree(J), torch.tensor(O.skeleton_offsets(J), dtype=torch.float64)
    x6d = torch.randn(N * W, J, 6, generator=g, dtype=torch.float64)
    seg = 0.5 + torch.rand(J, generator=g, dtype=torch.float64)
    root = torch.cumsum(0.05 * torch.randn(N, W, 3, generator=g, dtype=torch.float64), dim=1)
    pose = O.fwd_kin(x6d, tree, offs * seg[:, None], torch.zeros(N * W, 3, dtype=torch.float64), eps=1e-8)
    return r32(pose.reshape(N, W, J, 3) + root[:, :, None, :])


# ------------------------------------------------------------------------------------------------ the restatement
def _unit(v):
    return v / torch.linalg.norm(v, dim=-1, keepdim=True)


def parents(tree, J):
    """get_segment_len's parent table: joints outside every chain keep parent 0"""
    par = [0] * J
    par[0] = -1
    for chain in tree:
        for i in range(1, len(chain)):
            par[chain[i]] = chain[i - 1]
    return par


def inv_kin(pose, tree, offset, dt):
    """pose [F, J, 3] fp64 -> local quaternions [F, J, 4] in dt.  Every chain starts from the frame's root quaternion; the
    root quaternion of frame 0 of the flattened array is the identity (the reference's quirk)."""
    F_ = pose.shape[0]
    offset = torch.as_tensor(np.array(offset), dtype=torch.float64)
    fwd = _unit(pose[:, 0] - pose[:, 1])  # forward_indices = [1, 0]
    ex = torch.tensor([1.0, 0.0, 0.0], dtype=dt).expand(F_, 3)
    root_q = P.qbetween(fwd.to(dt), ex)
    root_q[0] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=dt)
    local = torch.zeros(F_, pose.shape[1], 4, dtype=dt)
    local[:, 0] = root_q
    for chain in tree:
        R = root_q
        for a, b in zip(chain[:-1], chain[1:]):
            v = _unit(pose[:, b] - pose[:, a])
            rot = P.qbetween(offset[b].to(dt).expand(F_, 3), v.to(dt))
            loc = P.qmul(P.qinv(R), rot)
            local[:, b] = loc
            R = P.qmul(R, loc)
    return local


def segment_len(pose, tree, offset):
    """pose [F, J, 3] fp64 -> (offsets, raw) [F, J, 3]: raw = |pose_j - pose_parent(j)| * OFFSET_j, offsets = raw truncated
    toward zero when OFFSET is an integer array (numpy's assignment into it), raw itself otherwise"""
    off = np.array(offset)
    par = parents(tree, pose.shape[1])
    raw = torch.as_tensor(off, dtype=torch.float64).expand(pose.shape).clone()
    for j in range(1, pose.shape[1]):
        raw[:, j] = torch.linalg.norm(pose[:, j] - pose[:, par[j]], dim=-1, keepdim=True) * raw[:, j]
    return (torch.trunc(raw) if np.issubdtype(off.dtype, np.integer) else raw), raw


def speed_parts(pose, parts=SPEED_PARTS):
    """pose [N, W, J, 3] -> [N, 3] = [root speed, first part, mean of the other parts].  The reference's
    `centered[:, part[0]:part[0]+1]` subtraction indexes the window axis and cancels under the frame difference, so it is left
    out (it only exists for W > part[0]).  With a single part the reference's mean over no limbs is NaN; the kernel defines 0."""
    root_spd = torch.sqrt((torch.diff(pose[..., 0, :], dim=-2) ** 2).sum(-1)).mean(-1)
    centered = pose - pose[..., 0:1, :]
    sp = [torch.sqrt((torch.diff(centered[..., list(part[1:]), :], dim=-3) ** 2).sum(-1)).mean(dim=(-1, -2)) for part in parts]
    limbs = torch.stack(sp[1:], dim=-1).mean(-1) if len(sp) > 1 else torch.zeros_like(root_spd)
    return torch.stack([root_spd, sp[0], limbs], dim=-1)


def speed_outliers(pose, threshold):
    """get_speed_outliers: (indices of the windows whose mean keypoint speed exceeds `threshold`, the speeds)"""
    spd = torch.sqrt((torch.diff(pose, dim=-3) ** 2).sum(-1)).mean(dim=(-1, -2))
    return torch.where(spd > threshold)[0], spd


def frame_yaw(pose):
    """pose [N, J, 3] -> yaw [N, 1]"""
    fwd = _unit(pose[:, 1] - pose[:, 0])
    return -torch.atan2(fwd[:, 1], fwd[:, 0])[:, None]


def restate(pose, tree, offset, keys=ALL_KEYS, direction_process="midfwd", parts=SPEED_PARTS, dt=torch.float64):
    """preprocess_windows on pose [N, W, J, 3] (fp64 tensor) with the quaternion helpers and forward kinematics in `dt`.  Returns
    tensors in `dt` (the reference stores float32) plus `yaw` and `offsets_raw` in fp64."""
    pose = torch.as_tensor(pose, dtype=torch.float64)
    N, W, J = pose.shape[:3]
    flat = pose.reshape(N * W, J, 3)
    out = {}
    if "avg_speed_3d" in keys:
        out["avg_speed_3d"] = speed_parts(pose, parts)
    yaw = frame_yaw(pose[:, W // 2])
    if "heading" in keys:
        out["heading"] = torch.cat([torch.sin(yaw), torch.cos(yaw)], dim=-1)
    root = pose[..., 0, :].clone()
    if direction_process in ("midfwd", "x360"):
        root[..., :2] -= root[:, W // 2, :2][:, None, :].clone()
    if "x6d" in keys or "target_pose" in keys:
        local = inv_kin(flat, tree, offset, dt).reshape(N, W, J, 4)
        if direction_process == "midfwd":
            fwd = torch.zeros(N, 4, dtype=torch.float64)
            fwd[:, 0], fwd[:, 3] = torch.cos(yaw / 2)[:, 0], torch.sin(yaw / 2)[:, 0]
            fwd = fwd[:, None, :].expand(N, W, 4).to(dt)
            local[..., 0, :] = P.qmul(fwd, local[..., 0, :].clone())
            if "root" in keys:
                root = P.qrot(fwd, root.to(dt))
        out["x6d"] = P.quaternion_to_cont6d(local)
    if "offsets" in keys or "target_pose" in keys:
        offs, raw = segment_len(flat, tree, offset)
        out["offsets"], out["offsets_raw"] = offs.reshape(pose.shape), raw.reshape(pose.shape)
    if "root" in keys:
        out["root"] = root
    out = {k: (v if k == "offsets_raw" else v.to(dt)) for k, v in out.items()}
    if "target_pose" in keys:  # the target pose's root does not move
        tp = O.fwd_kin(out["x6d"].reshape(N * W, J, 6), tree, out["offsets"].reshape(N * W, J, 3), torch.zeros(N * W, 3, dtype=dt), eps=1e-8)
        out["target_pose"] = tp.reshape(N, W, J, 3)
    out["yaw"] = yaw
    return out


# ------------------------------------------------------------------------------------------------ conditioning
def kappa(pose, tree, offset):
    """(kappa, kappa_pos) [N, W, J] in fp64.  kappa of an x6d entry: 1 / cos(theta_root / 2) plus the sum of 1 / cos(theta_b / 2)
    over the bones from the start of the joint's chain down to the joint; theta_b is the angle between bone b and its unit
    offset, theta_root the angle between pose[0] - pose[1] and +x.  kappa_pos of a target_pose entry adds the kappa_pos of the
    joint its chain starts from: the position of a joint is the sum of the rotated offsets along its whole path from joint 0,
    which for the chains that start at joint 1 or 5 is longer than the chain itself."""
    pose = torch.as_tensor(pose, dtype=torch.float64)
    J = pose.shape[-2]
    off = torch.as_tensor(np.array(offset), dtype=torch.float64)
    amp = lambda c: 1.0 / torch.sqrt(torch.clamp((1.0 + c) / 2.0, min=0.0))  # 1 / cos(theta / 2) from cos(theta)
    root = amp(_unit(pose[..., 0, :] - pose[..., 1, :])[..., 0])
    kap = torch.zeros(pose.shape[:-1], dtype=torch.float64)
    kpos = torch.zeros_like(kap)
    kap[..., 0] = root
    kpos[..., 0] = root
    for chain in tree:  # the chains are ordered so that a chain's first joint is placed before the chain is walked
        acc = root.clone()
        for a, b in zip(chain[:-1], chain[1:]):
            acc = acc + amp((_unit(pose[..., b, :] - pose[..., a, :]) * _unit(off[b])).sum(-1))
            kap[..., b] = acc
            kpos[..., b] = acc + (kpos[..., chain[0]] if chain[0] != 0 else 0.0)
    return kap, kpos


def bucket_shares(kap):
    k = kap.reshape(-1)
    return [float(((k >= lo) & (k < hi)).double().mean()) for lo, hi in zip(EDGES[:-1], EDGES[1:])]


# ------------------------------------------------------------------------------------------------ the bounds
def _cpu64(t):
    return torch.as_tensor(t).detach().cpu().double()


def same_pattern(name, got, t64, t32=None):
    """the non-finite entries of `got` (and of the fp32 restatement) are exactly those of the truth; returns the finite mask"""
    fin = torch.isfinite(_cpu64(t64))
    assert torch.equal(torch.isfinite(_cpu64(got)), fin), (name, "non-finite pattern", int((~fin).sum()),
                                                          int((~torch.isfinite(_cpu64(got))).sum()))
    if t32 is not None:
        assert torch.equal(torch.isfinite(_cpu64(t32)), fin), (name, "fp32 restatement's non-finite pattern")
    return fin


def gate_finite(name, got, t64, t32, denom=None):
    """latent_checks.gate on the entries where the truth is finite; the others are compared by pattern"""
    fin = same_pattern(name, got, t64, t32)
    z = lambda t: torch.where(fin, _cpu64(t), torch.zeros((), dtype=torch.float64))
    return gate(name, z(got), z(t64), z(t32), denom)


def gate_buckets(name, got, t64, t32, kap, relative=False, select=None):
    """per kappa bucket:  max |kernel - fp64|  <=  max(FACTOR * max |fp32 restatement - fp64|, FLOOR), both maxima over the finite
    entries [..., J, C] of that bucket (restricted to `select` [..., J] if given); relative: in units of the truth's max-norm.
    Prints one GATE line per non-empty bucket, then asserts all of them.  Returns {bucket: (err, e32)}."""
    got, t64, t32 = _cpu64(got), _cpu64(t64), _cpu64(t32)
    fin = same_pattern(name, got, t64, t32)
    d = float(t64[fin].abs().max()) if relative else 1.0
    assert d > 0 and math.isfinite(d), (name, d)
    zero = torch.zeros((), dtype=torch.float64)
    err = torch.where(fin, (got - t64).abs(), zero).amax(-1) / d
    e32 = torch.where(fin, (t32 - t64).abs(), zero).amax(-1) / d
    use = fin.any(-1) if select is None else (fin.any(-1) & select)
    kap = torch.nan_to_num(kap, nan=math.inf)  # a degenerate bone elsewhere in the frame: the last bucket
    res, bad = {}, []
    for lo, hi in zip(EDGES[:-1], EDGES[1:]):
        sel = use & (kap >= lo) & ((kap < hi) | (hi == math.inf))
        if not bool(sel.any()):
            continue
        e, y = float(err[sel].max()), float(e32[sel].max())
        bound = max(FACTOR * y, FLOOR)
        print(f"GATE {name} kappa [{lo:g},{hi:g}): share {float(sel.double().mean()):.2e} err {e:.3e} e32 {y:.3e} bound {bound:.3e} "
              f"err/e32 {e / max(y, 2.0 ** -24):.2f}")
        res[(lo, hi)] = (e, y)
        if not (math.isfinite(e) and e <= bound):
            bad.append((name, lo, hi, e, y, bound))
    assert not bad, bad
    return res


def trunc_clear(raw):
    """mask of the entries of raw = len * OFFSET (fp64) that are at least TRUNC_CLEAR * max(1, |v|) away from the nearest step of
    trunc().  trunc is constant on (-1, 1), so its steps are the non-zero integers: an exact 0 (OFFSET component 0) is clear."""
    n = torch.round(raw)
    n = torch.where(n == 0, torch.where(raw < 0, -torch.ones_like(raw), torch.ones_like(raw)), n)
    return (raw - n).abs() >= TRUNC_CLEAR * torch.clamp(raw.abs(), min=1.0)


def gate_trunc(name, got, t64, raw):
    """integer OFFSET: exact equality wherever the untruncated fp64 value is clear of a truncation step, |kernel - fp64| <= 1 on the
    entries left out, which may be at most TRUNC_SHARE of all"""
    got, t64 = _cpu64(got), _cpu64(t64)
    clear = trunc_clear(raw)
    share = float((~clear).double().mean())
    wrong = int((got[clear] != t64[clear]).sum())
    worst = float((got - t64)[~clear].abs().max()) if share > 0 else 0.0
    print(f"GATE {name}: truncated, left out {share:.2e} of {clear.numel()} (max dev there {worst:g}), unequal elsewhere {wrong}")
    assert share <= TRUNC_SHARE, (name, share)
    assert bool(torch.isfinite(got).all()) and wrong == 0 and worst <= 1.0, (name, wrong, worst)
    return clear


def gate_all(name, got, pose, tree, offset, direction_process, parts, t64=None, t32=None, frames=None):
    """gate every key of `got` (x6d, offsets, root, heading, target_pose, avg_speed_3d; any subset) against the restatement.
    frames [N, W] bool: restrict the x6d / target_pose gates to these frames (the pattern check still covers all)."""
    int_offset = np.issubdtype(np.array(offset).dtype, np.integer)
    if t64 is None:
        t64 = restate(pose, tree, offset, ALL_KEYS, direction_process, parts, torch.float64)
        t32 = restate(pose, tree, offset, ALL_KEYS, direction_process, parts, torch.float32)
    kap, kpos = kappa(pose, tree, offset)
    sel = None if frames is None else frames[..., None].expand(kap.shape)
    res = {}
    if "x6d" in got:
        res["x6d"] = gate_buckets(name + " x6d", got["x6d"], t64["x6d"], t32["x6d"], kap, select=sel)
    clear = None
    if "offsets" in got:
        if int_offset:
            clear = gate_trunc(name + " offsets", got["offsets"], t64["offsets"], t64["offsets_raw"])
        else:
            gate_finite(name + " offsets", got["offsets"], t64["offsets"], t32["offsets"])
    if "target_pose" in got:
        # a frame whose truncated lengths were left out above may legitimately carry another length: its FK is not compared
        ok = sel
        if clear is not None:
            ok = clear.all(-1).all(-1, keepdim=True).expand(kap.shape)
            ok = ok if sel is None else (ok & sel)
        res["target_pose"] = gate_buckets(name + " target_pose", got["target_pose"], t64["target_pose"], t32["target_pose"], kpos,
                                          relative=True, select=ok)
    for k in ("root", "heading", "avg_speed_3d"):
        if k in got:
            gate_finite(f"{name} {k}", got[k], t64[k], t32[k])
    return res


# ------------------------------------------------------------------------------------------------ inputs of the further tests
E2E = dict(J=18, window=51, stride=3, runs=(200, 30, 150))  # the middle id run is shorter than the window and yields none


def e2e_inputs():
    """raw pose [frames, J, 3] (fp64 holding fp32 values), ids [frames], the window index rows, the fp64 mean keypoint speed of
    every window and a speed threshold in the widest gap of the middle half of the sorted speeds (some windows go, some stay)"""
    frames = sum(E2E["runs"])
    pose = make_pose(1, frames, E2E["J"], seed=11)[0]
    ids = np.concatenate([np.full(n, 3 + 2 * i) for i, n in enumerate(E2E["runs"])])
    win = torch.from_numpy(np.ascontiguousarray(P.get_window_indices(ids, E2E["stride"], E2E["window"])))
    _, spd = speed_outliers(pose[win], 0.0)
    s = torch.sort(spd).values
    q = len(s) // 4
    i = q + int(torch.argmax(s[q + 1:len(s) - q] - s[q:len(s) - q - 1]))
    return pose, ids, win, spd, float(0.5 * (s[i] + s[i + 1]))


DEGENERATE = dict(N=200, W=64, J=18,
                  opposed=(5, 10, 2, 3),    # window, frame, bone a -> b set exactly against OFFSET[b] = +x: joints 3, 4 of the frame
                  coincident=(5, 40, 6, 7),  # joint 7 placed on joint 6 (same tile as the above): joints 7, 8 of the frame
                  root_back=(9, 20),         # pose[0] - pose[1] exactly along -x in a frame that is not the middle one: the whole frame
                  root_mid=(12, 32))         # joints 0 and 1 coincide in the middle frame: no yaw for the whole window


def degenerate_pose():
    """random 200 x 64 x 18 windows with four planted degenerate frames.  The planted differences are exact in fp32 and fp64 (the
    other two components are equal, so the normalised bone is exactly -+ the axis whatever the rounding of the third), hence
    w = |u||v| + u.v is exactly 0 in both and the reference's arithmetic yields 0 / 0."""
    d = DEGENERATE
    pose = make_pose(d["N"], d["W"], d["J"], seed=3).clone()
    n, f, a, b = d["opposed"]
    pose[n, f, b] = pose[n, f, a] - torch.tensor([0.75, 0.0, 0.0], dtype=torch.float64)
    n, f, a, b = d["coincident"]
    pose[n, f, b] = pose[n, f, a]
    n, f = d["root_back"]
    pose[n, f, 1] = pose[n, f, 0] + torch.tensor([0.75, 0.0, 0.0], dtype=torch.float64)
    n, f = d["root_mid"]
    pose[n, f, 1] = pose[n, f, 0]
    return r32(pose)
