"""Training batches built on the device from a resident recording (scrubvae_amd.data.recording, svae_window_batch and
svae_window_speed_parts in csrc/preprocess.hip, get.device_data) against `preprocess_pose` on the same inputs -- equality bit for
bit -- and, through tests/preprocess_checks.py, against the fp64 restatement, so that the check does not rest on the older kernel
alone.

The recordings are chosen by what they make the 64-frame-tile kernel do:
    380 x 18, W 51, stride 3, midfwd float   three id runs (one too short); rows straddle the tiles, the middle frame lies in
                                             another tile, the last window ends on the recording's last frame
    700 x 23, W 256, stride 7, x360 float    four tiles per row, 70,912 + 512 B of LDS, the padded input of the forward kinematics
    15 x 23, W 2, stride 1, None int         rows of two frames, truncated segment lengths, no centring and no rotation
    130 x 8, W 33, stride 2, midfwd float    one chain (the second wave idles), one speed part (limbs = 0)"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import preprocess_checks as PC
from tests.preprocess_checks import SENTINEL

pytestmark = pytest.mark.gpu

GUARD = 3  # sentinel rows behind every output buffer of the direct C ABI calls
KEYS = list(PC.ALL_KEYS) + ["ids"]
ONE_PART = ([0, 1, 2, 3, 4, 5, 6, 7],)


@pytest.fixture(scope="module")
def M():
    """the modules under test"""
    from types import SimpleNamespace
    from scrubvae_amd import _lib, get
    from scrubvae_amd.data import preprocess, recording
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return SimpleNamespace(PP=preprocess, R=recording, lib=_lib, get=get)


def skeleton(J, kind):
    tree, offset = PC.skeleton(J, kind)
    return {"KINEMATIC_TREE": tree, "OFFSET": offset}


def two_runs(runs, J, seed):
    """raw pose [frames, J, 3] (fp64 holding fp32 values) and ids of id runs of the given lengths"""
    pose = PC.make_pose(1, sum(runs), J, seed=seed)[0]
    return pose, np.concatenate([np.full(n, 2 + 3 * i) for i, n in enumerate(runs)])


def gap_threshold(pose, ids, W, stride):
    """PC.e2e_inputs' choice: the middle of the widest gap in the middle half of the sorted window speeds"""
    win = torch.from_numpy(np.ascontiguousarray(PC.P.get_window_indices(ids, stride, W)))
    s = torch.sort(PC.speed_outliers(pose[win], 0.0)[1]).values
    q = len(s) // 4
    i = q + int(torch.argmax(s[q + 1:len(s) - q] - s[q:len(s) - q - 1]))
    return float(0.5 * (s[i] + s[i + 1]))


def both(M, pose, ids, skel, W, stride, direction, thr, keys=KEYS, **kw):
    """-> (preprocess_pose's dict, the DeviceRecording) on the same inputs"""
    want = M.PP.preprocess_pose(pose.numpy(), ids, skel, W, stride, data_keys=[k for k in keys if k in KEYS], speed_threshold=thr,
                                direction_process=direction)
    ds = M.R.DeviceRecording(pose.numpy(), ids, skel, W, stride, data_keys=keys, speed_threshold=thr, direction_process=direction, **kw)
    torch.cuda.synchronize()
    return want, ds


def same(got, want, keys):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert torch.equal(got[k], want[k]), k


@pytest.fixture(scope="module")
def e2e(M):
    """PC.e2e_inputs() through both routes, once: (pose, ids, skeleton, threshold, preprocess_pose's dict, the DeviceRecording)"""
    pose, ids, win, spd, thr = PC.e2e_inputs()
    skel = skeleton(PC.E2E["J"], "float")
    want, ds = both(M, pose, ids, skel, PC.E2E["window"], PC.E2E["stride"], "midfwd", thr)
    assert 0 < int((spd <= thr).sum()) < len(win) == 84
    return pose, ids, skel, thr, want, ds


# ------------------------------------------------------------------------------------------------ 1. equality with preprocess_pose
def test_equals_preprocess_pose(e2e):
    pose, ids, skel, thr, want, ds = e2e
    assert len(ds) == want["raw_pose"].shape[0] and 0 < len(ds) < 84
    assert (ds.n_keypts, ds.kinematic_tree, ds.label, ds.data_keys) == (18, skel["KINEMATIC_TREE"], "train", KEYS)
    got = ds[:]
    assert list(got) == KEYS and len(got) == len(KEYS)
    same(got, want, KEYS)
    PC.gate_all("recording", {k: got[k] for k in PC.ALL_KEYS}, want["raw_pose"].cpu().double(), skel["KINEMATIC_TREE"], skel["OFFSET"],
                "midfwd", PC.SPEED_PARTS)


# ------------------------------------------------------------------------------------------------ 2. the identity-quirk row
def test_identity_row_follows_dataset_index_zero(M, e2e):
    pose, ids, skel, thr, want, ds = e2e
    n = len(ds)
    idx = [7, 3, 3, 0, n - 1, 1]
    got = ds[torch.tensor(idx)]
    same(got, {k: want[k][idx] for k in KEYS}, KEYS)
    assert torch.equal(got["x6d"][3, 0, 0], want["x6d"][0, 0, 0])
    assert torch.equal(got["x6d"][0, 0], want["x6d"][7, 0])
    # the gathered windows through svae_inv_kin put the identity on batch row 0 instead: this is what the index table is for
    naive = M.PP.inv_kin_windows(want["raw_pose"][idx], skel["KINEMATIC_TREE"], skel["OFFSET"], "midfwd")[0]
    assert not torch.equal(naive[0, 0, 0], want["x6d"][7, 0, 0]) and not torch.equal(naive[3, 0, 0], want["x6d"][0, 0, 0])
    assert torch.equal(naive[1:3], got["x6d"][1:3]) and torch.equal(naive[4:], got["x6d"][4:])


def test_indexing(e2e):
    pose, ids, skel, thr, want, ds = e2e
    n = len(ds)
    same(ds[2:n:5], {k: want[k][2:n:5] for k in KEYS}, KEYS)
    same(ds[5], {k: want[k][5] for k in KEYS}, KEYS)
    same(ds[-1], {k: want[k][n - 1] for k in KEYS}, KEYS)
    same(ds[torch.tensor([-n, n - 1], device="cuda")], {k: want[k][[0, n - 1]] for k in KEYS}, KEYS)
    assert ds[0:0]["x6d"].shape == (0, 51, 18, 6) and ds[0:0]["avg_speed_3d"].shape == (0, 3)
    for bad in (n, -n - 1, torch.tensor([0, n]), torch.tensor([-n - 1]), torch.tensor([0.5]), torch.tensor([True, False])):
        with pytest.raises(IndexError):
            ds[bad]
    with pytest.raises(KeyError):
        ds[:]["raw_pose"]
    with pytest.raises(TypeError):
        ds[:]["x6d"] = None


# ------------------------------------------------------------------------------------------------ 3. further geometries
GEOMETRIES = [
    # runs, J, W, stride, direction, OFFSET kind, speed parts, seed
    ((400, 300), 23, 256, 7, "x360", "float", PC.SPEED_PARTS, 21),
    ((9, 6), 23, 2, 1, None, "int", PC.SPEED_PARTS, 22),
    ((80, 50), 8, 33, 2, "midfwd", "float", ONE_PART, 23),
]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "{}x{}-W{}-{}-{}".format(sum(g[0]), g[1], g[2], g[4], g[5]))
def test_geometries(M, geo):
    runs, J, W, stride, direction, kind, parts, seed = geo
    pose, ids = two_runs(runs, J, seed)
    skel = skeleton(J, kind)
    thr = gap_threshold(pose, ids, W, stride)
    # preprocess_pose computes the speeds of the 18-joint parts only: with one part they come from get_speed_parts itself
    keys = KEYS if parts is PC.SPEED_PARTS else [k for k in KEYS if k != "avg_speed_3d"]
    want, ds = both(M, pose, ids, skel, W, stride, direction, thr, keys=keys, speed_parts=parts)
    n_all = sum((n - W) // stride + 1 for n in runs)
    assert len(ds) == want["raw_pose"].shape[0] and 0 < len(ds) < n_all
    got = dict(ds[:])
    same(got, want, keys)
    if parts is not PC.SPEED_PARTS:
        ds = M.R.DeviceRecording(pose.numpy(), ids, skel, W, stride, data_keys=["avg_speed_3d"], speed_threshold=thr,
                                 direction_process=direction, speed_parts=parts)
        got["avg_speed_3d"] = ds[:]["avg_speed_3d"]
        assert torch.equal(got["avg_speed_3d"], M.PP.get_speed_parts(want["raw_pose"], parts))
        assert float(got["avg_speed_3d"][:, 2].abs().max()) == 0.0
    PC.gate_all("recording", {k: got[k] for k in PC.ALL_KEYS}, want["raw_pose"].cpu().double(), skel["KINEMATIC_TREE"], skel["OFFSET"],
                direction, parts)


# ------------------------------------------------------------------------------------------------ 4. the loader
@pytest.fixture(scope="module")
def whole(M):
    """the 84-window set (no speed threshold) and its tensors"""
    pose, ids, _, _, _ = PC.e2e_inputs()
    ds = M.R.DeviceRecording(pose.numpy(), ids, skeleton(18, "float"), 51, 3, data_keys=KEYS, speed_threshold=None)
    assert len(ds) == 84
    return pose, ids, ds, dict(ds[:])


def test_loader_in_order(M, whole):
    pose, ids, ds, full = whole
    loader = M.R.DeviceWindowLoader(ds, 32)
    assert loader.dataset is ds and len(loader) == 3
    batches = list(loader)
    assert [len(b["x6d"]) for b in batches] == [32, 32, 20]
    assert all(type(b) is dict and list(b) == KEYS and all(v.is_cuda for v in b.values()) for b in batches)
    same({k: torch.cat([b[k] for b in batches]) for k in KEYS}, full, KEYS)


def test_loader_shuffled(M, whole):
    pose, ids, ds, full = whole
    loader = M.R.DeviceWindowLoader(ds, 32, shuffle=True, seed=5)
    loader.set_epoch(2)
    first = list(loader)
    order = M.R.shard_order(84, 32, True, 5, 2)
    assert len(first) == 3
    for i, b in enumerate(first):
        same(b, ds[order[32 * i: 32 * i + 32]], KEYS)
        same(b, {k: full[k][order[32 * i: 32 * i + 32].cuda()] for k in KEYS}, KEYS)
    loader.set_epoch(2)
    for a, b in zip(first, loader):
        same(a, b, KEYS)
    assert loader.epoch == 2
    nxt = list(loader)  # without set_epoch the epoch advances
    assert loader.epoch == 3
    same(nxt[0], ds[M.R.shard_order(84, 32, True, 5, 3)[:32]], KEYS)
    assert not torch.equal(nxt[0]["root"], first[0]["root"])
    fresh = M.R.DeviceWindowLoader(ds, 32, shuffle=True, seed=5)
    same(next(iter(fresh)), ds[M.R.shard_order(84, 32, True, 5, 0)[:32]], KEYS)


def test_loader_two_ranks(M, whole):
    pose, ids, ds, full = whole
    ranks = [list(M.R.DeviceWindowLoader(ds, 32, shuffle=True, seed=5, rank=r, world=2)) for r in range(2)]
    assert [len(r) for r in ranks] == [2, 2] == [len(M.R.DeviceWindowLoader(ds, 32, rank=r, world=2)) for r in range(2)]
    assert [[len(b["root"]) for b in r] for r in ranks] == [[32, 10], [32, 10]]
    orders = [M.R.shard_order(84, 32, True, 5, 0, r, 2) for r in range(2)]
    assert not set(orders[0].tolist()) & set(orders[1].tolist())
    for r in range(2):
        for i, b in enumerate(ranks[r]):
            same(b, ds[orders[r][32 * i: 32 * i + 32]], KEYS)
    rows = torch.cat([b["root"].reshape(len(b["root"]), -1) for r in ranks for b in r])
    assert len(torch.unique(rows, dim=0)) == 84 == len(rows)  # no window twice


def test_normalised_speed_and_factory(M, whole):
    pose, ids, ds, full = whole
    cfg = {"batch_size": 32, "direction_process": "midfwd", "arena_size": [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], "dataset": "4_mice"}
    loader = M.get.device_data(cfg, pose.numpy(), ids, skeleton(18, "float"), "val", data_keys=list(PC.ALL_KEYS), stride=3, window=51,
                               speed_threshold=None)
    d = loader.dataset
    assert isinstance(loader, M.R.DeviceWindowLoader) and len(loader) == 3 and len(d) == 84 and d.label == "val"
    mean = torch.tensor([0.4993, 0.7112, 0.6663], device="cuda")
    std = torch.tensor([0.4038, 0.3586, 0.4169], device="cuda")
    assert torch.equal(d.norm_params["avg_speed_3d"]["mean"], mean.cpu()) and torch.equal(d.norm_params["avg_speed_3d"]["std"], std.cpu())
    assert torch.equal(d[:]["avg_speed_3d"], (full["avg_speed_3d"] - mean) / std)
    same(d[:], full, [k for k in KEYS if k != "avg_speed_3d"])  # ids are served although not asked for, as mouse_data does
    assert torch.equal(d.discrete_classes["ids"].long(), torch.tensor([3, 7]))
    assert torch.equal(d.arena_size, torch.tensor(cfg["arena_size"])) and d.n_keypts == 18
    batches = list(loader)
    assert torch.equal(torch.cat([b["avg_speed_3d"] for b in batches]), d[:]["avg_speed_3d"])
    # "parkinsons": ids from 36 on are the lesioned animals' and come down by 36
    cfg["dataset"] = "parkinsons"
    ids_pd = np.where(ids == 7, 40, ids)
    d = M.get.device_data(cfg, pose.numpy(), ids_pd, skeleton(18, "float"), data_keys=["x6d", "pd_label"], stride=3, window=51,
                          speed_threshold=None).dataset
    lab = d[:]["pd_label"]
    assert lab.dtype == torch.int64 and lab.shape == (84, 1) and torch.equal(lab[:, 0].cpu(), (full["ids"] == 7).long().cpu())
    assert torch.equal(d[:]["ids"].long().cpu(), torch.where(full["ids"] == 7, 4, 3).long().cpu())
    assert torch.equal(d.discrete_classes["ids"], torch.arange(2)) and torch.equal(d.discrete_classes["pd_label"], torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        M.get.device_data(cfg, pose.numpy(), ids, skeleton(18, "float"), data_keys=["x6d", "fluorescence"])


# ------------------------------------------------------------------------------------------------ 5. the lazy mapping
def test_heading_alone_does_not_build_x6d(e2e):
    pose, ids, skel, thr, want, ds = e2e
    x6d_bytes = len(ds) * 51 * 18 * 6 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    heading = ds[:]["heading"]
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert torch.equal(heading, want["heading"])
    assert grown < x6d_bytes, (grown, x6d_bytes)


# ------------------------------------------------------------------------------------------------ 6. the C ABI, called directly
def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def only_sentinel(t):
    return t.numel() == 0 or bool((t == SENTINEL).all())


def uoff(offset):
    flat = [float(v) for row in offset for v in row]
    return (C.c_float * len(flat))(*flat)


class Abi:
    """the e2e recording on the device and the two entry points called into sentinel-filled buffers with GUARD rows behind what
    a call may write"""

    def __init__(self, M, ds, skel):
        self.lib, self.ds, self.W, self.J = M.lib, ds, ds.window, ds.n_keypts
        self.tree, self.uo = skel["KINEMATIC_TREE"], uoff(skel["OFFSET"])
        self.index = torch.arange(len(ds), device="cuda")

    def batch(self, B, want=("offsets", "root", "heading"), **kw):
        a = dict(pose=self.ds.pose.data_ptr(), frames=self.ds.frames, starts=self.ds.starts.data_ptr(), index=self.index.data_ptr(),
                 tree=self.lib.make_tree(self.J, self.tree), uo=self.uo, window=self.W, x6d=True, alloc=max(B, 0))
        a.update(kw)
        n, W, J = a["alloc"], self.W, self.J
        buf = dict(x6d=sentinel(n * W + GUARD, J, 6), offsets=sentinel(n * W + GUARD, J, 3), root=sentinel(n * W + GUARD, 3),
                   heading=sentinel(n + GUARD, 2))
        p = lambda k: buf[k].data_ptr() if (k == "x6d" and a["x6d"]) or k in want else None
        st = self.lib.lib().svae_window_batch(a["pose"], a["frames"], a["starts"], a["index"], a["uo"], C.byref(a["tree"]), a["window"], 1, 1,
                                              0, p("x6d"), p("offsets"), p("root"), p("heading"), B,
                                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return st, buf

    def speed(self, B, parts=PC.SPEED_PARTS, norm=(None, None), **kw):
        a = dict(pose=self.ds.pose.data_ptr(), frames=self.ds.frames, starts=self.ds.starts.data_ptr(), W=self.W, out=True)
        a.update(kw)
        flat = [j for part in parts for j in part]
        out = sentinel(max(B, 0) + GUARD, 3)
        st = self.lib.lib().svae_window_speed_parts(a["pose"], a["frames"], a["starts"], (C.c_int * len(flat))(*flat),
                                                    (C.c_int * len(parts))(*[len(q) for q in parts]), len(parts), a["W"], self.J,
                                                    norm[0], norm[1], out.data_ptr() if a["out"] else None, B,
                                                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return st, out


@pytest.fixture(scope="module")
def abi(M, e2e):
    pose, ids, skel, thr, want, ds = e2e
    return Abi(M, ds, skel)


def test_abi_buffer_discipline(M, e2e, abi):
    """the kept windows fill 49.4 tiles: nothing is written behind the last row, a null output changes no other output, and a
    batch of none launches nothing"""
    pose, ids, skel, thr, want, ds = e2e
    B, W = len(ds), ds.window
    st, full = abi.batch(B)
    assert st == 0, M.lib.last_error()
    rows = dict(x6d=B * W, offsets=B * W, root=B * W, heading=B)
    for k, n in rows.items():
        assert only_sentinel(full[k][n:]), k
        assert torch.equal(full[k][:n].reshape(want[k].shape), want[k]), k
    for sel in (("root", "heading"), ("offsets", "heading"), ("offsets", "root"), ()):
        st, part = abi.batch(B, want=sel)
        assert st == 0, M.lib.last_error()
        for k in rows:
            if k == "x6d" or k in sel:
                assert torch.equal(part[k], full[k]), (sel, k)
            else:
                assert only_sentinel(part[k]), (sel, k)
    st, none = abi.batch(B, index=None)  # no index table: no row carries the identity
    assert st == 0 and torch.equal(none["x6d"][1:], full["x6d"][1:]) and not torch.equal(none["x6d"][0, 0], full["x6d"][0, 0])
    st, spd = abi.speed(B)
    assert st == 0 and only_sentinel(spd[B:]) and torch.equal(spd[:B], want["avg_speed_3d"])
    mean, std = (C.c_float * 3)(0.5, 0.25, 2.0), (C.c_float * 3)(0.5, 3.0, 0.7)
    st, nrm = abi.speed(B, norm=(mean, std))
    dev = lambda a: torch.tensor(list(a), device="cuda")
    assert st == 0 and only_sentinel(nrm[B:]) and torch.equal(nrm[:B], (want["avg_speed_3d"] - dev(mean)) / dev(std))
    st, buf = abi.batch(0, alloc=4)
    assert st == 0 and all(only_sentinel(b) for b in buf.values())
    st, out = abi.speed(0)
    assert st == 0 and only_sentinel(out)


def test_abi_rejections(M, abi):
    """each returns its status with a message and launches nothing"""
    L = M.lib
    good = lambda: L.make_tree(abi.J, abi.tree)

    def rejected(res, status, text):
        st, bufs = res
        bufs = list(bufs.values()) if isinstance(bufs, dict) else [bufs]
        assert st == status, (st, text)
        assert text in L.last_error(), (L.last_error(), text)
        assert all(only_sentinel(b) for b in bufs), text

    rejected(abi.batch(4, pose=None), L.ERR_ARG, "window_batch: null pointer")
    rejected(abi.batch(4, starts=None), L.ERR_ARG, "window_batch: null pointer")
    rejected(abi.batch(4, x6d=False), L.ERR_ARG, "window_batch: null pointer")
    rejected(abi.batch(4, window=0), L.ERR_SHAPE, "window 0 < 1")
    rejected(abi.batch(4, frames=abi.W - 1), L.ERR_SHAPE, "shorter than window")
    rejected(abi.batch(-1), L.ERR_SHAPE, "batch -1 < 0")
    t = good()
    t.n_joints = 33
    rejected(abi.batch(4, tree=t), L.ERR_SHAPE, "window_batch: 33 joints")
    t = good()
    t.n_chains = 9
    rejected(abi.batch(4, tree=t), L.ERR_SHAPE, "window_batch: bad chain count")
    t = good()
    t.chain[0][1] = abi.J
    rejected(abi.batch(4, tree=t), L.ERR_SHAPE, "window_batch: joint index out of range")
    rejected(abi.speed(4, pose=None), L.ERR_ARG, "window_speed_parts: null pointer")
    rejected(abi.speed(4, starts=None), L.ERR_ARG, "window_speed_parts: null pointer")
    rejected(abi.speed(4, out=False), L.ERR_ARG, "window_speed_parts: null pointer")
    rejected(abi.speed(4, norm=((C.c_float * 3)(0, 0, 0), None)), L.ERR_ARG, "mean and std go together")
    rejected(abi.speed(4, W=1), L.ERR_SHAPE, "window_speed_parts: bad shape")
    rejected(abi.speed(4, frames=abi.W - 1), L.ERR_SHAPE, "shorter than window")
    rejected(abi.speed(-1), L.ERR_SHAPE, "batch -1 < 0")
    rejected(abi.speed(4, parts=([0, 1, abi.J],)), L.ERR_SHAPE, "window_speed_parts: joint index out of range")
    rejected(abi.speed(4, parts=([0, 1], [0, 2], [0, 3], [0, 4])), L.ERR_SHAPE, "window_speed_parts: bad shape")
    # and the same arguments, valid, still run
    st, buf = abi.batch(4)
    assert st == 0 and not bool((buf["x6d"][:4 * abi.W] == SENTINEL).any())


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_train_and_test_epoch_over_the_loader(M):
    from scrubvae_amd.train import trainer
    pose, ids, _, _, thr = PC.e2e_inputs()
    skel = skeleton(18, "float")
    keys = ["x6d", "root", "offsets", "target_pose", "avg_speed_3d", "heading", "ids"]
    cfg = {"batch_size": 32, "direction_process": "midfwd", "arena_size": [[-3.0, -3.0, -3.0], [3.0, 3.0, 3.0]], "dataset": "4_mice"}
    loader = M.get.device_data(cfg, pose.numpy(), ids, skel, "train", data_keys=keys, shuffle=True, stride=3, window=51, speed_threshold=thr)
    ds = loader.dataset
    dis = {"method": {"conditional": ["avg_speed_3d", "heading"]}, "alpha": 1.0, "features": ["avg_speed_3d", "heading"]}
    model_config = dict(type="rcnn", kernel=5, z_dim=8, window=51, activation="prelu", diag=True, init_dilation=None, prior="gaussian",
                        channel=[8, 16, 32, 64, 128])
    torch.manual_seed(0)
    model = M.get.model(model_config, None, None, dis, ds.n_keypts, "midfwd", arena_size=ds.arena_size, kinematic_tree=ds.kinematic_tree,
                        discrete_classes=ds.discrete_classes, device="cuda", verbose=0)
    config = {"loss": {"jpe": 1.0, "root": 1.0, "prior": 0.1}, "disentangle": dis, "data": cfg}
    steps = []
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    opt.register_step_post_hook(lambda *a: steps.append(1))
    metrics = trainer.train_test_epoch(config, model, loader, "cuda", 1, opt, None, "train")
    assert len(steps) == len(loader) == -(-len(ds) // 32)
    assert set(metrics) == {"total", "jpe", "root", "prior"} and all(np.isfinite(v) for v in metrics.values())
    test_metrics, z = trainer.test_epoch(config, model, loader, "cuda", 1)
    assert z.shape == (len(ds), 8) and bool(torch.isfinite(z).all())
    assert all(np.isfinite(test_metrics[k]) for k in ("total", "jpe", "root", "prior"))
