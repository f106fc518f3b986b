"""Training batches built on the device from a pose recording that stays resident in HBM.

The reference feeds `train()` from a dataset of preprocessed windows in host memory (`MouseDataset` behind a torch
`DataLoader`): 56 KB per window at W=64, J=18, about 130 times the recording it was cut from, gathered and copied to the
device every step.  Here the raw recording [frames, J, 3] (216 B per frame) is uploaded once and every batch is computed from
it for the window indices of that step: csrc/preprocess.hip's kernels read their windows through a table of first frames
(svae_window_batch, svae_window_speed_parts), the pose-tail kernel turns x6d / offsets into target_pose.  On the same windows
the tensors are bit-identical to `preprocess_pose`'s.

    window_starts, shard_order   host bookkeeping (no GPU)
    DeviceRecording              the dataset: `loader.dataset` for train() / test_epoch / decodability_metrics
    DeviceWindowLoader           the loader: yields one dict of device tensors per step
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Mapping

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import synthetic
from .preprocess import SPEED_PARTS

IK_KEYS = ("x6d", "offsets", "root", "heading", "target_pose")
OUTLIER_CHUNK = 16384  # windows per evaluation of the outlier speed (at most 65,536: nothing of dataset size is materialised)


def window_starts(ids, stride, window):
    """First frames of `get_window_indices(ids, stride, window)`'s rows, in the same order and with the same skipping of id runs
    shorter than the window; row i of that array is `window_starts(...)[i] + arange(window)`.  -> int64 [n] (host)."""
    ids = np.asarray(ids)
    if len(ids) == 0:
        return torch.zeros(0, dtype=torch.int64)
    change = np.concatenate([[0], np.where(np.diff(ids, prepend=ids[0]) != 0)[0], [len(ids)]])
    out = [np.zeros(0, dtype=np.int64)]
    for lo, hi in zip(change[:-1], change[1:]):
        if hi - lo >= window:
            out.append(np.arange(lo, hi - window + 1, stride, dtype=np.int64))
        else:
            print("ID {} length smaller than window size - skipping ...".format(ids[lo]))
    return torch.from_numpy(np.concatenate(out))


def shard_order(n, batch_size, shuffle, seed, epoch, rank=0, world=1):
    """Dataset indices one rank visits in one epoch, int64 [n // world] (host).  The order of the whole set is arange(n), or a
    permutation drawn from a host generator seeded with (seed, epoch), hence the same on every rank; rank r takes every
    world-th entry from the r-th on, cut to n // world, so that all ranks run the same number of steps on disjoint shards and
    at most world - 1 windows sit an epoch out."""
    if batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError("shard_order: batch_size {}, rank {} of {}".format(batch_size, rank, world))
    if shuffle:
        g = torch.Generator().manual_seed((int(seed) * 1000003 + int(epoch)) % (2 ** 63))
        order = torch.randperm(n, generator=g)
    else:
        order = torch.arange(n)
    return order[rank::world][: n // world].contiguous()


class _WindowBatch(Mapping):
    """Read-only mapping over a recording's data keys for one set of windows; each value is computed on the device the first
    time it is asked for (the heading of the whole set does not build its x6d)."""

    def __init__(self, rec, index, squeeze):
        self._rec, self._index, self._squeeze = rec, index, squeeze
        self._starts = rec.starts[index]
        self._built = {}

    def __iter__(self):
        return iter(self._rec.data_keys)

    def __len__(self):
        return len(self._rec.data_keys)

    def __getitem__(self, key):
        if key not in self._rec.data_keys:
            raise KeyError(key)
        if key not in self._built:
            self._rec._build(key, self._starts, self._index, self._built)
        v = self._built[key]
        return v[0] if self._squeeze else v


class DeviceRecording:
    """A pose recording [frames, J, 3] resident on the device, seen as the dataset of its windows.

    `pose`, `ids` [frames] and the arguments up to `direction_process` are `preprocess_pose`'s, and window i of this dataset is
    window i of its result (the same windows, cut at the same strides inside the id runs, the speed outliers dropped by the same
    expression).  `norm_params["avg_speed_3d"]` = {"mean", "std"} (3 values each) normalises avg_speed_3d as the reference's
    `mouse_data` does.  Carries what train() reads from `loader.dataset`."""

    def __init__(self, pose, ids, skeleton_config, window, stride=2, data_keys=("x6d", "root", "offsets"), speed_threshold=2.25,
                 direction_process="midfwd", norm_params=None, arena_size=None, discrete_classes=None, label="train",
                 device="cuda", speed_parts=SPEED_PARTS):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceRecording builds its batches with HIP kernels: device {!r} is not a GPU".format(str(device)))
        self.window, self.stride, self.direction_process = int(window), int(stride), direction_process
        self.data_keys = list(data_keys)
        self.kinematic_tree, self.offset = skeleton_config["KINEMATIC_TREE"], skeleton_config["OFFSET"]
        self.speed_parts = [list(p) for p in speed_parts]
        self.norm_params, self.discrete_classes, self.label = norm_params, discrete_classes, label
        self.arena_size = torch.tensor(arena_size) if arena_size is not None else None
        self.pose = torch.as_tensor(np.asarray(pose), dtype=torch.float32).to(self.device).contiguous()
        self.frames, self.n_keypts = int(self.pose.shape[0]), int(self.pose.shape[1])
        off = np.array(self.offset)
        self._truncate = int(np.issubdtype(off.dtype, np.integer))  # an integer OFFSET array truncates the segment lengths
        self._uoff = (C.c_float * (3 * self.n_keypts))(*[float(v) for v in off.reshape(-1)])
        self._tree = _lib.make_tree(self.n_keypts, self.kinematic_tree)
        flat = [j for part in self.speed_parts for j in part]
        self._parts = (C.c_int * len(flat))(*flat)
        self._part_len = (C.c_int * len(self.speed_parts))(*[len(p) for p in self.speed_parts])
        self._norm = None
        if norm_params is not None and "avg_speed_3d" in norm_params:
            self._norm = tuple((C.c_float * 3)(*[float(v) for v in norm_params["avg_speed_3d"][k]]) for k in ("mean", "std"))
        starts = window_starts(ids, self.stride, self.window).to(self.device)
        if speed_threshold is not None:
            starts = starts[self._within_speed(starts, speed_threshold)]
        self.starts = starts
        mid_ids = torch.as_tensor(np.asarray(ids))[(starts + self.window // 2).cpu()]
        self.window_labels = {"ids": mid_ids.to(torch.int16).to(self.device)}  # per-window tensors served by index

    def _within_speed(self, starts, threshold):
        """mask of the windows `get_speed_outliers` keeps: its expression on the gathered windows, a chunk at a time"""
        frame = torch.arange(self.window, device=self.device)
        keep = []
        for lo in range(0, len(starts), OUTLIER_CHUNK):
            win = self.pose[starts[lo: lo + OUTLIER_CHUNK, None] + frame]
            spd = torch.sqrt((torch.diff(win, n=1, dim=-3) ** 2).sum(dim=-1)).mean(dim=(-1, -2))
            keep.append(~(spd > threshold))
        keep = torch.cat(keep) if keep else torch.ones(0, dtype=torch.bool, device=self.device)
        print("Outlier frames above {}: {}".format(threshold, int((~keep).sum())))
        return keep

    def __len__(self):
        return int(self.starts.shape[0])

    def __getitem__(self, idx):
        n = len(self)
        if isinstance(idx, slice):
            return _WindowBatch(self, torch.arange(n, device=self.device)[idx], False)
        if torch.is_tensor(idx) or isinstance(idx, (list, tuple, np.ndarray)):
            index = torch.as_tensor(idx)
            if index.dtype == torch.bool or index.is_floating_point() or index.dim() != 1:
                raise IndexError("DeviceRecording takes an int, a slice or a 1-D integer tensor")
            index = index.to(torch.int64)
            if index.numel() and (int(index.min()) < -n or int(index.max()) >= n):
                raise IndexError("index out of range for {} windows".format(n))
            index = index.to(self.device)
            return _WindowBatch(self, torch.where(index < 0, index + n, index), False)
        i = int(idx)
        if not -n <= i < n:
            raise IndexError("index {} out of range for {} windows".format(i, n))
        return _WindowBatch(self, torch.tensor([i % n], device=self.device), True)

    # ------------------------------------------------------------------------------------------- the device side
    def _window_batch(self, starts, index, window, want):
        """svae_window_batch for rows of `window` frames from `starts` -> dict with x6d and the keys of `want`"""
        B, J, dev = int(starts.shape[0]), self.n_keypts, self.device
        out = {"x6d": torch.empty(B, window, J, 6, device=dev)}
        if "offsets" in want:
            out["offsets"] = torch.empty(B, window, J, 3, device=dev)
        if "root" in want:
            out["root"] = torch.empty(B, window, 3, device=dev)
        if "heading" in want:
            out["heading"] = torch.empty(B, 2, device=dev)
        p = lambda k: out[k].data_ptr() if k in out else None
        dp = self.direction_process
        if B == 0:
            return out
        check(_lib.lib().svae_window_batch(self.pose.data_ptr(), self.frames, starts.data_ptr(), None if index is None else index.data_ptr(),
                                           self._uoff, C.byref(self._tree), window, int(dp == "midfwd"), int(dp in ("midfwd", "x360")),
                                           self._truncate, p("x6d"), p("offsets"), p("root"), p("heading"), B, ops._stream()),
              "window_batch")
        return out

    def _build(self, key, starts, index, built):
        """compute `key` (and what comes out of the same launch) for the windows `index` into `built`"""
        starts, index = starts.contiguous(), index.contiguous()
        if key in self.window_labels:
            built[key] = self.window_labels[key][index]
        elif key == "avg_speed_3d":
            out = torch.empty(len(starts), 3, device=self.device)
            mean, std = self._norm if self._norm is not None else (None, None)
            if len(starts):
                check(_lib.lib().svae_window_speed_parts(self.pose.data_ptr(), self.frames, starts.data_ptr(), self._parts,
                                                         self._part_len, len(self.speed_parts), self.window, self.n_keypts, mean, std,
                                                         out.data_ptr(), len(starts), ops._stream()), "window_speed_parts")
            built[key] = out
        elif key == "heading" and "x6d" not in built:
            # [sin, cos] of the middle frame's yaw: that frame as a window of its own (its x6d is 1 / window of the set's)
            built[key] = self._window_batch(starts + self.window // 2, None, 1, ("heading",))["heading"]
        elif key in IK_KEYS:
            if "x6d" not in built:
                want = [k for k in ("offsets", "root", "heading") if k in self.data_keys and k not in built]
                if "target_pose" in self.data_keys and "offsets" not in want:
                    want.append("offsets")
                built.update(self._window_batch(starts, index, self.window, want))
            if key == "target_pose":  # its root does not move (dataset.py:429-441)
                built[key] = (synthetic.fwd_kin_cont6d(built["x6d"], self.kinematic_tree, built["offsets"]) if len(starts)
                              else torch.empty_like(built["offsets"]))
            elif key not in built:  # asked for outside data_keys' launch: cannot happen through the mapping
                raise KeyError(key)
        else:
            raise KeyError("{!r}: not a key DeviceRecording computes, nor one of its window_labels".format(key))

    def batch(self, index):
        """every data key for the windows `index` (int64 on the device, in range) as a plain dict: one loader step"""
        starts, built = self.starts[index], {}
        for k in self.data_keys:
            if k not in built:
                self._build(k, starts, index, built)
        return {k: built[k] for k in self.data_keys}


class DeviceWindowLoader:
    """Iterates a DeviceRecording in batches built on the device, on the caller's current stream: `len(loader)` steps of
    `shard_order`'s indices per epoch, the last one possibly short.  The permutation of epoch e depends on (seed, e) alone;
    `set_epoch(e)` names the next epoch, otherwise it advances by one per iteration (starting at 0)."""

    def __init__(self, dataset, batch_size, shuffle=False, seed=0, rank=0, world=1):
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("DeviceWindowLoader: batch_size {}, rank {} of {}".format(batch_size, rank, world))
        self.dataset, self.batch_size, self.shuffle, self.seed = dataset, int(batch_size), shuffle, seed
        self.rank, self.world = rank, world
        self.epoch, self._next_epoch = -1, None

    def __len__(self):
        return -(-(len(self.dataset) // self.world) // self.batch_size)

    def set_epoch(self, epoch):
        self._next_epoch = int(epoch)

    def __iter__(self):
        self.epoch = self.epoch + 1 if self._next_epoch is None else self._next_epoch
        self._next_epoch = None
        order = shard_order(len(self.dataset), self.batch_size, self.shuffle, self.seed, self.epoch, self.rank, self.world)
        order = order.to(self.dataset.device)
        for lo in range(0, len(order), self.batch_size):
            yield self.dataset.batch(order[lo: lo + self.batch_size])
