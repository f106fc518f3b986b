"""Host bookkeeping of scrubvae_amd.data.recording (window starts, the per-rank epoch order) and the declarations of its two
C entry points.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from tests import abi_header as ABI
from tests import preprocess_checks as PC


@pytest.fixture(scope="module")
def R():
    from scrubvae_amd.data import recording
    return recording


def test_window_starts_are_the_first_frames_of_the_index_rows(R):
    from scrubvae_amd.data.preprocess import get_window_indices
    _, ids, win, _, _ = PC.e2e_inputs()
    W, stride = PC.E2E["window"], PC.E2E["stride"]
    starts = R.window_starts(ids, stride, W)
    rows = get_window_indices(ids, stride, W)
    assert starts.dtype == torch.int64 and starts.shape == (84,)
    assert torch.equal(starts, rows[:, 0]) and torch.equal(rows, win)
    assert torch.equal(starts[:, None] + torch.arange(W), rows)
    # the 30-frame run in the middle yields none: no window holds one of its frames
    assert not bool(((rows >= 200) & (rows < 230)).any())
    # stride 1 and a window as long as a run
    ids2 = np.repeat([4, 9, 9, 2], [5, 3, 4, 6])
    assert torch.equal(R.window_starts(ids2, 1, 6), get_window_indices(ids2, 1, 6)[:, 0])
    assert R.window_starts(ids2, 1, 6).tolist() == [5, 6, 12]


def test_window_starts_every_run_too_short(R):
    ids = np.repeat([1, 2, 3], [10, 50, 7])
    starts = R.window_starts(ids, 3, 51)
    assert starts.dtype == torch.int64 and starts.shape == (0,)
    assert R.window_starts(np.zeros(0, dtype=np.int64), 2, 51).shape == (0,)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n", [84, 85])
def test_shard_order(R, n, world, shuffle):
    shards = [R.shard_order(n, 32, shuffle, 5, 2, r, world) for r in range(world)]
    assert all(s.dtype == torch.int64 and len(s) == n // world for s in shards)
    union = torch.cat(shards)
    assert len(set(union.tolist())) == len(union), "shards overlap"
    assert 0 <= int(union.min()) and int(union.max()) < n
    assert n - len(union) <= world - 1
    again = [R.shard_order(n, 32, shuffle, 5, 2, r, world) for r in range(world)]
    assert all(torch.equal(a, b) for a, b in zip(shards, again))
    other = [R.shard_order(n, 32, shuffle, 5, 3, r, world) for r in range(world)]
    if shuffle:
        assert not torch.equal(torch.cat(other), union)
        assert not torch.equal(R.shard_order(n, 32, True, 6, 2, 0, world), shards[0])
        assert not torch.equal(torch.sort(shards[0]).values, shards[0])
        # every rank cuts the same permutation
        whole = R.shard_order(n, 32, True, 5, 2)
        assert torch.equal(torch.sort(whole).values, torch.arange(n))
        for r in range(world):
            assert torch.equal(shards[r], whole[r::world][: n // world])
    else:
        assert all(torch.equal(a, b) for a, b in zip(shards, other))
        for r in range(world):
            assert torch.equal(shards[r], torch.arange(n)[r::world][: n // world])


def test_shard_order_rejects_bad_ranks(R):
    for args in ((10, 0, False, 0, 0), (10, 4, False, 0, 0, 2, 2), (10, 4, False, 0, 0, -1, 2), (10, 4, False, 0, 0, 0, 0)):
        with pytest.raises(ValueError):
            R.shard_order(*args)


def test_recording_needs_a_gpu(R):
    pose, ids, _, _, _ = PC.e2e_inputs()
    tree, offset = PC.skeleton(PC.E2E["J"], "float")
    with pytest.raises(RuntimeError, match="not a GPU"):
        R.DeviceRecording(pose.numpy(), ids, {"KINEMATIC_TREE": tree, "OFFSET": offset}, PC.E2E["window"], device="cpu")


def test_loader_length_needs_no_gpu(R):
    class Set:
        def __len__(self):
            return 85

    assert [len(R.DeviceWindowLoader(Set(), 32, world=w)) for w in (1, 2, 3)] == [3, 2, 1]
    assert len(R.DeviceWindowLoader(Set(), 85)) == 1 and len(R.DeviceWindowLoader(Set(), 84)) == 2
    with pytest.raises(ValueError):
        R.DeviceWindowLoader(Set(), 0)


def test_entry_points_declared_and_bound():
    from scrubvae_amd import get
    with open(ABI.HEADER) as f:
        assert "Training batches from a resident recording" in f.read()
    assert ABI.declared("svae_window_") == {"svae_window_batch", "svae_window_speed_parts"}
    assert callable(get.device_data)
