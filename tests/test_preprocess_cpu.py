"""tests/preprocess_checks.py against the oracle and the real reference's recorded outputs, and the fairness of the inputs that
test_gpu_preprocess.py feeds the kernels (kappa bucket shares, truncation share, threshold clearance).  No GPU."""
import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as P
from oracle import scvae_oracle as O
from tests import preprocess_checks as PC
from tests.test_preprocess import load

KEYS = ["x6d", "root", "offsets", "target_pose", "avg_speed_3d", "heading"]
FIXTURES = ["preprocess_tiny", "preprocess_tiny_float"]


def fixture_windows(golden_dir, name):
    fx, skel = load(golden_dir, name)
    win = P.get_window_indices(fx["raw_ids"], int(fx["stride"]), int(fx["window"]))
    return fx, skel, fx["raw_pose"][win]


@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_restatement_is_the_oracle(golden_dir, name):
    fx, skel, pose = fixture_windows(golden_dir, name)
    want = P.preprocess_windows(pose, skel["KINEMATIC_TREE"], skel["OFFSET"], KEYS, "midfwd", fwd_kin=O.fwd_kin)
    got = PC.restate(pose, skel["KINEMATIC_TREE"], skel["OFFSET"], KEYS, "midfwd", dt=torch.float32)
    for k in KEYS:
        assert got[k].dtype == torch.float32 and got[k].shape == want[k].shape, k
        assert float((got[k].double() - want[k].double()).abs().max()) <= 1e-5, k


@pytest.mark.parametrize("name", FIXTURES)
def test_fp64_restatement_is_the_reference(golden_dir, name):
    """the reference's own outputs pass, as `kernel`, the gate the kernels have to pass"""
    fx, skel, pose = fixture_windows(golden_dir, name)
    ref = {k: torch.from_numpy(fx["out/" + k]) for k in KEYS}
    PC.gate_all(name, ref, torch.from_numpy(pose), skel["KINEMATIC_TREE"], skel["OFFSET"], "midfwd", PC.SPEED_PARTS)


def test_speed_parts_keeps_the_reference_quirk_out_only_where_it_cancels():
    pose = PC.make_pose(7, 9, 18, seed=1)
    want = P.get_speed_parts(pose.numpy())
    want = np.concatenate([want[:, :2], want[:, 2:].mean(-1, keepdims=True)], -1)
    assert float((PC.speed_parts(pose) - torch.from_numpy(want)).abs().max()) <= 1e-12


@pytest.mark.parametrize("runs,window,stride", [
    ((40, 10, 33), 16, 4),   # an id run shorter than the window
    ((16, 20), 16, 3),       # a run of exactly the window length
    ((30, 25), 8, 1),        # stride 1
    ((30, 25), 8, 64),       # a stride larger than the run: one window per run
])
def test_window_indices_match_the_oracle(runs, window, stride):
    from scrubvae_amd.data import preprocess as PP
    ids = np.concatenate([np.full(n, 7 - i) for i, n in enumerate(runs)])
    got, want = PP.get_window_indices(ids, stride, window), P.get_window_indices(ids, stride, window)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    assert len(want) == sum((n - window) // stride + 1 for n in runs if n >= window)


@pytest.mark.parametrize("case", PC.CASES, ids=PC.case_id)
def test_gpu_case_inputs_are_fair(case):
    """Most entries are well conditioned, the ill-conditioned tail is no larger than random bone directions give, and hardly any
    truncated length sits on a truncation step.  For a random direction cos^2(theta / 2) is uniform on [0, 1], so
    P(1 / cos(theta / 2) > t) = 1 / t^2; a sum of n such terms exceeds k only if one exceeds k / n: share <= n (n / k)^2."""
    N, W, J, direction, kind, parts = case
    tree, offset = PC.skeleton(J, kind)
    pose = PC.make_pose(N, W, J)
    kap, kpos = PC.kappa(pose, tree, offset)
    assert bool(torch.isfinite(kap).all()) and bool(torch.isfinite(kpos).all())
    n = max(len(c) for c in tree)
    for k, n_terms in ((kap, n), (kpos, 2 * n)):
        sh = PC.bucket_shares(k)
        print(PC.case_id(case), ["%.2e" % s for s in sh])
        assert abs(sum(sh) - 1.0) < 1e-12
        assert sh[0] + sh[1] >= 0.5
        if N * W >= 1000:  # a share of a few frames is not a frequency
            assert sh[3] + sh[4] <= n_terms * (n_terms / 100.0) ** 2 and sh[4] <= n_terms * (n_terms / 1000.0) ** 2
    if kind == "int":
        _, raw = PC.segment_len(pose.reshape(N * W, J, 3), tree, offset)
        assert float((~PC.trunc_clear(raw)).double().mean()) <= PC.TRUNC_SHARE
    t64 = PC.restate(pose, tree, offset, PC.ALL_KEYS, direction, parts)
    assert all(bool(torch.isfinite(v).all()) for v in t64.values())


# observed max of e32 / (kappa 2^-24) over the entries: 5.23 at 512 x 64 x 18, 4.80 at 256 x 51 x 23 (median 0.36 / 0.31); C = 2 x the larger
C_KAPPA = 2 * 5.23


@pytest.mark.parametrize("N,W,J", [(512, 64, 18), (256, 51, 23)])
def test_kappa_explains_the_fp32_error(N, W, J):
    """guards the kappa formula, not the kernel: the fp32 restatement's x6d error is at most C_KAPPA kappa 2^-24 entry by entry"""
    tree, offset = PC.skeleton(J, "float")
    pose = PC.make_pose(N, W, J, seed=2)
    t64, t32 = (PC.restate(pose, tree, offset, ("x6d",), "midfwd", dt=dt)["x6d"] for dt in (torch.float64, torch.float32))
    kap, _ = PC.kappa(pose, tree, offset)
    ratio = (t32.double() - t64).abs().amax(-1) / (kap * 2.0 ** -24)
    print(f"e32 / (kappa 2^-24): max {float(ratio.max()):.2f} median {float(ratio.median()):.2f}")
    assert float(ratio.max()) <= C_KAPPA


def test_e2e_threshold_is_clear_of_every_window():
    pose, ids, win, spd, thr = PC.e2e_inputs()
    assert len(win) == sum((n - PC.E2E["window"]) // PC.E2E["stride"] + 1 for n in PC.E2E["runs"] if n >= PC.E2E["window"])
    assert float(((spd - thr).abs() / thr).min()) >= PC.THRESH_CLEAR
    dropped = int((spd > thr).sum())
    assert 0 < dropped < len(win)


def test_degenerate_poses_give_the_expected_pattern():
    """what the planted frames do to the reference's arithmetic, in fp32 and fp64 alike"""
    d = PC.DEGENERATE
    tree, offset = PC.skeleton(d["J"], "float")
    pose = PC.degenerate_pose()
    for dt in (torch.float64, torch.float32):
        t = PC.restate(pose, tree, offset, PC.ALL_KEYS, "midfwd", dt=dt)
        bad = ~torch.isfinite(t["x6d"]).all(-1)  # [N, W, J]
        assert torch.equal(bad, ~torch.isfinite(t["x6d"]).any(-1))  # a bad rotation is bad in all six entries
        want = torch.zeros_like(bad)
        n, f, a, b = d["opposed"]
        want[n, f, [3, 4]] = True
        n, f, a, b = d["coincident"]
        want[n, f, [7, 8]] = True
        n, f = d["root_back"]
        want[n, f, :] = True
        n, f = d["root_mid"]
        want[n, f, :] = True
        want[n, :, 0] = True
        assert torch.equal(bad, want)
        rbad = ~torch.isfinite(t["root"]).all(-1)
        assert torch.equal(rbad, ~torch.isfinite(t["root"]).any(-1)) and int(rbad.sum()) == d["W"] and bool(rbad[n].all())
        assert int((~torch.isfinite(t["heading"])).sum()) == 2 and not bool(torch.isfinite(t["heading"][n]).any())
        assert bool(torch.isfinite(t["offsets"]).all()) and bool(torch.isfinite(t["avg_speed_3d"]).all())
