"""What test_gpu_pose.py rests on, checked without a GPU: the generators of tests/pose_checks.py meet their stated conditioning at
every case's shape, the fp32 yardstick is itself accurate there (so the bound derived from it is tight), the helpers equal the oracle,
and the comparison has teeth -- the fp32 oracle with one planted mistake in place of the kernel is rejected at the final FACTOR,
the fp64 oracle passes."""
import math

import pytest
import torch

from oracle import scvae_oracle as O
from tests import pose_checks as PC

F32, F64 = torch.float32, torch.float64
TAIL_SHAPES = sorted({(name, ld, rows) for name, ld in PC.TRAIN_LD for rows in PC.TRAIN_ROWS}
                     | {(name, ld, rows) for name, ld in PC.NO_ARENA_LD for rows in (65,)}
                     | {("chain8", 64, PC.TREE_ROWS), ("single", 16, PC.TREE_ROWS), ("len1", 32, PC.TREE_ROWS), ("caps", 208, PC.TREE_ROWS)})
YARDSTICK_LIMIT = 1e-5  # per-row E32 of every output stays below it on the conditioned inputs (plain randn inputs reach 1e-4)


def _truths(d, tree, **kw):
    return PC.tail_truth(d, tree, F64, **kw), PC.tail_truth(d, tree, F32, **kw)


@pytest.mark.parametrize("name,ld,rows", TAIL_SHAPES)
@pytest.mark.parametrize("pre_tanh", [True, False])
def test_tail_generator_and_yardstick(name, ld, rows, pre_tanh):
    J, tree = PC.TREES[name]
    d = PC.tail_inputs(rows, J, ld, pre_tanh)
    arena = d["has_root"]
    assert all(bool(torch.isfinite(v).all()) for v in d.values() if isinstance(v, torch.Tensor))
    assert all(torch.equal(v, PC.r32(v)) for v in d.values() if isinstance(v, torch.Tensor))  # fp32 values
    assert bool((d["y"][:, 6 * J + (3 if arena else 0):] == PC.SENTINEL).all())
    n1, cr, amax = PC.tail_conditioning(d, pre_tanh)
    slack = 1 - 1e-6  # the one rounding of atanh(a) to fp32 moves tanh(y) by < 1e-7 relative
    assert n1 >= PC.R_LO * slack and cr >= PC.R_LO * math.sin(PC.TH_LO) * slack and amax <= PC.R_HI / slack, (n1, cr, amax)
    t64, t32 = _truths(d, tree, arena=arena, pre_tanh=pre_tanh, ext=(True, arena))
    rec = PC.tail_records(dict(x6d=t32["x6d"], root_hat=t32["root_hat"], pose=t32["pose"], dy=t32["dy"]), t64, t32, J, arena)
    rec += [PC.per_row("jpe", t32["jpe"][:, None], t64["jpe"][:, None], t32["jpe"][:, None])]
    for r in rec:
        assert r[4] and r[2] < YARDSTICK_LIMIT, r  # the yardstick against itself passes, and is accurate
    if J > 1:
        assert float(t64["pose"].abs().amax(1).min()) > 0
    assert float(t64["dy"].abs().amax(1).min()) > 0  # no row of the gradient vanishes: every row is compared relatively


def test_tail_shapes_fit_the_lds_rule():
    for name, ld, _ in TAIL_SHAPES:
        assert PC.tail_lds_bytes(PC.TREES[name][0], ld) <= 160 * 1024, (name, ld)
    assert PC.tail_lds_bytes(32, 208) == 105504
    J, tree = PC.TREES["caps"]
    assert J == 32 and len(tree) == 8 and max(len(c) for c in tree) == 8
    for J, tree in PC.TREES.values():  # every tree is one the wrapper accepts: heads placed before use, joints placed once, all covered
        seen = {0}
        for chain in tree:
            assert chain[0] in seen and not (set(chain[1:]) & seen) and len(set(chain[1:])) == len(chain) - 1
            seen |= set(chain[1:])
        assert seen == set(range(J))


@pytest.mark.parametrize("n", PC.ROT_SIZES + [20000])
def test_rot_generator_and_yardstick(n):
    d = PC.rot_inputs(n)
    t64, t32 = PC.rot_truth(d, F64), PC.rot_truth(d, F32)
    assert float((t64["loss"] - d["phi"]).abs().max()) <= 2e-7  # the per-row loss is phi, up to the rounding of the inputs to fp32
    assert math.sin(PC.PHI_LO / 2) - 1e-6 <= float(t64["s"].min()) and float(t64["s"].max()) <= math.sin(PC.PHI_HI / 2) + 1e-6
    for x in (d["x"], d["xh"]):
        n1 = x[:, :3].norm(dim=1)
        cr = torch.cross(x[:, :3] / n1[:, None], x[:, 3:], dim=1).norm(dim=1)
        assert float(n1.min()) >= PC.R_LO * (1 - 1e-6) and float(cr.min()) >= PC.R_LO * 0.5 * (1 - 1e-6)
    for r in (PC.per_row("loss", t32["loss"][:, None], t64["loss"][:, None], t32["loss"][:, None]),
              PC.per_row("dxh", t32["dxh"], t64["dxh"], t32["dxh"])):
        assert r[4] and r[2] < YARDSTICK_LIMIT, r
    assert abs(float(t64["loss"].sum() - O.stable_rotation_loss(d["x"], d["xh"]))) <= 1e-12 * n


def test_rot_identical_rows_are_exactly_zero_in_the_oracle():
    d = PC.rot_inputs(300)
    d["xh"] = d["x"].clone()
    for dtype in (F64, F32):
        t = PC.rot_truth(d, dtype)
        assert float(t["loss"].abs().max()) == 0.0 and float(t["dxh"].abs().max()) == 0.0


def test_planted_fwd_kin_without_a_plant_is_the_oracle():
    for name in ("mouse18", "len1", "caps"):
        J, tree = PC.TREES[name]
        d = PC.tail_inputs(5, J, PC.pad16(6 * J + 3), False)
        c6 = d["y"][:, :6 * J].reshape(5, J, 6)
        assert torch.equal(PC._fwd_kin_planted(c6, tree, d["offsets"], 1e-8), O.fwd_kin(c6, tree, d["offsets"], torch.zeros(5, 3, dtype=F64), eps=1e-8))


def _stand_in(t):
    return dict(x6d=t["x6d"], root_hat=t["root_hat"], pose=t["pose"], dy=t["dy"],
                lp=torch.stack([torch.stack([t[k][b:b + PC.TAIL_BLOCK].sum() for b in range(0, t[k].shape[0], PC.TAIL_BLOCK)])
                                for k in ("jpe", "rl")], dim=1))


# joint 4 ends chain 0, chain 2 = [1, 6, 7, 8] hangs off joint 1: started from joint 0's position it is misplaced
PLANTS = [("leaf", 4, "dy"), ("leaf", 17, "dy"), ("root_chain", 5, "dy"), ("root_chain", 1, "dy"), ("head", (2, 0), "pose"),
          ("ext0", None, "dy"), ("root_tanh", None, "dy")]


@pytest.mark.parametrize("kind,arg,where", PLANTS)
def test_comparison_rejects_a_planted_mistake(kind, arg, where):
    J, tree = PC.TREES["mouse18"]
    d = PC.tail_inputs(150, J, 112)
    kw = dict(arena=True, pre_tanh=True, ext=(True, True))
    t64, t32 = _truths(d, tree, **kw)
    PC.gate("fp32 oracle", PC.tail_records(_stand_in(t32), t64, t32, J, True))
    PC.gate("fp64 oracle", PC.tail_records(_stand_in(t64), t64, t32, J, True))
    wrong = PC.tail_truth(d, tree, F32, plant=(kind, arg), **kw)
    rec = PC.tail_records(_stand_in(wrong), t64, t32, J, True)
    failed = [r[0] for r in rec if not r[4]]
    assert any(f.startswith(where) for f in failed), (kind, arg, rec)
    with pytest.raises(AssertionError):
        PC.gate(kind, rec)


def test_a_late_leaf_mistake_is_seen_per_joint_but_not_by_a_whole_tensor_norm():
    """why the views are per joint: a 0.1 % error in the gradient of one leaf joint stays under the 5e-4-of-the-tensor-maximum bound of
    test_pose_tail, and fails here"""
    J, tree = PC.TREES["mouse18"]
    d = PC.tail_inputs(150, J, 112)
    t64, t32 = _truths(d, tree)
    wrong = dict(t32)
    wrong["dy"] = t32["dy"].clone()
    j = int(t64["dy"][:, :6 * J].reshape(150, J, 6).abs().amax((0, 2)).argmin())  # the joint with the smallest gradients
    wrong["dy"][:, 6 * j:6 * j + 6] *= 1.0 + 1e-3
    rec = PC.tail_records(dict(dy=wrong["dy"]), t64, t32, J, True)
    assert "dy /joint" in [r[0] for r in rec if not r[4]], rec
    whole = float((wrong["dy"].double() - t64["dy"]).abs().max() / t64["dy"].abs().max())
    assert whole < 5e-4


def test_rot_comparison_rejects_a_missing_asin_factor():
    d = PC.rot_inputs(1000)
    t64, t32 = PC.rot_truth(d, F64), PC.rot_truth(d, F32)
    part = lambda t: torch.stack([t["loss"][b:b + PC.ROT_BLOCK].sum() for b in range(0, 1000, PC.ROT_BLOCK)])
    PC.gate("fp32 oracle", PC.rot_records(dict(part=part(t32), dxh=t32["dxh"]), t64, t32))
    PC.gate("fp64 oracle", PC.rot_records(dict(part=part(t64), dxh=t64["dxh"]), t64, t32))
    wrong = PC.rot_truth(d, F32, plant="no_asin")
    rec = PC.rot_records(dict(part=part(t32), dxh=wrong["dxh"]), t64, t32)
    assert [r[0] for r in rec if not r[4]] == ["dxh /row"], rec
