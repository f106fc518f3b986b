"""pose_tail_kernel and rot_loss_kernel (csrc/pose_tail.hip) against the fp64 oracle, row by row, joint by joint and block by block
(tests/pose_checks.py has the inputs, the truth, the fp32 yardstick and the rule  error <= max(FACTOR E32, FLOOR)).

Inputs are well conditioned by construction (|a1| >= 0.3, |x x a2| >= 0.15, rotation-loss angles in [0.3, 2.4]) and rounded to fp32
once; the padding columns of y hold a sentinel nothing may depend on.  Every output buffer is allocated a few rows longer than the
launch writes and filled with the sentinel: the rows past `rows` (and the loss partials past tail_blocks(rows)) have to survive, the
padding columns of dy have to be exactly 0.  Every gate prints its figures (run with -s).

Deliberately not here:
  * rotations at angle pi in the rotation loss: the clamp decides between a zero and a ~4000x gradient on the last bit of s, and the
    reference is just as arbitrary there;
  * zero-length or parallel 6D vectors (the normalisations are ill-conditioned or undefined, in the reference too);
  * the SVAE_TAIL_ROWS experiment override: it is read once per process.
root_hat with pre_tanh = False is NOT a copy of the input (it is the arena rescaling of the root columns), so it is gated like every
other computed output; x6d_hat is a copy there and has to be bit-equal."""
import pytest
import torch

from tests import pose_checks as PC
from tests.pose_checks import SENTINEL

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
PAD_ROWS = 3  # every output is over-allocated by this many sentinel rows


@pytest.fixture(scope="module")
def ops():
    from scrubvae_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def dev(t):
    return t.float().contiguous().cuda()


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def only_sentinel(t):
    return bool((t == SENTINEL).all())


def launch(ops, d, tree, arena=True, pre_tanh=True, ext=(False, False), want_dy=True, want_pose=True, scales=(PC.JPE_SCALE, PC.ROOT_SCALE),
           target=None):
    """one svae_pose_tail launch on the case `d`; returns the written parts of the outputs after checking that nothing else was written"""
    from scrubvae_amd._lib import make_tree
    rows, J, ld = d["rows"], d["J"], d["ld"]
    nb = ops.tail_blocks(rows)
    assert nb == (rows + PC.TAIL_BLOCK - 1) // PC.TAIL_BLOCK
    y, offsets = dev(d["y"]), dev(d["offsets"])
    target = dev(d["target"]) if target is None else target
    buf = dict(x6d=sentinel(rows + PAD_ROWS, 6 * J), root_hat=sentinel(rows + PAD_ROWS, 3) if arena else None,
               pose=sentinel(rows + PAD_ROWS, 3 * J) if want_pose else None, dy=sentinel(rows + PAD_ROWS, ld) if want_dy else None)
    lp = sentinel(nb + PAD_ROWS, 2)
    ops.pose_tail(y, ld, offsets, target, dev(d["root"]) if arena else None, [v for a in PC.ARENA for v in a] if arena else None,
                  make_tree(J, tree), scales[0], scales[1], dev(d["E"]) if ext[0] else None, dev(d["Er"]) if ext[1] else None,
                  buf["x6d"], buf["root_hat"], lp, buf["dy"], rows, pre_tanh=pre_tanh, pose_out=buf["pose"])
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().double(), d["y"]) and torch.equal(offsets.cpu().double(), d["offsets"])  # inputs are read only
    out = dict(lp=lp[:nb].cpu())
    assert only_sentinel(lp[nb:])
    for k, b in buf.items():
        if b is not None:
            assert only_sentinel(b[rows:]), k
            out[k] = b[:rows].cpu()
    return out


def check_tail(ops, tag, d, tree, arena=True, pre_tanh=True, ext=(False, False)):
    """training-form launch (dy, pose_out) against the truth; returns the launch's outputs"""
    J = d["J"]
    kw = dict(arena=arena, pre_tanh=pre_tanh, ext=ext)
    t64, t32 = PC.tail_truth(d, tree, F64, **kw), PC.tail_truth(d, tree, F32, **kw)
    got = launch(ops, d, tree, **kw)
    n = 6 * J + (3 if arena else 0)
    assert float(got["dy"][:, n:].abs().max() if d["ld"] > n else 0.0) == 0.0  # padding columns carry exactly no gradient
    if not arena:
        assert float(got["lp"][:, 1].abs().max()) == 0.0
    if not pre_tanh:
        assert torch.equal(got["x6d"].double(), d["y"][:, :6 * J])  # a copy
    PC.gate(f"{tag} | rows={d['rows']} ld={d['ld']} ext={int(ext[0])}{int(ext[1])}", PC.tail_records(got, t64, t32, J, arena))
    return got


# ------------------------------------------------------------------------------------------------ pose tail: training form
@pytest.mark.parametrize("rows", PC.TRAIN_ROWS)
@pytest.mark.parametrize("name,ld", PC.TRAIN_LD)
def test_tail_train(ops, name, ld, rows):
    J, tree = PC.TREES[name]
    d = PC.tail_inputs(rows, J, ld)
    for ext in PC.EXT_FORMS:
        check_tail(ops, f"train {name}", d, tree, ext=ext)


@pytest.mark.parametrize("name,ld", [PC.TRAIN_LD[0], PC.TRAIN_LD[3]])
def test_tail_eval_form_is_bit_equal(ops, name, ld):
    """dy = None: the same outputs and loss partials as the training-form launch"""
    J, tree = PC.TREES[name]
    d = PC.tail_inputs(150, J, ld)
    a = launch(ops, d, tree, ext=(True, True))
    b = launch(ops, d, tree, want_dy=False)
    assert "dy" not in b
    for k in ("x6d", "root_hat", "pose", "lp"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name,ld", PC.NO_ARENA_LD)
@pytest.mark.parametrize("pre_tanh", [True, False])
def test_tail_no_arena(ops, name, ld, pre_tanh):
    """root, root_hat and arena None; ld = 6 J (108) and an ld that is no multiple of 16 (140)"""
    J, tree = PC.TREES[name]
    d = PC.tail_inputs(65, J, ld, pre_tanh)
    assert not d["has_root"]
    for ext0 in (False, True):
        check_tail(ops, f"no-arena {name} pre_tanh={int(pre_tanh)}", d, tree, arena=False, pre_tanh=pre_tanh, ext=(ext0, False))


@pytest.mark.parametrize("name,ld", [PC.TRAIN_LD[0], PC.TRAIN_LD[2]])
def test_tail_input_after_tanh_with_gradient(ops, name, ld):
    """pre_tanh = False with dy: the gradient carries no tanh factor, x6d_hat is a copy"""
    J, tree = PC.TREES[name]
    d = PC.tail_inputs(65, J, ld, pre_tanh=False)
    for ext in ((False, False), (True, True)):
        check_tail(ops, f"post-tanh {name}", d, tree, pre_tanh=False, ext=ext)


# ------------------------------------------------------------------------------------------------ pose tail: forward kinematics form
@pytest.mark.parametrize("name", ["mouse18", "syn23"])
def test_fwd_kin_cont6d(ops, name):
    """data/synthetic.py's use: pre_tanh = 0, pose_out == target, scales 0, no dy, no arena (J = 18: ld = 108 on the caller's tensor;
    J = 23: 138 is no multiple of 4, a padded copy)"""
    from scrubvae_amd.data import synthetic
    J, tree = PC.TREES[name]
    rows = 130
    d = PC.tail_inputs(rows, J, 6 * J, pre_tanh=False)
    t64, t32 = (PC.tail_truth(d, tree, dt, arena=False, pre_tanh=False, want_grad=False) for dt in (F64, F32))
    x6d = dev(d["y"]).reshape(2, rows // 2, J, 6)
    pose = synthetic.fwd_kin_cont6d(x6d, tree, dev(d["offsets"]).reshape(2, rows // 2, J, 3))
    torch.cuda.synchronize()
    assert pose.shape == (2, rows // 2, J, 3)
    PC.gate(f"fk synthetic {name}", [PC.per_row("pose", pose.reshape(rows, 3 * J), t64["pose"], t32["pose"])])


@pytest.mark.parametrize("name,ld", PC.NO_ARENA_LD)
def test_fwd_kin_form_with_a_separate_target(ops, name, ld):
    J, tree = PC.TREES[name]
    d = PC.tail_inputs(65, J, ld, pre_tanh=False)
    kw = dict(arena=False, pre_tanh=False)
    t64, t32 = (PC.tail_truth(d, tree, dt, want_grad=False, **kw) for dt in (F64, F32))
    target = dev(d["target"])
    got = launch(ops, d, tree, want_dy=False, scales=(0.0, 0.0), target=target, **kw)
    assert torch.equal(target.cpu().double(), d["target"].reshape(65, J, 3))
    assert torch.equal(got["x6d"].double(), d["y"][:, :6 * J]) and float(got["lp"][:, 1].abs().max()) == 0.0
    PC.gate(f"fk direct {name}", PC.tail_records(got, t64, t32, J, False))


# ------------------------------------------------------------------------------------------------ pose tail: other trees
@pytest.mark.parametrize("name", ["chain8", "single", "len1", "caps"])
def test_tail_trees(ops, name):
    J, tree = PC.TREES[name]
    ld = PC.pad16(6 * J + 3)
    assert PC.tail_lds_bytes(J, ld) <= 160 * 1024
    d = PC.tail_inputs(PC.TREE_ROWS, J, ld)
    got = check_tail(ops, f"tree {name}", d, tree, ext=(True, True))
    if name == "single":
        assert float(got["pose"].abs().max()) == 0.0
        check_tail(ops, f"tree {name}", d, tree, arena=True, ext=(True, False))
    else:
        check_tail(ops, f"tree {name}", d, tree, ext=(False, False))


# ------------------------------------------------------------------------------------------------ pose tail: what the wrapper refuses
REJECTED = [  # name, J, tree, ld, arena, root buffers, the wrapper's message
    ("uncovered", 4, [[0, 1, 2]], 32, True, True, "joint 3 not covered by the kinematic tree"),
    ("twice", 4, [[0, 1, 2], [0, 2, 3]], 32, True, True, "joint 2 placed twice"),
    ("unplaced head", 4, [[0, 1], [3, 2]], 32, True, True, "chain 1 starts at a joint not yet placed"),
    ("ld too small", 4, [[0, 1, 2, 3]], 24, True, True, "ld 24 too small or misaligned"),
    ("ld % 4", 4, [[0, 1, 2, 3]], 30, True, True, "ld 30 too small or misaligned"),
    ("arena without root", 4, [[0, 1, 2, 3]], 32, True, False, "arena without root buffers"),
]


@pytest.mark.parametrize("name,J,tree,ld,arena,roots,msg", REJECTED, ids=[r[0] for r in REJECTED])
def test_tail_rejections(ops, name, J, tree, ld, arena, roots, msg):
    """host-side validation only: no kernel is launched, no output is written"""
    from scrubvae_amd._lib import make_tree
    rows = 5
    out = [sentinel(rows, 6 * J), sentinel(rows, 3), sentinel(1, 2), sentinel(rows, 32)]
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(RuntimeError, match=msg):
        ops.pose_tail(z(rows, 32), ld, z(rows, J, 3), z(rows, J, 3), z(rows, 3) if roots else None, [v for a in PC.ARENA for v in a],
                      make_tree(J, tree), 1.0, 1.0, None, None, out[0], out[1] if roots else None, out[2], out[3], rows)
    torch.cuda.synchronize()
    assert all(only_sentinel(o) for o in out)


# ------------------------------------------------------------------------------------------------ rotation loss
def rot_launch(ops, x, xh, n, want_grad=True):
    nb = ops.rot_blocks(n)
    assert nb == (n + PC.ROT_BLOCK - 1) // PC.ROT_BLOCK
    part, dxh = sentinel(nb + PAD_ROWS), sentinel(n + PAD_ROWS, 6) if want_grad else None
    ops.rot_loss(x, xh, PC.ROT_SCALE, part, dxh, n)
    torch.cuda.synchronize()
    assert only_sentinel(part[nb:]) and (dxh is None or only_sentinel(dxh[n:]))
    return dict(part=part[:nb].cpu(), dxh=None if dxh is None else dxh[:n].cpu())


@pytest.mark.parametrize("n", PC.ROT_SIZES)
def test_rot_loss_rows(ops, n):
    d = PC.rot_inputs(n)
    t64, t32 = PC.rot_truth(d, F64), PC.rot_truth(d, F32)
    x, xh = dev(d["x"]), dev(d["xh"])
    got = rot_launch(ops, x, xh, n)
    PC.gate(f"rot n={n}", PC.rot_records(got, t64, t32))
    assert torch.equal(rot_launch(ops, x, xh, n, want_grad=False)["part"], got["part"])  # dx6d_hat = None: the same partials
    assert torch.equal(x.cpu().double(), d["x"]) and torch.equal(xh.cpu().double(), d["xh"])


def test_rot_loss_identical_rows(ops):
    """x_hat == x: loss and gradient are exactly 0 (as in the fp32 and fp64 oracle, test_pose_cpu.py)"""
    n = 300
    x = dev(PC.rot_inputs(n)["x"])
    got = rot_launch(ops, x, x.clone(), n)
    assert float(got["part"].abs().max()) == 0.0 and float(got["dxh"].abs().max()) == 0.0
