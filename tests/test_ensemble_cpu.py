"""What test_gpu_ensemble.py rests on, checked without a GPU: every generator of tests/ensemble_checks.py meets its stated conditions at
every case, truth and yardstick are finite there, the truths equal the references they restate (the inline fp64 reference of
test_fused_ensemble_fwd_bwd, the oracle's heads), and the comparison has teeth -- the fp32 yardstick with one planted mistake in place
of the kernel is rejected at a named case, the clean yardstick passes."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import scvae_oracle as O
from tests import ensemble_checks as EC

F32, F64 = torch.float32, torch.float64
ENS_CASES = (EC.RUNNER_H1 + EC.RUNNER_H2 + EC.GEOMETRY + [EC.TOO_WIDE + (33, 2)]) + list(EC.DIRECT.values())
LOSS_CASES = [c + (4,) for c in EC.LOSS_CASES] + [c + (1,) for c in EC.LOSS_CASES if c[2] in (2, 258)]


def _passes(rec):
    return all(r[4] for r in rec)


def _all_fp32(tensors):
    return all(torch.equal(t, EC.r32(t)) for t in tensors)


# ------------------------------------------------------------------------------------------------ conditions
@pytest.mark.parametrize("case", ENS_CASES, ids=str)
def test_ensemble_case_is_conditioned(case):
    c = EC.ens_case(*case)
    d, t64, t32 = c["d"], c["t64"], c["t32"]
    assert _all_fp32([d["x"], d["var"]] + d["d_outs"] + [t for mem in d["W"] for wb in mem for t in wb])
    assert EC.ens_why(d, t64) is None
    assert t64["min_pre"] >= EC.PRE_MARGIN
    for (name, a), (_, b) in zip(EC.ens_views(t64), EC.ens_views(t32)):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
        assert EC.row_ratio(a) >= EC.MIN_ROW, (name, EC.row_ratio(a))
    assert _passes(EC.ens_records(t32, t64, t32))  # the yardstick against itself
    assert d["rows"] == d["B"] * d["halves"] and t64["gx"].shape == (d["rows"], d["ind"]) and t64["dsrc"].shape == (d["B"], d["n0"])


def test_one_sample_has_dead_rows_and_they_are_exact_zeros():
    """B = 1: a hidden unit that is off has an identically zero dW row in the next layer, in both precisions"""
    c = EC.ens_case(32, 3, 1, 1)
    dead = 0
    for a, b in zip(c["t64"]["dW"], c["t32"]["dW"]):
        for w64, w32 in zip(a[1:], b[1:]):
            z = w64.abs().amax(1) == 0
            dead += int(z.sum())
            assert torch.equal(z, w32.abs().amax(1) == 0)
    assert dead > 10


def test_lds_rule():
    assert EC.ens_lds_bytes(*EC.CEILING) == 592 * 65 * 4 <= 160 * 1024
    assert EC.ens_lds_bytes(*EC.TOO_WIDE) == 672 * 65 * 4 > 160 * 1024
    for case in ENS_CASES:
        if case[:2] != EC.TOO_WIDE:
            assert EC.ens_lds_bytes(case[0], case[1], case[4] if len(case) > 4 else None) <= 160 * 1024, case
    assert EC._D == tuple(tuple(m) for m in EC.member_dims(32, 16))


@pytest.mark.parametrize("case", LOSS_CASES, ids=str)
def test_loss_case_is_conditioned(case):
    kind, C, rows, scale, n = case
    c = EC.loss_case(*case)
    d, t64, t32 = c["d"], c["t64"], c["t32"]
    assert EC.loss_why(d, t64) is None
    assert _all_fp32(d["outs"]) and (d["target"] is None or _all_fp32([d["target"]]))
    for t in (t64, t32):
        assert all(bool(torch.isfinite(v).all()) for k in ("rows", "dpred", "raw") for v in t[k])
    if kind == 0:
        assert all(0.25 * scale * (1 - 1e-6) <= float((o - d["target"]).abs().min()) for o in d["outs"])
    if kind == 1:
        assert int(d["labels"].min()) == 0 and int(d["labels"].max()) == C - 1
    if scale > 1.0:  # saturated: about half the rows are misclassified, and an exp without the max subtraction overflows
        assert all(float(o.max()) > 50.0 for o in d["outs"]) or rows == 2
        wrong = sum(int((r > 1.0).sum()) for r in t64["raw"])
        assert wrong >= 1 and (rows == 2 or wrong >= d["n"] * rows // 4)
    assert _passes(EC.loss_records(torch.cat([EC.block_sums(r, EC.LOSS_BLOCK) for r in t32["rows"]]), t32["dpred"], t64, t32, d))


@pytest.mark.parametrize("B,z", EC.DIAG_SHAPES + [EC.RANGE_SHAPE], ids=str)
def test_diag_case_is_conditioned_and_equals_the_oracle(B, z):
    ranged = (B, z) == EC.RANGE_SHAPE
    c = EC.diag_case(B, z, ranged)
    d = c["d"]
    assert _all_fp32([d[k] for k in ("mu", "raw", "eps", "dz", "dmu", "dsigma")])
    if ranged:
        assert sorted(set(d["raw"].reshape(-1).tolist())) == sorted(EC.r32(torch.tensor(EC.RANGE_DIAG, dtype=F64)).tolist())
    assert EC.diag_why(d, c["t64"].values()) is None
    for key, t64 in c["t64"].items():
        t32 = c["t32"][key]
        assert all(bool(torch.isfinite(t[k]).all()) for t in (t64, t32) for k in ("mu", "sigma", "z", "kl", "dh")), key
        got = dict(t32, kl_part=EC.block_sums(t32["kl"], EC.DIAG_BLOCK))
        assert _passes(EC.diag_records(got, t64, t32)), key
    # the oracle: CholeskyL(diag) + prior_loss, and autograd through them
    ks = EC.diag_kl_scale(B)
    for use, with_eps in c["t64"]:
        t = c["t64"][(use, with_eps)]
        h = torch.cat([d["mu"], d["raw"]], 1).clone().requires_grad_(True)
        mu = h[:, :z]
        L = O.cholesky_L(h[:, z:], z, True)
        s = L.diagonal(dim1=-2, dim2=-1)
        zz = torch.matmul(L, d["eps"][..., None]).squeeze(-1) + mu if with_eps else mu
        kl = O.prior_loss(mu, L) * B
        obj = ks * kl
        for name, val in (("dz", zz), ("dmu", mu), ("dsigma", s)):
            if name in use:
                obj = obj + (val * d[name]).sum()
        obj.backward()
        s, zz = s.detach(), zz.detach()
        tol = lambda ref: 1e-12 * max(1.0, float(ref.abs().max()))
        assert float((t["sigma"] - s).abs().max()) <= tol(s) and float((t["z"] - zz).abs().max()) <= tol(zz)
        assert abs(float(t["kl"].sum() - kl.detach())) <= 1e-12 * max(1.0, abs(float(kl.detach()))) * B * z
        assert float((t["dh"] - h.grad).abs().max()) <= tol(h.grad)


# ------------------------------------------------------------------------------------------------ the truths restate their references
@pytest.mark.parametrize("case", EC.LEGACY, ids=str)
def test_ensemble_truth_equals_the_inline_reference(case):
    """the generation and the fp64 reference of tests/test_gpu_kernels.py::test_fused_ensemble_fwd_bwd, restated"""
    ind, outd, B, halves = case
    g = torch.Generator().manual_seed(sum(case))
    z = ind if halves == 1 else ind - 5
    dims = EC.member_dims(ind, outd)
    W = []
    for dd in dims:
        mem = []
        for a, b in zip(dd, dd[1:]):
            w = torch.randn(a, b, generator=g, dtype=F64) / math.sqrt(a)
            mem.append((w, torch.randn(b, generator=g, dtype=F64) * 0.5))
        W.append(mem)
    mu = torch.randn(B, z, generator=g, dtype=F64)
    var = torch.randn(B, 5, generator=g, dtype=F64)
    perm = torch.randperm(B, generator=g)
    d_outs = [torch.randn(B * halves, outd, generator=g, dtype=F64) for _ in range(4)]
    # the inline reference
    x64 = mu.clone().requires_grad_(True)
    if halves == 1:
        xin = x64
    else:
        v2 = var.clone()
        v2[:, 3] = var[perm, 3]
        xin = torch.cat([torch.cat([x64, x64], 0), torch.cat([var, v2], 0)], 1)
    ws = [[(w.clone().requires_grad_(True), b.clone().requires_grad_(True)) for w, b in mem] for mem in W]
    ref_outs = []
    for mem in ws:
        h = xin
        for i, (w, b) in enumerate(mem):
            h = h @ w + b
            if i < len(mem) - 1:
                h = torch.relu(h)
        ref_outs.append(h)
    torch.autograd.backward(ref_outs, d_outs)
    d = dict(ind=ind, outd=outd, B=B, halves=halves, rows=B * halves, n0=z, dims=dims, W=W, x=mu, var=var, perm=perm, shuf_col=3,
             d_outs=d_outs)
    t = EC.ens_truth(d, F64)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert all(close(a, b.detach()) for a, b in zip(t["outs"], ref_outs))
    assert close(t["dsrc"], x64.grad)
    for mi, mem in enumerate(ws):
        for li, (w, b) in enumerate(mem):
            assert close(t["dW"][mi][li], w.grad) and close(t["db"][mi][li], b.grad)
    if halves == 1:
        assert close(t["gx"], x64.grad)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_loss_truth_is_the_summed_loss(kind):
    """the per-row losses add up to the reduction="sum" forms test_fused_ensemble_losses compares with"""
    C = (3, 5, 2)[kind]
    d = EC.loss_case(kind, C, 600, 1.0)["d"]
    loss, grad = EC.loss_truth(d, 1, F64)
    x = d["outs"][1].clone().requires_grad_(True)
    if kind == 0:
        ref = ((x - d["target"]) ** 2).sum()
    elif kind == 1:
        ref = F.cross_entropy(x, d["labels"], reduction="sum")
    else:
        ref = F.cross_entropy(torch.softmax(x, -1), F.one_hot((torch.arange(600) >= 300).long(), 2).double(), reduction="sum")
    ref.backward()
    ref = ref.detach()
    assert abs(float(loss.sum() - ref)) <= 1e-12 * float(ref) and float((grad - x.grad).abs().max()) <= 1e-13


# ------------------------------------------------------------------------------------------------ planted mistakes
ENS_PLANTS = [  # the mistake, the case at which it has to be caught, a view that has to catch it
    ("unshuffled", (37, 2, 33, 2), "out0"),   # the second half reads the unshuffled column
    ("half0", (37, 2, 33, 2), "dsrc"),        # the input gradient is summed over half 0 only
    ("drop_tile", (32, 3, 130, 1), "dW1.0"),  # dW misses rows 64 .. 127
    ("pad_rows", (32, 3, 65, 1), "db3.1"),    # rows past the batch keep relu(bias) activations with non-zero g
    ("relu_mask", (32, 3, 65, 1), "gx"),      # the ReLU mask is taken from the wrong layer
]


@pytest.mark.parametrize("plant,case,view", ENS_PLANTS, ids=[p[0] for p in ENS_PLANTS])
def test_planted_ensemble_mistake_is_caught(plant, case, view):
    c = EC.ens_case(*case)
    bad = EC.ens_truth(c["d"], F32, plant)
    rec = EC.ens_records(bad, c["t64"], c["t32"])
    failed = [r[0] for r in rec if not r[4]]
    assert view + " /row" in failed, (plant, failed)
    assert _passes(EC.ens_records(c["t32"], c["t64"], c["t32"]))
    assert _passes(EC.ens_records(EC.ens_truth(c["d"], F64), c["t64"], c["t32"]))


LOSS_PLANTS = [
    ("no_lw2", (0, 3, 600, 1.0), "part2 /block"),     # lw is not applied to member 2
    ("threshold", (2, 2, 600, 1.0), "dpred0 /row"),   # the class threshold is row > rows / 2
    ("no_max", (1, 5, 600, 40.0), "part0 /block"),    # CE without the max subtraction
]


@pytest.mark.parametrize("plant,case,view", LOSS_PLANTS, ids=[p[0] for p in LOSS_PLANTS])
def test_planted_loss_mistake_is_caught(plant, case, view):
    c = EC.loss_case(*case)
    d = c["d"]
    parts = lambda t: torch.cat([EC.block_sums(r, EC.LOSS_BLOCK) for r in t["rows"]])
    bad = EC.loss_truths(d, F32, plant=plant)
    failed = [r[0] for r in EC.loss_records(parts(bad), bad["dpred"], c["t64"], c["t32"], d) if not r[4]]
    assert view in failed, (plant, failed)
    if plant == "threshold":
        assert "part0 /block" in failed  # one row of 600 moves its block's sum by far more than the bound
    assert _passes(EC.loss_records(parts(c["t32"]), c["t32"]["dpred"], c["t64"], c["t32"], d))


DIAG_PLANTS = [
    ("no_log", ("dz",), ["kl_part /block", "dh /row"]),          # KL is missing the 2 log s term
    ("no_dsigma", ("dz", "dmu", "dsigma"), ["dh /row"]),          # dsigma is ignored
]


@pytest.mark.parametrize("plant,use,views", DIAG_PLANTS, ids=[p[0] for p in DIAG_PLANTS])
def test_planted_heads_mistake_is_caught(plant, use, views):
    B, z = 64, 32
    c = EC.diag_case(B, z)
    t64, t32 = c["t64"][(use, True)], c["t32"][(use, True)]
    bad = EC.diag_truth(c["d"], F32, EC.diag_kl_scale(B), use, True, plant)
    failed = [r[0] for r in EC.diag_records(dict(bad, kl_part=EC.block_sums(bad["kl"], EC.DIAG_BLOCK)), t64, t32) if not r[4]]
    assert all(v in failed for v in views), (plant, failed)
    assert _passes(EC.diag_records(dict(t32, kl_part=EC.block_sums(t32["kl"], EC.DIAG_BLOCK)), t64, t32))
