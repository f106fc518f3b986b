"""tests/bn_checks.py without a GPU: every case meets the conditions its gates rely on, the truth functions are nn.BatchNorm1d /
nn.PReLU / nn.Upsample plus autograd, every planted mistake is rejected at a named case while the clean fp32 yardstick passes, and
the case lists are the ones test_gpu_bn_stage.py runs."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_checks as K
from tests.bn_checks import F32, F64


def _failed(records, name):
    return [r for r in records if r[0] == name and not r[4]]


# ------------------------------------------------------------------------------------------------ conditions
@pytest.mark.parametrize("case", K.all_stage_cases(), ids=lambda c: f"{c[2]}-{c[0]}x{c[1]}" + ("-offset" if c[3] else ""))
def test_every_case_meets_the_conditions(case):
    rows, C, mode, ratios = case
    d, t64, t32 = K.stage_case(*case)
    assert K.stage_why(d, t64) is None
    if mode != "bn_tanh":
        assert K.kink_margin(d) > K.KINK_MARGIN
    for name, t in K.stage_views(t64, C):
        if ratios is not None and name in ("mean", "rm", "shift"):
            continue  # the offset family holds channels at mean 0: compared in units of std (scaled_view) or through y
        den = t.abs().amax(1)
        live = den > 0
        assert float(den[live].min()) >= K.MIN_ROW * float(den.max()), (case, name)
    if d["npad"]:  # the padding of a layer: y = act(beta) in every row, dx = 0
        pad = slice(C - d["npad"], C)
        b = d["beta"][pad]
        act = torch.tanh(b) if mode == "bn_tanh" else torch.where(b > 0, b, K.ALPHA * b)
        assert torch.allclose(t64["y"][:, pad], act.expand(rows, -1), rtol=1e-14, atol=0)
        assert mode == "eval" or float(t64["dx"][:, pad].abs().max()) == 0.0
    if ratios is not None:  # the sample itself sits at the ratios (x is standardised, then rounded and moved off the kink)
        mean, var, _ = K.batch_stats(d["x"])
        want = torch.tensor([ratios[c % len(ratios)] for c in range(C)], dtype=F64)
        assert float((mean / var.sqrt() - want).abs().max()) < 0.02
    # the clean yardstick passes its own gates; the pivot of the case lags the batch mean by at most half a standard deviation
    K.gate(f"cpu {case}", K.stage_records(t32, t64, t32, d, offset=ratios is not None))
    if mode not in ("bare", "eval"):
        live = C - d["npad"]
        assert float(((d["rm0"] - t64["mean"]) * t64["rstd"])[:live].abs().max()) <= 0.5 + 1e-6


# ------------------------------------------------------------------------------------------------ the truths
@pytest.mark.parametrize("mode", ["bn_prelu", "bn_tanh"])
def test_truth_is_batchnorm1d_and_autograd(mode):
    d, t64, _ = K.stage_case(37, 48, mode)
    bn = torch.nn.BatchNorm1d(48, eps=K.EPS, momentum=K.MOMENTUM).double()
    act = torch.nn.PReLU(init=K.ALPHA).double() if mode == "bn_prelu" else torch.nn.Tanh()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]); bn.bias.copy_(d["beta"]); bn.running_mean.copy_(d["rm0"]); bn.running_var.copy_(d["rv0"])
    x = d["x"].clone().requires_grad_(True)
    y = act(bn(x))
    y.backward(d["dy"])
    eq = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-14)
    assert eq(t64["y"], y) and eq(t64["dx"], x.grad) and eq(t64["dgamma"], bn.weight.grad) and eq(t64["dbeta"], bn.bias.grad)
    assert eq(t64["rm"], bn.running_mean) and eq(t64["rv"], bn.running_var)
    if mode == "bn_prelu":
        assert eq(t64["dalpha"], act.weight.grad)
    m = d["x"].mean(0)
    v = ((d["x"] - m) ** 2).mean(0)
    assert eq(t64["mean"], m) and eq(t64["rstd"], 1 / torch.sqrt(v + K.EPS))
    assert eq(t64["scale"], d["gamma"] / torch.sqrt(v + K.EPS)) and eq(t64["shift"], d["beta"] - m * t64["scale"])
    assert eq(t64["colsum"], x.grad.sum(0))
    bn.eval()
    de, te, _ = K.stage_case(37, 48, "eval")
    with torch.no_grad():
        bn.weight.copy_(de["gamma"]); bn.bias.copy_(de["beta"]); bn.running_mean.copy_(de["rm0"]); bn.running_var.copy_(de["rv0"])
    if mode == "bn_prelu":
        assert eq(te["y"], act(bn(de["x"]))) and eq(te["y"], F.prelu(de["x"] * te["scale"] + te["shift"], de["alpha"]))


def test_bare_truth_is_prelu():
    d, t64, t32 = K.stage_case(129, 64, "bare")
    x, a = d["x"].clone().requires_grad_(True), d["alpha"].clone().requires_grad_(True)
    F.prelu(x, a).backward(d["dy"])
    assert torch.equal(t64["dx"], x.grad) and torch.equal(t64["dalpha"], a.grad) and "dgamma" not in t64


def test_upsample_truth_and_plant():
    for B, L, C in K.UP2_CASES:
        d = K.up2_inputs(B, L, C)
        t64, t32 = K.up2_truth(d, F64, accumulate=True), K.up2_truth(d, F32, accumulate=True)
        up = torch.nn.Upsample(scale_factor=2, mode="linear")
        x = d["x"].clone().requires_grad_(True)
        y = up(x.transpose(1, 2)).transpose(1, 2)
        y.backward(d["dy"])
        assert torch.equal(t64["y"], y) and torch.allclose(t64["dx"], x.grad + d["dx0"], rtol=1e-14, atol=0)
        flat = lambda t: t.reshape(B * L, C)
        assert K.per_row("dx", flat(t32["dx"]), flat(t64["dx"]), flat(t32["dx"]))[4]
        bad = K.up2_truth(d, F32, accumulate=True, plant="no_clamp")
        assert not K.per_row("dx", flat(bad["dx"]), flat(t64["dx"]), flat(t32["dx"]))[4], (B, L, C)


# ------------------------------------------------------------------------------------------------ planted mistakes
PLANT_CASES = [  # plant, the case, the view that has to reject it
    ("biased_rv", (37, 48, "bn_prelu"), "rv /channel"),
    ("chunk_means", (129, 64, "bn_prelu"), "mean /channel"),   # the second chunk holds one row
    ("no_xhat_term", (37, 48, "bn_prelu"), "dx /channel"),
    ("slope_ge", (129, 64, "bn_prelu"), "dalpha /terms"),
    ("slope_ge", (129, 64, "bare"), "dalpha /terms"),
]


@pytest.mark.parametrize("plant,case,view", PLANT_CASES)
def test_planted_mistake_is_rejected(plant, case, view):
    d, t64, t32 = K.stage_case(*case)
    assert not [r for r in K.stage_records(t32, t64, t32, d) if not r[4]]
    bad = K.stage_records(K.stage_truth(d, F32, plant=plant), t64, t32, d)
    assert _failed(bad, view), (plant, case, [(r[0], r[4]) for r in bad])


def test_chunk_means_plant_needs_a_ragged_chunk():
    d, t64, t32 = K.stage_case(128, 16, "bn_prelu")  # one full chunk: the planted mean is the mean
    assert not [r for r in K.stage_records(K.stage_truth(d, F32, plant="chunk_means"), t64, t32, d) if r[0].startswith("mean") and not r[4]]


def _ratio_channels(t, k, C):
    return t[[c for c in range(C) if c % 4 == k]]


@pytest.mark.parametrize("C", [16, 64])
def test_onepass_fp32_is_rejected_by_the_offset_family(C):
    """the statistics algorithm before the pivot: rejected by the per-channel rstd view at mean / std = 4 and 37 rows (and
    at 16), although it passes at mean / std = 0 and 1 -- and passes the old tests' global max-norm on their own input."""
    d, t64, t32 = K.stage_case(37, C, "bn_prelu", K.OFFSET_RATIOS)
    bad = K.stage_truth(d, F32, plant="onepass_fp32")
    verdict = {}
    for k, r in enumerate(K.OFFSET_RATIOS):
        sub = lambda t: _ratio_channels(t["rstd"], k, C)
        rec = K.per_channel(f"rstd ratio {r:g}", sub(bad), sub(t64), sub(t32), C // 4)
        print(f"onepass_fp32 37 x {C} ratio {r:g}: err {rec[1] / K.U:.1f} u, yardstick {rec[2] / K.U:.1f} u, bound {rec[3] / K.U:.1f} u")
        verdict[r] = rec[4]
    assert verdict[0.0] and verdict[1.0] and not verdict[4.0] and not verdict[16.0], verdict
    assert _failed(K.stage_records(bad, t64, t32, d, offset=True), "rstd /channel")
    # the restated algorithm is the cold kernel: it stays inside the derived cold gate
    assert K.cold_rstd_view("rstd", bad["rstd"], t64, t32)[4]


@pytest.mark.parametrize("rows,C", [(37, 16), (700, 48)])
def test_onepass_fp32_passes_the_old_global_norm(rows, C):
    """test_bn_prelu_fwd_bwd's input (every channel randn * 2 + 0.7, |mean| / std = 0.35) and measure (one max-norm, 5e-6)"""
    g = torch.Generator().manual_seed(rows)
    x = K.r32(torch.randn(rows, C, generator=g, dtype=F64) * 2 + 0.7)
    gamma, beta = K.r32(1 + 0.1 * torch.randn(C, generator=g, dtype=F64)), K.r32(0.1 * torch.randn(C, generator=g, dtype=F64))
    y = F.prelu(F.batch_norm(x, None, None, gamma, beta, True, 0.1, K.EPS), torch.tensor([K.ALPHA], dtype=F64))
    mean, rstd = K.onepass_fp32(x)
    scale = gamma.float() * rstd
    got = F.prelu(x.float() * scale + (beta.float() - mean * scale), torch.tensor([K.ALPHA]))
    assert K.global_maxnorm(got, y) < 5e-6


@pytest.mark.parametrize("rows,C", K.OFFSET_CASES)
def test_cold_gate_holds_for_the_restated_algorithm(rows, C):
    """the derived cold bound against the CPU restatement of the un-pivoted kernel (the GPU file asserts it for the kernels)"""
    d, t64, t32 = K.stage_case(rows, C, "bn_prelu", K.OFFSET_RATIOS)
    mean, rstd = K.onepass_fp32(d["x"])
    rec = K.cold_rstd_view("rstd cold", rstd, t64, t32)
    print(f"cold restated {rows} x {C}: worst {rec[1] / K.U:.1f} u of a bound of {rec[3] / K.U:.1f} u;",
          {r: round(v, 1) for r, v in K.by_ratio(rstd, t64, K.OFFSET_RATIOS).items()})
    assert rec[4], rec


def test_colsum_truth():
    d = K.colsum_inputs(513, 144)
    assert torch.equal(K.colsum_truth(d, F64, True), d["x"].sum(0) + d["out0"])
    rec = K.cancel_view("colsum", K.colsum_truth(d, F32), K.colsum_truth(d, F64), K.colsum_truth(d, F32), d["x"].abs().sum(0))
    assert rec[4]
    wrong = K.colsum_truth(d, F32) - d["x"][512].float()  # the ragged chunk's row dropped
    assert not K.cancel_view("colsum", wrong, K.colsum_truth(d, F64), K.colsum_truth(d, F32), d["x"].abs().sum(0))[4]


# ------------------------------------------------------------------------------------------------ the GPU file runs these lists
def test_gpu_file_runs_these_case_lists():
    from tests import test_gpu_bn_stage as G
    for name in ("SHAPE_CASES", "TANH_CASES", "BARE_CASES", "EVAL_CASES", "TRIP_CASES", "LD_CASES", "WORLD2_CASES", "ACC_CASES",
                 "OFFSET_CASES", "UP2_CASES", "COLSUM_TASKS", "CONV_STAT_CASES"):
        assert getattr(G.K, name) is getattr(K, name)
    assert G.K is K
    ran = set(G.STAGE_CASES_RUN)
    assert ran == set(K.all_stage_cases()), ran ^ set(K.all_stage_cases())
