"""Inputs, fp64 truth, fp32 yardstick, planted mistakes and the per-channel comparison for the BatchNorm + PReLU / tanh stage behind
every conv of the training step (csrc/elementwise.hip: bn_stats_partial, bn_reduce_partials, bn_finalize, bn_stats_finalize,
bn_bwd_reduce, bn_eval_coeffs, affine_prelu_fwd / _bwd_partial / _bwd_apply, upsample2_fwd / _bwd, the batched column sums; and the
fused statistics of the conv epilogues), used by test_bn_stage_cpu.py (no GPU) and test_gpu_bn_stage.py.

The pattern is that of tests/pose_checks.py and tests/ensemble_checks.py: every truth function is dtype-generic -- on float64
tensors it is the truth (F.batch_norm in train / eval mode, F.prelu / torch.tanh, F.interpolate, autograd), on the same values as
float32 tensors it is the yardstick, the error torch's own fp32 arithmetic makes at these inputs.  Inputs are drawn in fp64 and
rounded to fp32 once.

Views.  y and dx are looked at ROW BY ROW (pose_checks.per_row) and CHANNEL BY CHANNEL (per_channel: one view row per channel over
all rows of the case, the error relative to that channel's largest true entry); mean, rstd, scale, shift, the running statistics,
dgamma and the eval coefficients channel by channel.  A view passes when its worst row / channel is at most

    max(FACTOR * E32, FLOOR),      E32 = the worst yardstick error of the same view in the same case.

Sums that cancel (dbeta, the column sums of dx, the slope gradient dalpha) are measured, kernel and yardstick alike, relative to the
sum of the ABSOLUTE terms (cancel_view), as conv_checks.bn_bwd_fused_check does.

Conditions (asserted for every case by test_bn_stage_cpu.py, met by a seed search like ensemble_checks._search):
  * every live channel of every tensor compared per channel has a largest true entry of at least 1/256 of the tensor's max-norm;
  * PReLU cases: no pre-activation u = gamma * xhat + beta lies within 1e-3 rms(u) of the kink.  The statistics come from x itself,
    so the offending entries of x are MOVED away from the kink and the statistics recomputed until it holds; nothing is excluded;
  * every output buffer of the GPU tests is followed by guard rows and, where ld > C, guard columns (conv_checks.guarded).

The statistics and the pivot.  The batch variance is Q/N - (S/N)^2 with S, Q summed in fp32 per 128-row chunk (or per conv row
tile), so the rounding of Q sits at the size of var + mean^2: with a channel mean of 4 (16) standard deviations the one-pass sums
are off by 29 - 35 (215 - 672) u of rstd at 37 rows (measured, below) while torch's fp32 BatchNorm stays below 2 u (plant
"onepass_fp32" restates that algorithm; the offset family is the case that rejects it).  The producers can sum x - p about a
per-channel pivot p (the layer's running mean where ResVAE.bn_pivot is on; NULL, zeros, is the model's default), and the rounding sits
at var + (mean - p)^2.  The offset family (channel c at mean / std = (0, 1, 4, 16)[c % 4]) runs twice: with a pivot that lags the
batch mean by U[-0.5, 0.5] std -- FACTOR applies -- and cold, with no pivot.  Cold, the error is the algorithm's and no yardstick
multiple applies; its gate is derived: each fp32 partial is a sum of at most 8 rounded squares and 16 lane sums (plus the row-wave
sums of a conv epilogue), hence |dvar| <= 75 u (var + d^2), d = mean - p, and

    |drstd| / rstd  <=  37.5 u (var + d^2) / (var + eps) + 2 u          (cold_rstd_view).

FACTOR: the project's 8 (latent_checks.FACTOR) was the starting point.  Worst  kernel error / max(E32, 2^-24)  per family and view,
measured on an MI355X at the commit that added this file (test_gpu_bn_stage.py prints every figure with -s):

  family (GATE tag)      y/row y/ch  dx/row dx/ch  mean  rstd  scale shift  rm    rv   dgamma dbeta colsum dalpha
  shape bn_prelu single   2.05  2.06  2.26  2.40  2.72  1.78  1.93  1.35  1.06  1.18  3.42  2.63    -    0.65
  shape bn_prelu split    2.05  2.06  2.26  2.40  2.72  1.99  1.93  1.35  1.06  1.18  3.42  2.63  1.57   0.65
  shape bn_tanh single    2.42  2.40  1.71  1.19  2.35  1.53  1.17  1.10  1.00  1.15  1.23  2.08    -      -
  shape bn_tanh split     2.42  2.40  2.20  1.48  2.35  1.49  1.11  1.10  1.00  1.15  1.23  2.08  2.12     -
  shape bare              exact exact exact exact   -     -     -     -     -     -     -     -   0.88   0.11
  shape eval              1.16  1.35    -     -     -     -   1.00  1.67    -     -     -     -     -      -
  trips                   0.96  0.83  0.92  0.71  1.11  0.89  1.00  1.31  1.00  1.00  0.63  0.38  0.28   0.25
  ld = C + 16 single      1.28  1.36  1.46  1.76  2.26  1.10  0.79  1.44  1.00  1.18  1.41  1.05  1.17   0.02
  ld = C + 16 split       1.28  1.04  1.83  1.76  2.21  1.99  1.57  1.44  1.00  1.18  1.41  1.05  1.17   0.02
  accumulate single       1.21  1.94  1.46  2.40  2.26  1.35  1.93  0.56  1.00  1.18  4.11  1.41  1.18   0.20
  accumulate split        1.21  1.94  1.83  2.40  1.63  1.99  1.93  0.41  1.00  1.18  4.11  1.41  1.18   0.20
  world 2                 1.08  1.26  1.14  1.40  1.65  0.89  0.85  2.17  1.00  0.88  1.27  1.05    -    0.11
  offset, pivot (both)    1.71  2.16  1.06  1.10  1.01* 1.16  1.01    -   1.00* 1.00  1.24  1.12    -    0.19
  conv tile_epilogue      1.12  1.10    -     -   0.91  0.95  0.87    -   1.00  1.00    -     -     -      -
  conv tile_epilogue16    0.87  1.18    -     -   0.98  1.10  1.10    -   1.00  1.26    -     -     -      -
  conv ..., accumulate      -     -     -     -   0.91  1.05  0.91    -   1.00  1.00    -     -     -      -
  conv ...16, accumulate    -     -     -     -   0.98  0.90  0.95    -   1.00  1.26    -     -     -      -
  upsample2 (all cases)   1.81  1.26  1.34  1.24    -     -     -     -     -     -     -     -     -      -
  column sums (one flush)   -     -     -     -     -     -     -     -     -     -     -     -   1.42     -
(* in units of the channel's standard deviation, scaled_view; "exact": every entry equal to the truth's.)

Everything but dgamma stays at or below 2.72, twice that 5.4: FACTOR stays at the project's 8.  dgamma reaches 4.11 (37 x 48 with
accumulate, where E32 is 3 u), above 4, so its view uses FACTOR_SUMS = 16 as the parameter-gradient views of ensemble_checks do, for
the same reason: it is a sum over the batch of du * xhat that the kernel adds row after row in fp32 within a chunk (eight rows a
lane, sixteen lanes), with xhat formed from the fp32-rounded mean and rstd, where torch's fp32 BatchNorm backward sums in its own
vectorised order; a channel's sum is a few times smaller than its running partial sums.

Cold (no pivot), |drstd| / rstd in u by mean / std (0, 1, 4, 16), same machine and commit -- what the first steps of a run cost
before running_mean has followed the batch mean (momentum 0.1: the lag falls below one std of a channel at 16 std after ~27 steps):
  37 x 16:   0.5  2.5  34.6 214.7      700 x 16:  0.5  1.6  15.7  62.9      4133 x 16:  0.8  0.5  6.4   71.5
  37 x 64:   1.7  3.3  28.9 672.5      700 x 64:  1.0  1.8  16.8 332.5      4133 x 64:  0.8  0.8  5.8  141.7
  conv tile_epilogue (160 rows, ratios 4 / 16): 25.8 / 339.2     conv tile_epilogue16 (160 rows): 31.0 / 650.7
The worst is 0.07 of its derived bound (37 x 64 at 16: 672.5 u of 9639 u).  Held to what the pivoted run of the same case is held
to, FACTOR * E32 = 10.6 .. 13.3 u, the same launches with pivot = None miss the per-channel rstd view
  at mean / std = 16 at every size:  214.7, 672.5 / 62.9, 332.5 / 71.5, 141.7 u  (37 / 700 / 4133 rows; C = 16, 64),
  at mean / std = 4 at 37 and 700 rows:  34.6, 28.9 / 15.7, 16.8 u;  at 4133 rows they pass (6.4, 5.8 u),
and pass at 0 and 1 (test_offset_family_cold prints each figure against its FACTOR * E32); with the pivot the same channels sit
at 0.4 .. 1.9 u.

With the pivot no view comes near 64, the ratio at which a kernel has a precision defect to be fixed rather than a bound to be
widened; without it the statistics are that defect."""
import functools
import math

import torch
import torch.nn.functional as F

from tests.ensemble_checks import MIN_ROW, _search, conditioned
from tests.latent_checks import FLOOR, _gen, f32, r32  # noqa: F401  (re-exported to the two test files)
from tests.pose_checks import FACTOR, _cpu64, _view, gate, per_row, ratio  # noqa: F401

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
EPS = f32(1e-4)
MOMENTUM = f32(0.1)
FACTOR_SUMS = 16.0  # the dgamma view, see above
ALPHA = 0.25  # exact in fp32
STAT_ROWS = 128  # rows per chunk of bn_stats_partial / affine_prelu_bwd_partial
CS_ROWS = 512    # rows per chunk of the batched column sums
KINK_MARGIN = 1e-3  # of rms(u): the condition; the generator moves entries to three times that
STALE = 7.0  # what the gradient tensors hold before a launch (overwritten, or added to under accumulate); exact in fp32
OFFSET_RATIOS = (0.0, 1.0, 4.0, 16.0)
MODES = ("bn_prelu", "bn_tanh", "bare", "eval")

# ---- the case lists (test_gpu_bn_stage.py imports them; test_bn_stage_cpu.py holds every one of them to the conditions) ----
# shape: every C of {16, 48, 64, 144, 512, 1024, 2048} and every row count of {2, 37, 127, 128, 129, 700} at least once.
#   C / 4 a power of two, the one-quad-per-thread path: 16, 64, 512, 1024 (1024: C / 4 = 256, its last size); generic path: 48, 144,
#   2048 (C / 4 = 512); 144 = three 64-column blocks, the last ragged; fin_cpb = 1, 2, 4, 8 at 16 / 144 / 512 / 1024.
#   rows: 2 = the smallest batch BatchNorm takes, 37 < one chunk, 127 / 128 / 129 around a chunk, 700 = five chunks and a ragged one.
#   48 and 144 carry 8 and 3 all-zero pad channels (a 40- and a 141-channel layer; not in the bare mode, which has no beta): exact
#   y = act(beta), dx = 0.
SHAPE_CASES = [(2, 16), (37, 48), (127, 64), (128, 144), (129, 512), (700, 1024), (37, 2048), (700, 144), (129, 64), (128, 16)]
PADS = {48: 8, 144: 3}
TANH_CASES = [(37, 48), (700, 144), (129, 64)]
BARE_CASES = [(37, 48), (129, 64), (700, 16)]
EVAL_CASES = [(37, 48), (129, 512), (2, 16)]
# trips: (4133, 512) and (32773, 16): 33 / 257 chunks, a finalize lane (256 / cpb of them per channel) walks two at cpb = 8 / 1;
# (262200, 16): 4097 workgroups of work, the second trip of the capped 4096-block grid of affine_prelu_fwd / _bwd_apply;
# (16400, 64) with column sums: 1025 workgroups of work on the 1024-block grid
TRIP_CASES = [(4133, 512, False), (32773, 16, False), (262200, 16, False), (16400, 64, True)]  # rows, C, column sums of dx
LD_CASES = [(129, 48), (129, 64)]  # run at ld = C + 16
WORLD2_CASES = [(700, 64, 283), (129, 48, 100)]  # rows, C, rows of rank 0
ACC_CASES = [(129, 64), (37, 48)]  # both accumulate values, both paths
OFFSET_CASES = [(rows, C) for rows in (37, 700, 4133) for C in (16, 64)]
UP2_CASES = [(3, 1, 16), (2, 2, 48), (2, 7, 16), (5, 4, 64)]  # B, L, C; each at ld = C and C + 16
# column sums: tasks of different C in one flush; 16900 rows = 34 chunks of 512, a final-kernel lane (32 per column) takes two.
# "add": ColsumBatch.add, a matrix; "partials": ColsumBatch.add_partials, the rows another kernel left behind (ld = C)
COLSUM_TASKS = [(1, 16, 16, "add"), (511, 48, 48, "partials"), (512, 64, 80, "add"), (513, 144, 144, "add"), (16900, 16, 32, "add"),
                (700, 1024, 1024, "add"), (1024, 64, 64, "partials")]  # rows, C, ld, kind
# conv cases of test_gpu_kernels.CONV_CASES (index, tile code, pieces, the epilogue it has to run): a split kernel with stats_tiles() > 0
CONV_STAT_CASES = [(1, 128064, 3, "tile_epilogue"), (2, 18128128, 22, "tile_epilogue16")]
CONV_RATIOS = (4.0, 16.0)


# ------------------------------------------------------------------------------------------------ inputs
def _uniform(g, lo, hi, *shape):
    return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=F64)


def _signed(g, lo, hi, *shape):
    return _uniform(g, lo, hi, *shape) * (2.0 * (torch.rand(*shape, generator=g, dtype=F64) < 0.5) - 1.0)


def batch_stats(x):
    """fp64 (mean, biased var, rstd) per channel"""
    var, mean = torch.var_mean(x.double(), 0, unbiased=False)
    return mean, var, (var + EPS).rsqrt()


def pre_activation(d):
    """u of the case in fp64 (bare: x itself; eval: from the running statistics)"""
    x = d["x"]
    if d["mode"] == "bare":
        return x
    if d["mode"] == "eval":
        return (x - d["rm0"]) * (d["rv0"] + EPS).rsqrt() * d["gamma"] + d["beta"]
    mean, _, rstd = batch_stats(x)
    return (x - mean) * rstd * d["gamma"] + d["beta"]


def kink_margin(d):
    """min |u| / rms(u) over the live channels (inf for tanh)"""
    if d["mode"] == "bn_tanh":
        return math.inf
    u = pre_activation(d)[:, : d["C"] - d["npad"]]
    return float(u.abs().min() / u.pow(2).mean().sqrt())


def _unkink(d):
    """move the entries of x whose u lies within 3 KINK_MARGIN rms(u) of zero to that distance, on their own side; the statistics
    follow x, so repeat (two rounds suffice where a channel has more than two rows)"""
    live = d["C"] - d["npad"]
    for _ in range(6):
        x = d["x"]
        u = pre_activation(d)[:, :live]
        lim = 3 * KINK_MARGIN * float(u.pow(2).mean().sqrt())
        bad = u.abs() < lim
        if not bool(bad.any()):
            return
        target = torch.where(u < 0, -1.25 * lim, 1.25 * lim)
        if d["mode"] == "bare":
            xt = target
        else:
            if d["mode"] == "eval":
                mean, rstd = d["rm0"], (d["rv0"] + EPS).rsqrt()
            else:
                mean, _, rstd = batch_stats(x)
            xt = mean[:live] + (target - d["beta"][:live]) / (d["gamma"][:live] * rstd[:live])
        x = x.clone()
        x[:, :live] = torch.where(bad, xt, x[:, :live])
        d["x"] = r32(x)


def stage_inputs(rows, C, mode, seed=0, ratios=None, npad=0):
    """one stage case, fp64 tensors holding fp32 values: x, dy [rows, C], gamma in [0.5, 1.5], beta, the running statistics before the
    step (rm0 lags the batch mean by U[-0.5, 0.5] std: it is also the pivot), alpha.  Channel c has std in [0.5, 2] and mean / std =
    ratios[c % len(ratios)] (default: +-U[0.6, 1], which keeps the updated running mean away from zero); the draw is standardised
    per channel, so the ratios hold for the sample itself.  beta is drawn through shift = beta - mean * scale = +-U[0.1, 1] (eval:
    through the eval shift), so that no channel's shift is a difference around zero.  The last npad channels are the padding of a
    layer as the model holds it: x = 0, dy = 0, gamma = 0, rm0 = 0 -- and a beta of +-U[0.2, 0.5], so that y = act(beta) is visible."""
    g = _gen(rows, C, MODES.index(mode), seed, 41)
    live = C - npad
    z = torch.randn(rows, C, generator=g, dtype=F64)
    z = (z - z.mean(0)) / z.var(0, unbiased=False).sqrt()
    std = _uniform(g, 0.5, 2.0, C)
    rat = _signed(g, 0.6, 1.0, C)
    if ratios is not None:
        rat = torch.tensor([ratios[c % len(ratios)] for c in range(C)], dtype=F64)
    x = std * (z + rat)
    gamma, shift = _uniform(g, 0.5, 1.5, C), _signed(g, 0.1, 1.0, C)
    # the upstream gradient leans on xhat (slope +-U[0.5, 1] per channel), so that dgamma = sum du xhat is no sum around zero
    dy = torch.randn(rows, C, generator=g, dtype=F64) + _signed(g, 0.5, 1.0, C) * z
    lag = _uniform(g, -0.5, 0.5, C)
    rv_f = _uniform(g, 0.5, 2.0, C)
    if npad:
        x[:, live:], dy[:, live:], gamma[live:] = 0.0, 0.0, 0.0
    d = dict(rows=rows, C=C, mode=mode, seed=seed, npad=npad, ratios=ratios, x=r32(x), dy=r32(dy), gamma=r32(gamma),
             alpha=torch.tensor([ALPHA], dtype=F64))
    mean, var, rstd = batch_stats(d["x"])
    d["rm0"], d["rv0"] = r32(mean + lag * var.sqrt()), r32(rv_f * var + (var == 0) * 1.0)
    d["rm0"][live:] = 0.0
    beta = shift + (d["rm0"] * (d["rv0"] + EPS).rsqrt() if mode == "eval" else mean * rstd) * d["gamma"]
    if npad:
        beta[live:] = _signed(g, 0.2, 0.5, npad)
    d["beta"] = r32(beta)
    if mode != "bn_tanh":
        _unkink(d)
    return d


# ------------------------------------------------------------------------------------------------ truth / yardstick
PLANTS = ("biased_rv", "chunk_means", "no_xhat_term", "slope_ge", "onepass_fp32")


def _act(u, alpha, mode):
    return torch.tanh(u) if mode == "bn_tanh" else F.prelu(u, alpha)


def onepass_fp32(x):
    """The statistics as the kernels took them before the pivot, restated in torch: per 128-row chunk sixteen lanes add eight rows
    each in fp32 (sum and sum of rounded squares), the lanes are added in order in fp32, the chunks in fp64;
    var = Q / N - (S / N)^2.  Returns (mean, rstd), rounded to fp32 once as the kernel stores them."""
    x = x.float()
    rows, C = x.shape
    ch = (rows + STAT_ROWS - 1) // STAT_ROWS
    v = F.pad(x, (0, 0, 0, ch * STAT_ROWS - rows)).reshape(ch, STAT_ROWS // 16, 16, C)  # row = 16 i + lane: adding a zero row is exact
    s, q = torch.zeros(ch, 16, C), torch.zeros(ch, 16, C)
    for i in range(STAT_ROWS // 16):
        s = s + v[:, i]
        q = q + v[:, i] * v[:, i]
    S, Q = torch.zeros(ch, C), torch.zeros(ch, C)
    for lane in range(16):
        S = S + s[:, lane]
        Q = Q + q[:, lane]
    mean = S.double().sum(0) / rows
    var = (Q.double().sum(0) / rows - mean * mean).clamp_min(0.0)
    return mean.float(), (var + EPS).rsqrt().float()


def stage_truth(d, dtype, plant=None):
    """the stage in `dtype`.  train modes: mean, rstd, scale, shift, rm, rv (running statistics after the step), y, dx, dgamma,
    dbeta; PReLU modes: dalpha; all backward modes: colsum (column sums of dx).  eval: scale, shift, y.  The fp64 call also returns
    the sums of absolute terms behind the cancelling sums (dbeta_abs, colsum_abs, dalpha_abs).  plant: one deliberate mistake."""
    mode = d["mode"]
    c = lambda t: t.to(dtype)
    x = c(d["x"]).clone().requires_grad_(mode != "eval")
    gamma, beta, alpha = (c(d[k]).clone().requires_grad_(mode != "eval") for k in ("gamma", "beta", "alpha"))
    out = {}
    if mode == "eval":
        rstd = (c(d["rv0"]) + EPS).rsqrt()
        out["scale"] = gamma * rstd
        out["shift"] = beta - c(d["rm0"]) * out["scale"]
        out["y"] = _act(F.batch_norm(x, c(d["rm0"]), c(d["rv0"]), gamma, beta, False, MOMENTUM, EPS), alpha, mode)
        return out
    if mode == "bare":
        u = x
    else:
        rm, rv = c(d["rm0"]).clone(), c(d["rv0"]).clone()
        u = F.batch_norm(x, rm, rv, gamma, beta, True, MOMENTUM, EPS)
        var, mean = torch.var_mean(x.detach(), 0, unbiased=False)
        rstd = (var + EPS).rsqrt()
        if plant == "biased_rv":
            rv = (1 - MOMENTUM) * c(d["rv0"]) + MOMENTUM * var
        if plant == "chunk_means":  # the chunk means averaged as if every chunk were full
            mean = torch.stack([ch.mean(0) for ch in x.detach().split(STAT_ROWS)]).mean(0)
        if plant == "onepass_fp32":
            mean, rstd = (c(t) for t in onepass_fp32(x.detach()))
        scale = gamma.detach() * rstd
        out.update(mean=mean, rstd=rstd, scale=scale, shift=beta.detach() - mean * scale, rm=rm, rv=rv)
    y = _act(u, alpha, mode)
    y.backward(c(d["dy"]))
    out.update(y=y.detach(), dx=x.grad)
    if plant in ("chunk_means", "onepass_fp32"):
        out["y"] = _act(x.detach() * out["scale"] + out["shift"], alpha.detach(), mode)
    ud, dyd = u.detach(), c(d["dy"])
    du = dyd * ((1 - torch.tanh(ud) ** 2) if mode == "bn_tanh" else torch.where(ud > 0, torch.ones_like(ud), alpha.detach() * torch.ones_like(ud)))
    if mode != "bare":
        out.update(dgamma=gamma.grad, dbeta=beta.grad)
        if plant == "no_xhat_term":  # dx = gamma rstd (du - s0 / N - xhat s1 / N) without its last term
            xhat = (x.detach() - mean) * rstd
            out["dx"] = out["dx"] + scale * xhat * (du * xhat).sum(0) / d["rows"]
    if mode != "bn_tanh":
        out["dalpha"] = alpha.grad
        if plant == "slope_ge":  # the slope's gradient summed over the wrong side of the kink
            out["dalpha"] = (dyd * ud * (ud >= 0)).sum().reshape(1)
    out["colsum"] = out["dx"].sum(0)
    if dtype == F64:
        out.update(dbeta_abs=du.abs().sum(0), colsum_abs=out["dx"].abs().sum(0), dalpha_abs=(dyd * ud * (ud <= 0)).abs().sum().reshape(1))
    return out


# ------------------------------------------------------------------------------------------------ upsample / column sums
def up2_inputs(B, L, C, seed=0):
    g = _gen(B, L, C, seed, 42)
    rn = lambda *s: r32(torch.randn(*s, generator=g, dtype=F64))
    return dict(B=B, L=L, C=C, x=rn(B, L, C), dy=rn(B, 2 * L, C), dx0=rn(B, L, C))


def up2_truth(d, dtype, accumulate=False, plant=None):
    """y [B, 2L, C] = nn.Upsample(scale_factor=2, mode="linear") and dx (+ dx0 under accumulate).  plant "no_clamp": the backward
    without the edge clamp (the first and last input row lose the quarter that the clamped neighbour sends back)."""
    x = d["x"].to(dtype).clone().requires_grad_(True)
    y = F.interpolate(x.transpose(1, 2), scale_factor=2, mode="linear", align_corners=False).transpose(1, 2)
    dy = d["dy"].to(dtype)
    y.backward(dy)
    dx = x.grad
    if plant == "no_clamp":
        L = d["L"]
        e, o = dy[:, 0::2], dy[:, 1::2]
        nx = torch.cat([dy[:, 2::2], torch.zeros_like(dy[:, :1])], 1)   # dy[2 i + 2], nothing past the end
        pv = torch.cat([torch.zeros_like(dy[:, :1]), dy[:, 1:2 * L - 2:2]], 1)  # dy[2 i - 1], nothing before the start
        dx = 0.75 * (e + o) + 0.25 * (nx + pv)
    if accumulate:
        dx = dx + d["dx0"].to(dtype)
    return dict(y=y.detach(), dx=dx)


def colsum_inputs(rows, C, seed=0):
    g = _gen(rows, C, seed, 43)
    return dict(rows=rows, C=C, x=r32(torch.randn(rows, C, generator=g, dtype=F64) + 0.3), out0=r32(torch.randn(C, generator=g, dtype=F64)))


def colsum_truth(d, dtype, accumulate=False):
    s = d["x"].to(dtype).sum(0)
    return s + d["out0"].to(dtype) if accumulate else s


# ------------------------------------------------------------------------------------------------ the comparison
def _ch(t, C):
    """[rows, C] or [C] -> [C, rows]: one view row per channel"""
    return _cpu64(t).reshape(-1, C).t().contiguous()


def per_channel(name, got, t64, t32, C, factor=FACTOR):
    return _view(name + " /channel", _ch(got, C), _ch(t64, C), _ch(t32, C), factor)


def cancel_view(name, got, t64, t32, terms, factor=FACTOR):
    """a sum that cancels: kernel and yardstick error relative to the sum of the absolute terms (entries without terms: exactly 0)"""
    got, t64, t32, terms = (_cpu64(t).reshape(-1) for t in (got, t64, t32, terms))
    live = terms > 0
    ok = bool(torch.isfinite(got).all()) and bool((got[~live] == t64[~live]).all())
    if not bool(live.any()):
        return name + " /terms", 0.0, 0.0, FLOOR, ok
    err = float(((got - t64).abs()[live] / terms[live]).max())
    e32 = float(((t32 - t64).abs()[live] / terms[live]).max())
    bound = max(factor * e32, FLOOR)
    return name + " /terms", err, e32, bound, ok and math.isfinite(err) and err <= bound


def scaled_view(name, got, t64, t32, scale, factor=FACTOR):
    """per channel, relative to a given per-channel scale: the batch mean of the offset family in units of the channel's standard
    deviation (a channel at mean / std = 0 has a mean around 1e-8 std, which is no denominator)"""
    return (name + " /channel std",) + cancel_view(name, got, t64, t32, scale, factor)[1:]


def cold_rstd_bound(t64, pivot=None):
    """the derived per-channel bound on |drstd| / rstd of statistics taken about `pivot` (None: 0), see the module docstring"""
    var = (1.0 / t64["rstd"].double() ** 2 - EPS).clamp_min(0.0)
    dm = t64["mean"].double() - (0.0 if pivot is None else _cpu64(pivot))
    return 37.5 * U * (var + dm * dm) / (var + EPS) + 2 * U


def cold_rstd_view(name, got_rstd, t64, t32, pivot=None):
    """(name, worst |drstd| / rstd, the yardstick's, the derived bound of that channel, ok): every channel against its own bound"""
    rel = (_cpu64(got_rstd) - t64["rstd"]).abs() / t64["rstd"]
    bound = cold_rstd_bound(t64, pivot)
    i = int((rel / bound).argmax())
    e32 = float(((t32["rstd"].double() - t64["rstd"]).abs() / t64["rstd"]).max())
    return name + " /channel derived", float(rel[i]), e32, float(bound[i]), bool(torch.isfinite(rel).all()) and bool((rel <= bound).all())


def by_ratio(got, t64, ratios, what="rstd"):
    """{mean / std class: worst relative error of a per-channel vector in u}: the figures written next to the table"""
    rel = (_cpu64(got) - t64[what]).abs() / t64[what].abs()
    C = rel.shape[0]
    return {r: float(rel[[c for c in range(C) if c % len(ratios) == k]].max()) / U for k, r in enumerate(ratios)}


def global_maxnorm(got, t64):
    """the old tests' measure (test_gpu_kernels.relerr): one max-norm over the whole tensor"""
    return float((_cpu64(got) - t64.double()).abs().max() / t64.double().abs().max())


CHANNEL_KEYS = ("mean", "rstd", "scale", "shift", "rm", "rv", "dgamma")


def stage_views(t, C):
    """[(name, [C, n] truth)] of everything compared per channel: the tensors the conditions are asserted on"""
    return [(k, _ch(t[k], C)) for k in ("y", "dx") + CHANNEL_KEYS if k in t]


def stage_records(got, t64, t32, d, offset=False):
    """the views of one run of the stage; `got` holds what the launches produced, a missing entry is not compared.  offset: the
    offset family -- mean and the running mean in units of the channel's std, shift left to y (see scaled_view)."""
    C = d["C"]
    rec = []
    for k in ("y", "dx"):
        if k in got:
            rec += [per_row(k, got[k], t64[k], t32[k]), per_channel(k, got[k], t64[k], t32[k], C)]
    for k in CHANNEL_KEYS:
        if k not in got or k not in t64:
            continue
        if offset and k in ("mean", "rm"):
            rec.append(scaled_view(k, got[k], t64[k], t32[k], 1.0 / t64["rstd"]))
        elif not (offset and k == "shift"):
            rec.append(per_channel(k, got[k], t64[k], t32[k], C, FACTOR_SUMS if k == "dgamma" else FACTOR))
    for k in ("dbeta", "colsum", "dalpha"):
        if k in got and k in t64:
            rec.append(cancel_view(k, got[k], t64[k], t32[k], t64[k + "_abs"]))
    return rec


def stage_why(d, t64):
    """None, or the condition the case misses"""
    if kink_margin(d) <= KINK_MARGIN:
        return "kink"
    views = stage_views(t64, d["C"])
    if d["ratios"] is not None:  # the offset family: mean, rm and shift are not compared relative to themselves
        views = [(k, t) for k, t in views if k not in ("mean", "rm", "shift")] + [("std", (1.0 / t64["rstd"])[:, None])]
    return conditioned(views)


@functools.lru_cache(maxsize=None)
def stage_case(rows, C, mode, ratios=None):
    """(d, t64, t32) of the first seed that meets the conditions"""
    def make(seed):
        d = stage_inputs(rows, C, mode, seed, ratios, PADS.get(C, 0) if ratios is None and mode != "bare" else 0)
        t64 = stage_truth(d, F64)
        return dict(d=d, t64=t64, why=stage_why(d, t64))
    r = _search(make)
    return r["d"], r["t64"], stage_truth(r["d"], F32)


def all_stage_cases():
    """every (rows, C, mode, ratios) the GPU file runs"""
    cases = [(r, c, "bn_prelu", None) for r, c in SHAPE_CASES + LD_CASES + ACC_CASES] + [(r, c, "bn_tanh", None) for r, c in TANH_CASES]
    cases += [(r, c, "bare", None) for r, c in BARE_CASES] + [(r, c, "eval", None) for r, c in EVAL_CASES]
    cases += [(r, c, "bn_prelu", None) for r, c, _ in TRIP_CASES + WORLD2_CASES] + [(r, c, "bn_prelu", OFFSET_RATIOS) for r, c in OFFSET_CASES]
    return list(dict.fromkeys(cases))
