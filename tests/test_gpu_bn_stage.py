"""The BatchNorm + PReLU / tanh stage, the x2 upsample and the batched column sums on a real MI355X against fp64 truth and the fp32
yardstick of tests/bn_checks.py, channel by channel and row by row, driven through scrubvae_amd.ops the way ResVAE._bn_act /
_bn_act_bwd drive it: the single-launch path (bn_stats_finalize, bn_bwd_reduce) and the split path of sync-BN (bn_reduce_partials +
bn_finalize, parameter gradients from affine_prelu_bwd_apply).  Every output sits in a guarded buffer.  Run with -s for the GATE lines."""
import ctypes as C_

import pytest
import torch

from tests import bn_checks as K
from tests.bn_checks import F32, F64
from tests.conv_checks import check_guards, guarded

pytestmark = pytest.mark.gpu

GUARD = 777.0  # conv_checks.SENTINEL: what guard rows and guard columns hold


@pytest.fixture(scope="module")
def ops():
    from scrubvae_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


# ------------------------------------------------------------------------------------------------ device side of a case
def _mat(t, ld=None):
    """[rows, C] fp64 -> (buffer, view [rows, ld]) fp32 on the device; the columns past C and the rows past the end hold GUARD"""
    rows, C = t.shape
    buf, v = guarded(rows, ld or C, fill=GUARD)
    v[:, :C] = t.float().cuda()
    return buf, v


def _vec(C, init=None):
    """a guarded [C] vector: NaN (a launch has to write it) or a copy of `init`"""
    buf, v = guarded(1, C)
    if init is not None:
        v[0] = torch.as_tensor(init).float().cuda()
    return buf


def _out(buf, rows, C, ld, what):
    """the [rows, C] a launch wrote into a guarded [rows, ld] buffer, on the host; rows and columns past it untouched"""
    check_guards(buf, rows * ld, what, ld, C)
    got = buf[: rows * ld].view(rows, ld)[:, :C]
    assert bool(torch.isfinite(got).all()), f"{what}: elements left unwritten"
    return got.cpu()


class Stage:
    """the device tensors of rows [lo, hi) of a case"""

    def __init__(self, d, ld=None, lo=0, hi=None):
        hi = d["rows"] if hi is None else hi
        self.d, self.rows, self.C, self.ld = d, hi - lo, d["C"], ld or d["C"]
        self.x, _ = _mat(d["x"][lo:hi], self.ld)
        self.dy, _ = _mat(d["dy"][lo:hi], self.ld)
        dev = lambda t: t.float().cuda().contiguous()
        self.gamma, self.beta = dev(d["gamma"]), dev(d["beta"])
        self.alpha = None if d["mode"] == "bn_tanh" else dev(d["alpha"])
        self.nch = None

    def partials(self, ops, pivot):
        """forward statistics about `pivot` -> guarded [chunks, 2, C]"""
        self.nch = ops.bn_chunks(self.rows)
        assert self.nch == (self.rows + K.STAT_ROWS - 1) // K.STAT_ROWS
        buf, _ = guarded(self.nch * 2, self.C)
        ops.bn_stats_partial(self.x, self.rows, self.C, self.ld, buf, pivot)
        _out(buf, self.nch * 2, self.C, self.C, "bn_stats_partial")
        return buf

    def coeffs(self):
        return {k: _vec(self.C) for k in ("mean", "rstd", "scale", "shift")}

    def act(self, ops, co, bare=False):
        buf, _ = guarded(self.rows, self.ld, fill=GUARD)
        ops.affine_prelu_fwd(self.x, None if bare else co["scale"], None if bare else co["shift"], self.alpha, buf, self.rows, self.C, self.ld)
        return _out(buf, self.rows, self.C, self.ld, "affine_prelu_fwd")

    def bwd_partials(self, ops, co, bare=False):
        """first backward pass -> (guarded [chunks, 2, C], guarded slope partials, their count)"""
        n_dap = 2 * self.nch * ((self.C + 63) // 64)
        bufp, _ = guarded(self.nch * 2, self.C)
        bufa, _ = guarded(n_dap, 1)
        g = lambda k: None if bare else co[k]
        ops.affine_prelu_bwd_partial(self.dy, self.x, g("scale"), g("shift"), g("mean"), g("rstd"), self.alpha, self.rows, self.C, self.ld,
                                     bufp, bufa)
        _out(bufp, self.nch * 2, self.C, self.C, "affine_prelu_bwd_partial")
        _out(bufa, n_dap, 1, 1, "slope partials")
        return bufp, bufa, n_dap


def _host(buf, C):
    v = buf[:C]
    check_guards(buf, C, "per-channel vector")
    assert bool(torch.isfinite(v).all()), "per-channel vector left unwritten"
    return v.cpu()


def _colsum_of(ops, s, cp, n, accumulate):
    out = _vec(s.C, torch.full((s.C,), K.STALE))
    batch = ops.ColsumBatch()
    batch.add_partials(cp, n, s.C, out)
    batch.flush(lambda nbytes: torch.empty(nbytes // 4 + 16, device="cuda"), accumulate=accumulate)
    return _host(out, s.C)


def run_stage(ops, d, path, pivoted=True, ld=None, accumulate=False, colsum=False):
    """one training step of the stage on the whole batch, as ResVAE._bn_act + _bn_act_bwd run it on one rank (path "single") or
    under sync-BN (path "split").  The pivot is the running-mean buffer itself, as in the model."""
    s = Stage(d, ld)
    C, rows, mode = s.C, s.rows, d["mode"]
    got = {}
    if mode == "eval":
        co = {k: _vec(C) for k in ("scale", "shift")}
        ops.bn_eval_coeffs(C, s.gamma, s.beta, K.EPS, d["rm0"].float().cuda(), d["rv0"].float().cuda(), co["scale"], co["shift"])
        got.update({k: _host(co[k], C) for k in co}, y=s.act(ops, co))
        return got
    bare = mode == "bare"
    co = None
    if not bare:
        rm, rv = _vec(C, d["rm0"]), _vec(C, d["rv0"])
        pivot = rm if pivoted else None
        part = s.partials(ops, pivot)
        co = s.coeffs()
        if path == "single":
            nbt = torch.zeros((), dtype=torch.long, device="cuda")
            ops.bn_stats_finalize(part, s.nch, rows, C, s.gamma, s.beta, K.EPS, K.MOMENTUM, rm, rv, nbt, co["mean"], co["rstd"],
                                  co["scale"], co["shift"], pivot)
            assert int(nbt) == 1
        else:
            sums = _vec(2 * C)
            ops.bn_reduce_partials(part, s.nch, C, sums)
            check_guards(sums, 2 * C, "bn_reduce_partials sums")
            ops.bn_finalize(sums, rows, C, s.gamma, s.beta, K.EPS, K.MOMENTUM, rm, rv, co["mean"], co["rstd"],
                            co["scale"], co["shift"], pivot)
        got.update({k: _host(co[k], C) for k in co}, rm=_host(rm, C), rv=_host(rv, C))
    else:
        s.nch = ops.bn_chunks(rows)
    got["y"] = s.act(ops, co, bare)
    # backward
    bufp, bufa, n_dap = s.bwd_partials(ops, co, bare)
    stale = torch.full((C,), K.STALE)
    dg, db, da = _vec(C, stale), _vec(C, stale), _vec(1, stale[:1])
    dxb, _ = guarded(rows, s.ld, fill=GUARD)
    n_cs = ops.affine_prelu_colsum_rows(rows, C) if colsum else 0
    assert not colsum or n_cs > 0
    cp = guarded(n_cs, C)[0] if n_cs else None
    g = lambda k: None if bare else co[k]
    da_arg = None if s.alpha is None else da
    if bare:
        ops.affine_prelu_bwd_apply(s.dy, s.x, None, None, None, None, None, s.alpha, None, 1.0, dxb, rows, C, s.ld, None, None, da_arg,
                                   bufa, n_dap, accumulate, colsum_part=cp)
    elif path == "single":
        sums = _vec(2 * C)
        ops.bn_bwd_reduce(bufp, s.nch, C, sums, dg, db, da_arg, bufa, n_dap, accumulate)
        ops.affine_prelu_bwd_apply(s.dy, s.x, g("scale"), g("shift"), g("mean"), g("rstd"), s.gamma, s.alpha, sums, rows, dxb, rows, C,
                                   s.ld, None, None, None, bufa, n_dap, accumulate, colsum_part=cp)
        check_guards(sums, 2 * C, "bn_bwd_reduce sums")
    else:
        sums = _vec(2 * C)
        ops.bn_reduce_partials(bufp, s.nch, C, sums)
        ops.affine_prelu_bwd_apply(s.dy, s.x, g("scale"), g("shift"), g("mean"), g("rstd"), s.gamma, s.alpha, sums, rows, dxb, rows, C,
                                   s.ld, dg, db, da_arg, bufa, n_dap, accumulate, colsum_part=cp)
        check_guards(sums, 2 * C, "bn_reduce_partials sums")
    got["dx"] = _out(dxb, rows, C, s.ld, "affine_prelu_bwd_apply")
    if not bare:
        got.update(dgamma=_host(dg, C), dbeta=_host(db, C))
    if s.alpha is not None:
        got["dalpha"] = _host(da, 1)
    if n_cs:
        _out(cp, n_cs, C, C, "column-sum partials")
        got["colsum"] = _colsum_of(ops, s, cp, n_cs, accumulate)
    return got


def _accumulated(t, accumulate):
    """the truth / yardstick of a run whose gradient tensors held STALE: added to under accumulate (the column sums likewise)"""
    if not accumulate:
        return t
    t = dict(t)
    for k in ("dgamma", "dbeta", "dalpha", "colsum"):
        if k in t:
            t[k] = t[k] + K.STALE
    return t


def _check_pads(d, got):
    """the padding of a layer: exact y = act(beta) in every row (PReLU: beta, or the rounded product alpha * beta) and dx = 0"""
    if not d["npad"]:
        return
    pad = slice(d["C"] - d["npad"], d["C"])
    assert d["mode"] == "eval" or float(got["dx"][:, pad].abs().max()) == 0.0
    if d["mode"] == "bn_tanh":
        # tanh(beta), the same in every row.  Not bit for bit: the device's tanhf and torch's differ in the last place, so each
        # channel is held to the y gate, FACTOR times what torch's own fp32 tanh misses the fp64 value by (FLOOR at least)
        assert bool((got["y"][:, pad] == got["y"][:1, pad]).all())
        b = d["beta"][pad]
        t64, t32 = torch.tanh(b), torch.tanh(b.float()).double()
        bound = ((t32 - t64).abs() / t64.abs() * K.FACTOR).clamp_min(K.FLOOR)
        assert bool(((got["y"][0, pad].double() - t64).abs() / t64.abs() <= bound).all())
    else:
        b = d["beta"][pad].float()
        assert torch.equal(got["y"][:, pad], torch.where(b > 0, b, torch.tensor(K.ALPHA) * b).expand(d["rows"], -1))


def _run_and_gate(ops, tag, case, path, **kw):
    d, t64, t32 = K.stage_case(*case)
    got = run_stage(ops, d, path, **kw)
    acc = kw.get("accumulate", False)
    K.gate(tag, K.stage_records(got, _accumulated(t64, acc), _accumulated(t32, acc), d, offset=case[3] is not None))
    _check_pads(d, got)
    return d, t64, t32, got


PATHS = ["single", "split"]
STAGE_PARAMS = ([(r, c, "bn_prelu", None) for r, c in K.SHAPE_CASES] + [(r, c, "bn_tanh", None) for r, c in K.TANH_CASES]
                + [(r, c, "bare", None) for r, c in K.BARE_CASES] + [(r, c, "eval", None) for r, c in K.EVAL_CASES])
OFFSET_PARAMS = [(r, c, "bn_prelu", K.OFFSET_RATIOS) for r, c in K.OFFSET_CASES]
# every (rows, C, mode, ratios) this file runs: test_bn_stage_cpu.py holds each of them to the conditions
STAGE_CASES_RUN = (STAGE_PARAMS + OFFSET_PARAMS + [(r, c, "bn_prelu", None) for r, c, _ in K.TRIP_CASES + K.WORLD2_CASES]
                   + [(r, c, "bn_prelu", None) for r, c in K.LD_CASES + K.ACC_CASES])
_id = lambda c: f"{c[2]}-{c[0]}x{c[1]}"


# ------------------------------------------------------------------------------------------------ the families
@pytest.mark.parametrize("case,path", [(c, p) for c in STAGE_PARAMS for p in (PATHS if c[2].startswith("bn_") else PATHS[:1])],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_shape_family(ops, case, path):
    """(bare and eval have no statistics, hence one path)"""
    colsum = (path == "split" or case[2] == "bare") and case[2] != "eval" and ops.affine_prelu_colsum_rows(case[0], case[1]) > 0
    _run_and_gate(ops, f"shape {_id(case)} {path}", case, path, colsum=colsum)


@pytest.mark.parametrize("rows,C,colsum", K.TRIP_CASES)
def test_trip_family(ops, rows, C, colsum):
    _run_and_gate(ops, f"trips {rows}x{C}", (rows, C, "bn_prelu", None), "single", colsum=colsum)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("rows,C", K.LD_CASES)
def test_ld_family(ops, rows, C, path):
    colsum = ops.affine_prelu_colsum_rows(rows, C) > 0
    _run_and_gate(ops, f"ld {rows}x{C}+16 {path}", (rows, C, "bn_prelu", None), path, ld=C + 16, colsum=colsum)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("rows,C", K.ACC_CASES)
def test_accumulate_family(ops, rows, C, path, accumulate):
    colsum = ops.affine_prelu_colsum_rows(rows, C) > 0
    _run_and_gate(ops, f"acc={int(accumulate)} {rows}x{C} {path}", (rows, C, "bn_prelu", None), path, accumulate=accumulate, colsum=colsum)


@pytest.mark.parametrize("rows,C,r0", K.WORLD2_CASES)
def test_world2_family(ops, rows, C, r0):
    """two ranks with unequal shares of the batch on one device: statistics per rank, their [2, C] sums added in fp32 (the
    all-reduce), bn_finalize(count = all rows); backward likewise, the global sums into affine_prelu_bwd_apply(count = all rows),
    the local ones into the parameter gradients.  The truth is BatchNorm over all rows."""
    d, t64, t32 = K.stage_case(rows, C, "bn_prelu")
    ranks = [Stage(d, None, 0, r0), Stage(d, None, r0, rows)]
    rms = [_vec(C, d["rm0"]) for _ in ranks]  # identical on every rank, before and after
    rvs = [_vec(C, d["rv0"]) for _ in ranks]
    local = []
    for s, rm in zip(ranks, rms):
        sums = _vec(2 * C)
        ops.bn_reduce_partials(s.partials(ops, rm), s.nch, C, sums)
        local.append(_host(sums, 2 * C).cuda())
    glob = local[0] + local[1]
    cos = []
    for s, rm, rv in zip(ranks, rms, rvs):
        co = s.coeffs()
        ops.bn_finalize(glob, rows, C, s.gamma, s.beta, K.EPS, K.MOMENTUM, rm, rv, co["mean"], co["rstd"], co["scale"], co["shift"], rm)
        cos.append(co)
    got = {k: _host(cos[0][k], C) for k in cos[0]}
    got.update(rm=_host(rms[0], C), rv=_host(rvs[0], C))
    for k in cos[0]:
        assert torch.equal(_host(cos[1][k], C), got[k])
    assert torch.equal(_host(rms[1], C), got["rm"]) and torch.equal(_host(rvs[1], C), got["rv"])
    got["y"] = torch.cat([s.act(ops, co) for s, co in zip(ranks, cos)])
    back = [s.bwd_partials(ops, co) for s, co in zip(ranks, cos)]
    local = []
    for s, (bufp, _, _) in zip(ranks, back):
        sums = _vec(2 * C)
        ops.bn_reduce_partials(bufp, s.nch, C, sums)
        local.append(_host(sums, 2 * C).cuda())
    glob = local[0] + local[1]
    dx, da_sum = [], torch.zeros(1, dtype=F64)
    for s, co, (_, bufa, n_dap) in zip(ranks, cos, back):
        dxb, _ = guarded(s.rows, C, fill=GUARD)
        da = _vec(1, [K.STALE])
        ops.affine_prelu_bwd_apply(s.dy, s.x, co["scale"], co["shift"], co["mean"], co["rstd"], s.gamma, s.alpha, glob, rows, dxb, s.rows,
                                   C, C, None, None, da, bufa, n_dap, False)
        dx.append(_out(dxb, s.rows, C, C, "affine_prelu_bwd_apply"))
        da_sum += _host(da, 1).double()
    got["dx"] = torch.cat(dx)
    both = (local[0].double() + local[1].double()).cpu()  # the gradient all-reduce adds the ranks' local parameter gradients
    got.update(dbeta=both[:C], dgamma=both[C:], dalpha=da_sum)
    K.gate(f"world2 {rows}x{C} ({r0} + {rows - r0})", K.stage_records(got, t64, t32, d))
    _check_pads(d, got)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", OFFSET_PARAMS, ids=_id)
def test_offset_family_with_a_pivot(ops, case, path):
    d, t64, t32, got = _run_and_gate(ops, f"offset {_id(case)} {path}", case, path)
    print(f"GATE offset {_id(case)} {path} | rstd error in u by mean / std:", {r: round(v, 1) for r, v in K.by_ratio(got["rstd"], t64, K.OFFSET_RATIOS).items()})


@pytest.mark.parametrize("case", OFFSET_PARAMS, ids=_id)
def test_offset_family_cold(ops, case):
    """no pivot: the error is the one-pass algorithm's; gated by the derived bound (bn_checks docstring), and printed against the
    yardstick multiple that the pivoted run is held to, to show what the first steps of a run, before running_mean has followed
    the batch mean, still cost"""
    d, t64, t32 = K.stage_case(*case)
    got = run_stage(ops, d, "single", pivoted=False)
    rec = K.per_channel("rstd cold (not asserted)", got["rstd"], t64["rstd"], t32["rstd"], d["C"])
    print(f"GATE cold {_id(case)} | {rec[0]}: err {rec[1]:.3e} e32 {rec[2]:.3e} ratio {K.ratio(rec):.2f} {'ok' if rec[4] else 'beyond FACTOR'}")
    held = K.FACTOR * max(rec[2], K.U) / K.U  # what the pivoted run of the same case is held to, in u
    for r, v in K.by_ratio(got["rstd"], t64, K.OFFSET_RATIOS).items():
        print(f"GATE cold {_id(case)} | rstd at mean / std {r:g}: {v:.1f} u against FACTOR * E32 = {held:.1f} u: "
              f"{'within' if v <= held else 'MISSES'} the pivoted run's gate")
    K.gate(f"cold {_id(case)}", [K.cold_rstd_view("rstd", got["rstd"], t64, t32)])


@pytest.mark.parametrize("rows,C", [(37, 48), (700, 144), (4133, 512)])
def test_null_pivot_is_a_pivot_of_zeros(ops, rows, C):
    """with no pivot every partial has the bits it had before the pivot existed: x - 0 is x"""
    d, _, _ = K.stage_case(rows, C, "bn_prelu")
    s = Stage(d)
    a = s.partials(ops, None)
    b = s.partials(ops, torch.zeros(C, device="cuda"))
    assert torch.equal(a, b)
    co_a, co_b = s.coeffs(), s.coeffs()
    for co, piv in ((co_a, None), (co_b, torch.zeros(C, device="cuda"))):
        ops.bn_stats_finalize(a, s.nch, rows, C, s.gamma, s.beta, K.EPS, K.MOMENTUM, None, None, None, co["mean"], co["rstd"], co["scale"],
                              co["shift"], piv)
    for k in co_a:
        assert torch.equal(co_a[k], co_b[k])


# ------------------------------------------------------------------------------------------------ upsample, column sums
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("wide", [0, 16])
@pytest.mark.parametrize("B,L,C", K.UP2_CASES)
def test_upsample2_family(ops, B, L, C, wide, accumulate):
    d = K.up2_inputs(B, L, C)
    t64, t32 = K.up2_truth(d, F64, accumulate), K.up2_truth(d, F32, accumulate)
    ld = C + wide
    xb, _ = _mat(d["x"].reshape(B * L, C), ld)
    yb, _ = guarded(B * 2 * L, ld, fill=GUARD)
    ops.upsample2_fwd(xb, yb, B, L, C, ld)
    y = _out(yb, B * 2 * L, C, ld, "upsample2_fwd")
    dyb, _ = _mat(d["dy"].reshape(B * 2 * L, C), ld)
    dxb, _ = _mat(d["dx0"].reshape(B * L, C), ld)  # stale content: added to under accumulate, overwritten without
    ops.upsample2_bwd(dyb, dxb, B, L, C, ld, accumulate=accumulate)
    dx = _out(dxb, B * L, C, ld, "upsample2_bwd")
    f2, f1 = (lambda t: t.reshape(B * 2 * L, C)), (lambda t: t.reshape(B * L, C))
    K.gate(f"up2 B{B} L{L} C{C} ld{ld} acc={int(accumulate)}",
           [K.per_row("y", y, f2(t64["y"]), f2(t32["y"])), K.per_channel("y", y, f2(t64["y"]), f2(t32["y"]), C),
            K.per_row("dx", dx, f1(t64["dx"]), f1(t32["dx"])), K.per_channel("dx", dx, f1(t64["dx"]), f1(t32["dx"]), C)])


@pytest.mark.parametrize("accumulate", [False, True])
def test_column_sum_family(ops, accumulate):
    """ColsumBatch.add (matrices of different C and ld in one flush) and add_partials (partials another kernel left behind)"""
    batch, want = ops.ColsumBatch(), []
    for i, (rows, C, ld, kind) in enumerate(K.COLSUM_TASKS):
        d = K.colsum_inputs(rows, C, seed=i)
        xb, _ = _mat(d["x"], ld)
        out = _vec(C, d["out0"])
        if kind == "partials":
            batch.add_partials(xb, rows, C, out)
        else:
            batch.add(xb, rows, C, ld, out)
        want.append((f"{kind} {rows}x{C} ld{ld}", d, out, xb))
    batch.flush(lambda nbytes: torch.empty(nbytes // 4 + 16, device="cuda"), accumulate=accumulate)
    rec = []
    for name, d, out, _ in want:
        rec.append(K.cancel_view(name, _host(out, d["C"]), K.colsum_truth(d, F64, accumulate), K.colsum_truth(d, F32, accumulate),
                                 d["x"].abs().sum(0) + (d["out0"].abs() if accumulate else 0.0)))
    K.gate(f"colsum acc={int(accumulate)}", rec)


# ------------------------------------------------------------------------------------------------ the conv epilogues' statistics
def _conv_setup(ops, idx, code, pieces):
    """CONV_CASES[idx] with a bias that puts output channel c at mean / std = CONV_RATIOS[c % 2], on the tile `code`"""
    import torch.nn.functional as F

    from tests.test_gpu_kernels import CONV_CASES, to_nlc
    B, L, Cin, Cout, k, s, p, tr = CONV_CASES[idx]
    g = K._gen(idx, code, 44)
    x = K.r32(torch.randn(B, Cin, L, generator=g, dtype=F64))
    w = K.r32(torch.randn(*((Cin, Cout, k) if tr else (Cout, Cin, k)), generator=g, dtype=F64) / (Cin * k) ** 0.5)
    y0 = (F.conv_transpose1d if tr else F.conv1d)(x, w, None, stride=s, padding=p)
    m0, s0 = y0.mean((0, 2)), y0.var((0, 2), unbiased=False).sqrt()
    rat = torch.tensor([K.CONV_RATIOS[c % 2] for c in range(Cout)], dtype=F64)
    bias = K.r32(rat * s0 - m0)
    cv = ops.Conv(B, L, Cin, Cout, k, s, p, 1, tr, pieces=pieces)
    cv.__dict__["_tuned"] = {"fwd", "dgrad", "wgrad"}
    cv.desc.tile[0] = code
    ops.bump_weight_epoch()
    wd = ops.conv_weight_to_tio(w.float(), tr).cuda().contiguous()
    bd = torch.zeros(cv.c_out_p)
    bd[:Cout] = bias.float()
    assert cv.c_out_p == Cout
    return cv, to_nlc(x), wd, bd.cuda(), rat


@pytest.mark.parametrize("idx,code,pieces,epilogue", K.CONV_STAT_CASES)
def test_conv_epilogue_statistics(ops, idx, code, pieces, epilogue):
    """statistics fused into a split conv forward, finalized as ResVAE._bn_act does, against the fp64 BatchNorm of the conv output
    the launch wrote: one case on the 32 x 32 epilogue (tile_epilogue), one on tile_epilogue16, output channels at mean / std 4 and
    16, with a pivot (FACTOR) and cold (derived bound); a NULL pivot gives the bits of a pivot of zeros"""
    from scrubvae_amd import _lib
    cv, xd, wd, bd, rat = _conv_setup(ops, idx, code, pieces)
    bm, bn, variant, rmax = C_.c_int(), C_.c_int(), C_.c_int(), C_.c_int()
    assert _lib.lib().svae_conv_split_tile(C_.byref(cv.desc), 0, C_.byref(bm), C_.byref(bn), C_.byref(variant), C_.byref(rmax)) == 0
    assert (variant.value == 18) == (epilogue == "tile_epilogue16"), variant.value  # 18: the 16 x 16 MFMA kernel, the only user of tile_epilogue16
    nt, rows, C = cv.stats_tiles(), cv.batch * cv.l_out, cv.c_out_p
    assert nt > 0

    def launch(pivot):
        yb, _ = guarded(rows, C)
        pb, _ = guarded(nt * 2, C)
        cv.fwd(xd, wd, bd, yb, stats=pb, pivot=pivot)
        _out(pb, nt * 2, C, C, "fused statistics")
        return yb, pb, _out(yb, rows, C, C, "conv output")

    yb0, p_none, y_conv = launch(None)
    yb1, p_zero, _ = launch(torch.zeros(C, device="cuda"))
    assert torch.equal(p_none, p_zero) and torch.equal(yb0, yb1)
    # the stage behind the conv: its input is the conv output as written
    g = K._gen(idx, 45)
    gamma, beta = K.r32(K._uniform(g, 0.5, 1.5, C)), K.r32(K._uniform(g, -0.5, 0.5, C))
    mean, var, _ = K.batch_stats(y_conv)
    d = dict(rows=rows, C=C, mode="bn_prelu", npad=0, ratios=K.CONV_RATIOS, x=y_conv.double(), dy=torch.zeros(rows, C, dtype=F64),
             gamma=gamma, beta=beta, alpha=torch.tensor([K.ALPHA], dtype=F64), rm0=K.r32(mean + K._uniform(g, -0.5, 0.5, C) * var.sqrt()),
             rv0=K.r32(var))
    assert float((mean / var.sqrt() - rat).abs().max()) < 0.05  # the conv output sits at the ratios
    t64, t32 = K.stage_truth(d, F64), K.stage_truth(d, F32)
    gd, btd, ad = gamma.float().cuda(), beta.float().cuda(), torch.tensor([K.ALPHA], device="cuda")
    for cold in (False, True):
        rm, rv = _vec(C, d["rm0"]), _vec(C, d["rv0"])
        pivot = None if cold else rm
        yb, pb, y_again = launch(pivot)
        assert torch.equal(y_again, y_conv)
        co = {k: _vec(C) for k in ("mean", "rstd", "scale", "shift")}
        ops.bn_stats_finalize(pb, nt, rows, C, gd, btd, K.EPS, K.MOMENTUM, rm, rv, None, co["mean"], co["rstd"], co["scale"], co["shift"], pivot)
        ab, _ = guarded(rows, C)
        ops.affine_prelu_fwd(yb, co["scale"], co["shift"], ad, ab, rows, C, C)
        got = {k: _host(co[k], C) for k in co}
        got.update(y=_out(ab, rows, C, C, "affine_prelu_fwd"), rm=_host(rm, C), rv=_host(rv, C))
        tag = f"conv {epilogue} {'cold' if cold else 'pivot'}"
        print(f"GATE {tag} | rstd error in u by mean / std:", {r: round(v, 1) for r, v in K.by_ratio(got["rstd"], t64, K.CONV_RATIOS).items()})
        if cold:
            K.gate(tag, [K.cold_rstd_view("rstd", got["rstd"], t64, t32)])
        else:
            K.gate(tag, [K.per_channel(k, got[k], t64[k], t32[k], C) for k in ("rstd", "mean", "scale", "rm", "rv", "y")]
                   + [K.per_row("y", got["y"], t64["y"], t32["y"])])
    # Accumulating onto a previous content, with a pivot: what the second conv of a residual block launches (the statistics of
    # skip + residual).  On the kernels that have one (variants 0 .. 3, 8, 9, 19, 29: test_gpu_epilogue.py) an accumulating launch
    # takes the 16-byte epilogue, which loads the pivot per accumulator column like the dword path: switched off and on the launch
    # has to leave the same bits, and its statistics are those of what it wrote.
    piv2 = _vec(C, 2 * d["rm0"])  # the content doubles, mean and std with it
    keep, runs = ops.EPILOGUE_WIDE, {}
    try:
        for wide in (False, True):
            ops.set_epilogue_wide(wide)
            yb, _ = guarded(rows, C)
            yb[: rows * C] = yb0[: rows * C]
            pb, _ = guarded(nt * 2, C)
            cv.fwd(xd, wd, bd, yb, accumulate=True, stats=pb, pivot=piv2)
            _out(pb, nt * 2, C, C, "fused statistics (accumulate)")
            runs[wide] = (yb, pb, _out(yb, rows, C, C, "conv output (accumulate)"))
    finally:
        ops.set_epilogue_wide(keep)
    assert torch.equal(runs[False][0], runs[True][0]) and torch.equal(runs[False][1], runs[True][1])
    yb, pb, y_acc = runs[True]
    mean2, var2, _ = K.batch_stats(y_acc)
    assert float((mean2 / var2.sqrt() - rat).abs().max()) < 0.05
    d2 = dict(d, x=y_acc.double(), rm0=2 * d["rm0"], rv0=K.r32(var2))
    t64, t32 = K.stage_truth(d2, F64), K.stage_truth(d2, F32)
    rv = _vec(C, d2["rv0"])
    co = {k: _vec(C) for k in ("mean", "rstd", "scale", "shift")}
    ops.bn_stats_finalize(pb, nt, rows, C, gd, btd, K.EPS, K.MOMENTUM, piv2, rv, None, co["mean"], co["rstd"], co["scale"], co["shift"], piv2)
    got = {k: _host(co[k], C) for k in co}
    got.update(rm=_host(piv2, C), rv=_host(rv, C))
    K.gate(f"conv {epilogue} accumulate pivot", [K.per_channel(k, got[k], t64[k], t32[k], C) for k in ("rstd", "mean", "scale", "rm", "rv")])


# ------------------------------------------------------------------------------------------------ the model's switch
def test_model_bn_pivot_switch(ops):
    """ResVAE.bn_pivot hands every BatchNorm's running mean to its statistics producer (conv epilogue or bn_stats_partial) and to
    its finalize.  The first train-mode forward finds running means of zero: a pivot of zeros, the bits of the model without the
    switch.  Later forwards sum about the moving running mean: the same mathematics, so outputs and running statistics stay within
    the project's 1e-4 agreement bound between its arithmetic variants (a producer and a finalize that disagreed about the pivot
    would be off by the running mean itself)."""
    from oracle import scvae_oracle as O
    from tests.test_gpu_model import ARENA, build_model, to_dev
    cfg = O.OracleConfig(n_keypts=18, window=64, z_dim=8, kernel=5, channel=(16, 16, 16, 32, 32), diag=True, arena_size=ARENA)
    sd = O.init_state_dict(cfg, seed=5)
    data = to_dev(O.synth_batch(cfg, 8, seed=5))
    data["eps"] = torch.randn(8, 8, generator=torch.Generator().manual_seed(3)).cuda()
    runs = {}
    for on in (False, True):
        m, _ = build_model(cfg, sd)
        m.bn_pivot = on
        m.train()
        snaps = []
        with torch.no_grad():
            for _ in range(3):
                o = m(data)
                snaps.append((o["x6d"].clone(), o["mu"].clone(), {k: v.clone() for k, v in m.state_dict().items() if "running_" in k}))
        runs[on] = snaps
    rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
    x0, mu0, st0 = runs[False][0]
    x1, mu1, st1 = runs[True][0]
    assert torch.equal(x0, x1) and torch.equal(mu0, mu1) and all(torch.equal(st0[k], st1[k]) for k in st0)
    moved = max(float(v.abs().max()) for k, v in st1.items() if "running_mean" in k)
    assert moved > 1e-3  # the later forwards do have a pivot
    for (xa, ma, sa), (xb, mb, sb) in zip(runs[False][1:], runs[True][1:]):
        assert rel(xb, xa) < 1e-4 and rel(mb, ma) < 1e-4
        assert all(rel(sb[k], sa[k]) < 1e-4 for k in sa)
