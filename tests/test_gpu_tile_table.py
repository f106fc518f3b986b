"""Every entry of the shipped tile table (scrubvae_amd/tuned_tiles.json) at the size it runs at in the benchmark, against a float64
reference of the same operation computed on the device.

One test per table key: the Conv is rebuilt from the key, `Conv._tune` takes the table path (nothing is forced, nothing is timed), and
the one pass the key names runs on random fp32 inputs at the key's batch and shape.  Checked for each pass:
  * the whole output against fp64, under the split kernels' tolerance of test_gpu_kernels (`_SPLIT_TOL[pieces] * sqrt(K) + tol`;
    2e-6 per sqrt(K) for the fp32 kernels), and the rms error of the worst 256-row block (weight gradients: (tap, 128 x 128)
    block) within 4x that of the median block -- one bad tile cannot hide under a global max-norm;
  * every output element written (NaN-filled before), nothing written past the end (guard rows / guard columns beyond c_out where
    ld_out is wider, bit-identical afterwards), pad channels zero, and `accumulate=True` adding onto the previous content;
  * the epilogues: the forward's BatchNorm statistics, the data-gradient's fused BatchNorm + PReLU backward sums (svae_conv_dgrad_split_bn
    + svae_bn_bwd_reduce, as ResVAE._bn_act_bwd uses them) and the up2 forwards' upsampled by-product.

The fp64 reference runs on the GPU as a sum over taps of shifted fp64 matmuls (test_device_reference_matches_cpu checks it against
torch's CPU convolutions).  Run with `-s` for one line per entry and a per-family summary at the end of the module."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.conv_checks import (SENTINEL, check_guards, err_bound, guarded, row_block_ratio, w_block_ratio, bn_bwd_fused_check,
                                ref_dgrad, ref_fwd, ref_up2, ref_wgrad)
from tests.test_gpu_kernels import CONV_CASES, _SPLIT_TOL
from tests.test_tile_table_keys import KEYS, parse_key

PAD = 5  # channels at the end of each padded width that are zero padding (as for the model's 141 -> 144 output conv)
BLOCK_RATIO = 4.0
_REPORT = {}  # kernel family -> dict of worst figures (printed at the end of the module)


@pytest.mark.parametrize("case", CONV_CASES + [("up2", 3, 9, 48, 40, 6, 1, 2, False)])
def test_device_reference_matches_cpu(case):
    """The device reference (shifted fp64 matmuls) against torch's CPU convolutions and their autograd in fp64."""
    up2 = case[0] == "up2"
    B, L, Cin, Cout, k, s, p, tr = case[1:] if up2 else case
    g = torch.Generator().manual_seed(sum(case[-8:-1]))
    x = torch.randn(B, Cin, L, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(*((Cin, Cout, k) if tr else (Cout, Cin, k)), generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Cout, generator=g, dtype=torch.float64, requires_grad=True)
    xin = F.interpolate(x, scale_factor=2, mode="linear", align_corners=False) if up2 else x
    y = (F.conv_transpose1d if tr else F.conv1d)(xin, w, b, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    wt = (w.detach().permute(2, 0, 1) if tr else w.detach().permute(2, 1, 0)).contiguous().cuda()  # [k, Cin, Cout]
    xd = x.detach().transpose(1, 2).contiguous().cuda()
    xu = ref_up2(xd) if up2 else xd
    yd = ref_fwd(xu, wt, b.detach().cuda(), y.shape[-1], s, p, 1, tr)
    rel = lambda a, r: float((a.cpu() - r).abs().max() / r.abs().max())
    assert rel(yd.transpose(1, 2), y.detach()) < 1e-12
    if up2:
        assert rel(xu.transpose(1, 2), xin.detach()) < 1e-12
        return
    dyd = dy.transpose(1, 2).contiguous().cuda()
    assert rel(ref_dgrad(dyd, wt, L, s, p, 1, tr).transpose(1, 2), x.grad) < 1e-12
    dw, db = ref_wgrad(xd, dyd, k, s, p, 1, tr)
    assert rel(dw.permute(1, 2, 0) if tr else dw.permute(2, 1, 0), w.grad) < 1e-12
    assert rel(db, b.grad) < 1e-12


def _note(family, **vals):
    d = _REPORT.setdefault(family, {})
    for k, v in vals.items():
        d[k] = max(d.get(k, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    import time
    t0 = time.time()
    yield
    print(f"\n[tile table] {time.time() - t0:.0f} s; worst figures per kernel family (error / bound, worst / median block rms):")
    for fam in sorted(_REPORT):
        print("  " + fam + ": " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_REPORT[fam].items())))


def _family(name):
    return name.split("<")[0] + ("<256, 256" if name.split("<")[1].startswith("256, 256") else "")


def _stats_check(part, nt, y, what):
    """Forward BatchNorm partials [nt, 2, N] of the written y [rows, N]: tile sums in fp64 against column sums, 2e-5 of sum |y| / y^2."""
    assert not torch.isnan(part[:nt]).any(), f"{what}: stats partials left unwritten"
    s = part[:nt].double().sum(0)
    yd = y.double()
    d0 = (s[0] - yd.sum(0)).abs() / yd.abs().sum(0).clamp_min(1e-300)
    y2 = yd * yd
    d1 = (s[1] - y2.sum(0)).abs() / y2.sum(0).clamp_min(1e-300)
    w0, w1 = float(d0.max()), float(d1.max())
    assert w0 <= 2e-5 and w1 <= 2e-5, (what, w0, w1)
    return max(w0, w1) / 2e-5


# ------------------------------------------------------------------ one test per table entry
@pytest.mark.parametrize("key", KEYS)
def test_table_entry_full_size(key):
    from scrubvae_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    kind, base, cv = parse_key(key)
    assert cv.tile_key(kind) == key
    d = cv.desc
    B, l_in, l_out, k, s, p, tr = cv.batch, cv.l_in, cv.l_out, cv.kernel, d.stride, d.padding, bool(d.transposed)
    ci, co, ldi, ldo = cv.c_in_p, cv.c_out_p, d.ld_in, d.ld_out
    cir, cor = ci - PAD, co - PAD  # real channels; the last PAD of each width are zero padding
    log_before = dict(ops.TUNED_LOG)

    def no_tuning():
        raise AssertionError(f"{key}: not taken from the tile table (the tuner would time candidates)")

    cv._tune(kind, no_tuning)  # the table path: the benchmark's choice
    assert ops.TUNED_LOG == log_before
    v = int(ops.TILE_TABLE[key])
    assert d.tile[ops._KIND_ID[kind]] == v % ops.Conv._F32_FLAG
    pieces = 0 if v >= ops.Conv._F32_FLAG else base
    assert cv._kind_pieces(kind) == pieces
    name = cv.kernel_name(kind)
    fam = f"{kind}: {_family(name)}" + (f" @{pieces}" if pieces else " fp32")
    ops.bump_weight_epoch()

    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(key.encode()))
    w = torch.randn(k, ci, co, generator=g, device="cuda") / math.sqrt(cir * k)
    w[:, cir:] = 0
    w[:, :, cor:] = 0
    w64 = w.double()
    tol = _SPLIT_TOL[pieces] if pieces else 2e-6
    out = {}
    if kind == "fwd":
        lx = l_in // 2 if cv.up2 else l_in
        xb = torch.randn(B * lx, ldi, generator=g, device="cuda")
        xb[:, cir:ci] = 0
        bias = torch.randn(co, generator=g, device="cuda")
        bias[cor:] = 0
        x64 = xb.view(B, lx, ldi)[:, :, :ci].double()
        if cv.up2:
            x64 = ref_up2(x64)
        y_ref = ref_fwd(x64, w64, bias.double(), l_out, s, p, 1, tr).view(B * l_out, co)
        del x64
        bound = tol * math.sqrt(cir * k) + tol
        rows = B * l_out
        buf, y = guarded(rows, ldo)
        if ldo > co:
            y[:, co:] = SENTINEL  # another tensor's columns
        cv.fwd(xb, w, bias, buf)
        check_guards(buf, rows * ldo, "fwd y", ldo, co)
        out["err"] = err_bound(y[:, :co], y_ref, bound, "fwd")
        assert float(y[:, cor:co].abs().max()) == 0.0, "pad channels of y not zero"
        out["block"] = row_block_ratio(y[:, :co], y_ref)
        if cv.up2:  # the upsampled operand rows, left behind for the weight gradient
            bufu, upo = guarded(B * l_in, ci)
            buf2, y2 = guarded(rows, ldo)
            cv.fwd(xb, w, bias, buf2, up_out=bufu)
            check_guards(bufu, B * l_in * ci, "fwd up_out")
            err_bound(upo, ref_up2(xb.view(B, lx, ldi)[:, :, :ci].double()).reshape(B * l_in, ci), 1e-6, "fwd up_out")
            assert torch.equal(y2[:, :co], y[:, :co])
            del bufu, upo, buf2, y2
        nt = cv.stats_tiles()
        if nt > 0:
            bufp, part = guarded(nt * 2, co)
            buf2, y2 = guarded(rows, ldo)
            if ldo > co:
                y2[:, co:] = SENTINEL
            cv.fwd(xb, w, bias, buf2, stats=bufp)
            check_guards(buf2, rows * ldo, "fwd(stats) y", ldo, co)
            check_guards(bufp, nt * 2 * co, "fwd stats partials")
            out["err"] = max(out["err"], err_bound(y2[:, :co], y_ref, bound, "fwd(stats)"))
            out["stats"] = _stats_check(part.view(nt, 2, co), nt, y2[:, :co], "fwd stats")
            del buf2, y2
            part.fill_(float("nan"))
        cv.fwd(xb, w, bias, buf, accumulate=True, stats=bufp if nt > 0 else None)
        check_guards(buf, rows * ldo, "fwd(accumulate) y", ldo, co)
        out["err"] = max(out["err"], err_bound(y[:, :co], 2 * y_ref, bound, "fwd(accumulate)"))
        if nt > 0:
            check_guards(bufp, nt * 2 * co, "fwd(accumulate) stats partials")
            out["stats"] = max(out["stats"], _stats_check(part.view(nt, 2, co), nt, y[:, :co], "fwd(accumulate) stats"))
    elif kind == "dgrad":
        dyb = torch.randn(B * l_out, ldo, generator=g, device="cuda")  # columns past co: another tensor's (must not be read)
        dyb[:, cor:co] = 0
        dx_ref = ref_dgrad(dyb.view(B, l_out, ldo)[:, :, :co].double(), w64, l_in, s, p, 1, tr).view(B * l_in, ci)
        bound = tol * math.sqrt(cor * k) + tol
        rows = B * l_in
        buf, dx = guarded(rows, ldi)
        cv.dgrad(dyb, w, buf)
        check_guards(buf, rows * ldi, "dgrad dx", ldi, ci)
        out["err"] = err_bound(dx[:, :ci], dx_ref, bound, "dgrad")
        assert float(dx[:, cir:ci].abs().max()) == 0.0, "pad channels of dx not zero"
        out["block"] = row_block_ratio(dx[:, :ci], dx_ref)
        if cv.dgrad_stats_tiles()[0] > 0:
            acc, eb, eg, ea = bn_bwd_fused_check(ops, cv, dyb, w, dx_ref, bound, "bn_prelu", seed=zlib.crc32(key.encode()) + 1)
            _, eb2, eg2, ea2 = bn_bwd_fused_check(ops, cv, dyb, w, dx_ref, bound, "bn_prelu", accumulate_onto=acc,
                                                  seed=zlib.crc32(key.encode()) + 1)
            out["dbeta"], out["dgamma"], out["dalpha"] = max(eb, eb2), max(eg, eg2), max(ea, ea2)
        cv.dgrad(dyb, w, buf, accumulate=True)
        check_guards(buf, rows * ldi, "dgrad(accumulate) dx", ldi, ci)
        out["err"] = max(out["err"], err_bound(dx[:, :ci], 2 * dx_ref, bound, "dgrad(accumulate)"))
    else:
        xb = torch.randn(B * l_in, ldi, generator=g, device="cuda")
        xb[:, cir:ci] = 0
        dyb = torch.randn(B * l_out, ldo, generator=g, device="cuda")
        dyb[:, cor:co] = 0
        dw_ref, db_ref = ref_wgrad(xb.view(B, l_in, ldi)[:, :, :ci].double(), dyb.view(B, l_out, ldo)[:, :, :co].double(), k, s, p, 1, tr)
        bound = tol * math.sqrt(B * l_out) + tol
        nws = cv.wgrad_workspace_bytes() // 4 + 1
        bufw = torch.full((nws + 4096,), SENTINEL, device="cuda")
        ws = bufw[:nws]  # the size the library asked for; the rest is a guard
        bufd, dw = guarded(k * ci, co)
        bufb, db = guarded(1, co)
        cv.wgrad(xb, dyb, bufd, bufb, ws)
        check_guards(bufd, k * ci * co, "wgrad dw")
        check_guards(bufb, co, "wgrad db")
        check_guards(bufw, nws, "wgrad workspace")
        dw3 = dw.view(k, ci, co)
        out["err"] = err_bound(dw3, dw_ref, bound, "wgrad dw")
        out["err_db"] = err_bound(db[0], db_ref, bound, "wgrad db")
        assert float(dw3[:, cir:].abs().max()) == 0.0 and float(dw3[:, :, cor:].abs().max()) == 0.0, "pad entries of dw not zero"
        assert float(db[0, cor:].abs().max()) == 0.0, "pad entries of db not zero"
        out["block"] = w_block_ratio(dw3, dw_ref)
        cv.wgrad(xb, dyb, bufd, bufb, ws, accumulate=True)
        check_guards(bufd, k * ci * co, "wgrad(accumulate) dw")
        check_guards(bufw, nws, "wgrad(accumulate) workspace")
        out["err"] = max(out["err"], err_bound(dw3, 2 * dw_ref, bound, "wgrad(accumulate) dw"))
        out["err_db"] = max(out["err_db"], err_bound(db[0], 2 * db_ref, bound, "wgrad(accumulate) db"))
    torch.cuda.synchronize()
    assert ops.TUNED_LOG == log_before
    print(f"\n{key} -> {name}: " + ", ".join(f"{k_} {v_:.3g}" for k_, v_ in out.items()))
    _note(fam, **out)
    assert out["block"] <= BLOCK_RATIO, (key, name, "worst / median block rms error", out["block"])
