"""Shared checks of the conv kernel tests (test_gpu_kernels, test_gpu_tile_table): a float64 reference of the conv passes that runs on
the device, guarded output buffers, error / block-ratio measures and the check of the data-gradient's fused BatchNorm + activation
backward epilogue."""
import math

import torch
import torch.nn.functional as F

GUARD_ROWS = 256  # one full row tile past the end of every output
SENTINEL = 777.0


# ------------------------------------------------------------------ fp64 reference on the device
def _taps(n_a, n_b, s, p, d, t):
    """Rows a in [0, n_a) whose partner b = a * s + t * d - p lies in [0, n_b): (a0, a1, b0) with a in [a0, a1), b = b0 + (a - a0) * s."""
    off = t * d - p
    a0 = max(0, -(off // s))  # ceil(-off / s)
    a1 = min(n_a, (n_b - 1 - off) // s + 1) if n_b - 1 - off >= 0 else 0
    return a0, max(a0, a1), a0 * s + off


def ref_fwd(x, w, b, l_out, s, p, d, tr):
    """x [B, l_in, Cin], w [k, Cin, Cout], b [Cout] or None (all fp64) -> y [B, l_out, Cout] of nn.Conv1d / nn.ConvTranspose1d."""
    B, l_in, _ = x.shape
    y = torch.zeros(B, l_out, w.shape[2], dtype=x.dtype, device=x.device)
    for t in range(w.shape[0]):
        if tr:  # a = input row, b = output row
            a0, a1, b0 = _taps(l_in, l_out, s, p, d, t)
            if a1 > a0:
                y[:, b0: b0 + (a1 - a0 - 1) * s + 1: s] += torch.matmul(x[:, a0:a1], w[t])
        else:  # a = output row, b = input row
            a0, a1, b0 = _taps(l_out, l_in, s, p, d, t)
            if a1 > a0:
                y[:, a0:a1] += torch.matmul(x[:, b0: b0 + (a1 - a0 - 1) * s + 1: s], w[t])
    if b is not None:
        y += b
    return y


def ref_dgrad(dy, w, l_in, s, p, d, tr):
    """dy [B, l_out, Cout] -> dx [B, l_in, Cin]: the adjoint of ref_fwd in its input."""
    B, l_out, _ = dy.shape
    dx = torch.zeros(B, l_in, w.shape[1], dtype=dy.dtype, device=dy.device)
    for t in range(w.shape[0]):
        wt = w[t].t()
        if tr:
            a0, a1, b0 = _taps(l_in, l_out, s, p, d, t)
            if a1 > a0:
                dx[:, a0:a1] += torch.matmul(dy[:, b0: b0 + (a1 - a0 - 1) * s + 1: s], wt)
        else:
            a0, a1, b0 = _taps(l_out, l_in, s, p, d, t)
            if a1 > a0:
                dx[:, b0: b0 + (a1 - a0 - 1) * s + 1: s] += torch.matmul(dy[:, a0:a1], wt)
    return dx


def ref_wgrad(x, dy, k, s, p, d, tr):
    """x [B, l_in, Cin], dy [B, l_out, Cout] -> (dw [k, Cin, Cout], db [Cout]): the adjoint of ref_fwd in its weights and bias."""
    B, l_in, ci = x.shape
    l_out, co = dy.shape[1], dy.shape[2]
    dw = torch.zeros(k, ci, co, dtype=x.dtype, device=x.device)
    for t in range(k):
        if tr:
            a0, a1, b0 = _taps(l_in, l_out, s, p, d, t)
            xa, da = x[:, a0:a1], dy[:, b0: b0 + (a1 - a0 - 1) * s + 1: s]
        else:
            a0, a1, b0 = _taps(l_out, l_in, s, p, d, t)
            xa, da = x[:, b0: b0 + (a1 - a0 - 1) * s + 1: s], dy[:, a0:a1]
        if a1 > a0:
            dw[t] = xa.reshape(-1, ci).t() @ da.reshape(-1, co)
    return dw, dy.sum((0, 1))


def ref_up2(x):
    """[B, L, C] -> [B, 2L, C]: nn.Upsample(scale_factor=2, mode="linear") (align_corners=False)."""
    return F.interpolate(x.transpose(1, 2), scale_factor=2, mode="linear", align_corners=False).transpose(1, 2)


# ------------------------------------------------------------------ helpers
def guarded(rows, ld, fill=float("nan")):
    """(buffer, view): a [rows, ld] fp32 view filled with `fill`, followed by GUARD_ROWS rows of SENTINEL."""
    buf = torch.full(((rows + GUARD_ROWS) * ld,), SENTINEL, device="cuda")
    v = buf[: rows * ld].view(rows, ld)
    v.fill_(fill)
    return buf, v


def check_guards(buf, n_valid, what, ld=None, width=None):
    """Everything past the first n_valid floats (and, with ld / width, the columns [width, ld) of the valid rows) still SENTINEL."""
    tail = buf[n_valid:]
    assert torch.equal(tail, torch.full_like(tail, SENTINEL)), f"{what}: written past the end"
    if ld is not None and width < ld:
        cols = buf[:n_valid].view(-1, ld)[:, width:]
        assert torch.equal(cols, torch.full_like(cols, SENTINEL)), f"{what}: written into the columns [{width}, {ld}) of another tensor"


def err_bound(out, ref, bound, what):
    """Max-norm relative error of out (fp32) against ref (fp64) within bound; returns the error as a fraction of the bound."""
    assert not torch.isnan(out).any(), f"{what}: elements left unwritten (NaN)"
    e = float((out.double() - ref).abs().max() / ref.abs().max())
    assert e < bound, (what, e, bound)
    return e / bound


def block_ratio(err2, counts):
    """err2: per-block sums of squared errors, counts: elements per block -> worst / median block rms."""
    rms = (err2 / counts).sqrt()
    med = float(rms.median())
    worst = float(rms.max())
    if worst == 0.0:
        return 0.0
    return worst / med if med > 0 else math.inf


def row_block_ratio(out, ref):
    """[rows, C] -> worst / median rms error over 256-row blocks (the last one ragged)."""
    e2 = (out.double() - ref).pow(2).sum(1)
    n = e2.shape[0]
    nb = (n + 255) // 256
    e2 = F.pad(e2, (0, nb * 256 - n)).view(nb, 256).sum(1)
    counts = torch.full((nb,), 256.0 * out.shape[1], dtype=torch.float64, device=out.device)
    counts[-1] = (n - (nb - 1) * 256) * out.shape[1]
    return block_ratio(e2, counts)


def w_block_ratio(out, ref):
    """[k, Cin, Cout] -> worst / median rms error over (tap, 128 x 128) blocks."""
    k, ci, co = out.shape
    e2 = (out.double() - ref).pow(2)
    bi, bo = (ci + 127) // 128, (co + 127) // 128
    e2 = F.pad(e2, (0, bo * 128 - co, 0, bi * 128 - ci)).view(k, bi, 128, bo, 128).sum((2, 4))
    ones = F.pad(torch.ones(ci, co, dtype=torch.float64, device=out.device), (0, bo * 128 - co, 0, bi * 128 - ci))
    counts = ones.view(bi, 128, bo, 128).sum((1, 3)).expand(k, bi, bo)
    return block_ratio(e2.reshape(-1), counts.reshape(-1))


# ------------------------------------------------------------------ the fused BatchNorm + activation backward of dgrad
def bn_bwd_fused_check(ops, cv, dy, w, dx_ref, bound, mode, accumulate_onto=None, seed=0):
    """Data-gradient launch with the fused first pass of a BatchNorm + activation backward (ResVAE._dgrad_into_bn / _bn_act_bwd):
    mode "bn_prelu" (scale / shift / mean / rstd / slope), "bare" (PReLU without BatchNorm: scale = NULL) or "bn_tanh" (alpha = NULL).
    dx_ref [rows, c_in_p] fp64: the data gradient; the written dx must match it (2x with accumulate).  The epilogue's sums are checked
    against fp64 autograd of act(gamma * xhat + beta) with the kernel's own written dx as upstream gradient.  Returns the worst
    (dbeta, dgamma, dalpha) errors as fractions of their gates."""
    from scrubvae_amd._lib import BnBwdFuse
    n, cb = cv.dgrad_stats_tiles()
    assert n > 0
    rows, Cp = cv.batch * cv.l_in, cv.c_in_p
    g = torch.Generator(device="cuda").manual_seed(seed)
    gamma = 1 + 0.2 * torch.randn(Cp, generator=g, device="cuda")
    beta = 0.3 * torch.randn(Cp, generator=g, device="cuda")
    mean = 0.5 * torch.randn(Cp, generator=g, device="cuda")
    rstd = 0.5 + torch.rand(Cp, generator=g, device="cuda")
    alpha = torch.tensor([0.25], device="cuda")
    bn = mode != "bare"
    scale = gamma * rstd if bn else torch.ones(Cp, device="cuda")
    shift = beta - mean * scale if bn else torch.zeros(Cp, device="cuda")
    # the saved input x: drawn through u = x * scale + shift so that no u lies within 1e-3 rms(u) of the PReLU's kink
    u = torch.randn(rows, Cp, generator=g, device="cuda", dtype=torch.float64)
    u = torch.where(u.abs() < 2e-3, torch.where(u < 0, -2e-3, 2e-3), u)
    x = ((u - shift.double()) / scale.double()).float().contiguous()
    u64 = x.double() * scale.double() + shift.double()
    assert float(u64.abs().min()) > 1e-3 * float(u64.pow(2).mean().sqrt())
    bufp, part = guarded(n * 2, Cp)
    bufa, dap = guarded(2 * n * cb, 1)
    f = BnBwdFuse()
    f.x, f.part = x.data_ptr(), bufp.data_ptr()
    if bn:
        f.scale, f.shift, f.mean, f.rstd = scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    f.alpha = alpha.data_ptr() if mode != "bn_tanh" else None
    f.dalpha_part = bufa.data_ptr() if mode != "bn_tanh" else None
    if accumulate_onto is None:
        bufx, dx = guarded(rows, cv.desc.ld_in)
        cv.dgrad(dy, w, bufx, fuse=f)
    else:
        bufx, dx = accumulate_onto
        cv.dgrad(dy, w, bufx, accumulate=True, fuse=f)
        dx_ref = 2 * dx_ref
    check_guards(bufx, rows * cv.desc.ld_in, "dgrad(fuse) dx")
    check_guards(bufp, n * 2 * Cp, "dgrad(fuse) BatchNorm partials")
    err_bound(dx[:, :Cp], dx_ref, bound, f"dgrad(fuse={mode}) dx")
    assert not torch.isnan(part).any(), "fused partials left unwritten"
    sums = torch.empty(2, Cp, device="cuda")
    dgam, dbet, dal = torch.zeros(Cp, device="cuda"), torch.zeros(Cp, device="cuda"), torch.zeros(1, device="cuda")
    if mode != "bn_tanh":
        check_guards(bufa, 2 * n * cb, "dgrad(fuse) slope partials")
        assert not torch.isnan(dap).any(), "slope partials left unwritten"
    ops.bn_bwd_reduce(bufp, n, Cp, sums, dgam, dbet, dal if mode != "bn_tanh" else None, bufa if mode != "bn_tanh" else None,
                      2 * n * cb if mode != "bn_tanh" else 0, False)
    # reference: fp64 autograd of act(gamma * xhat + beta) (bare: act(x)) with upstream gradient = the dx the launch wrote
    up = dx[:, :Cp].double()
    xd = x.double()
    if bn:
        xhat = (xd - mean.double()) * rstd.double()
        g64 = gamma.double().requires_grad_(True)
        b64 = beta.double().requires_grad_(True)
        uu = g64 * xhat + b64
    else:
        xhat = torch.zeros_like(xd)
        uu = xd.clone().requires_grad_(True)
    a64 = alpha.double().requires_grad_(True)
    act = torch.tanh(uu) if mode == "bn_tanh" else F.prelu(uu, a64)
    act.backward(up)
    du = torch.where(uu.detach() > 0, up, a64.detach() * up) if mode != "bn_tanh" else up * (1 - torch.tanh(uu.detach()) ** 2)
    ref_b = b64.grad if bn else du.sum(0)
    ref_g = g64.grad if bn else torch.zeros(Cp, dtype=torch.float64, device="cuda")
    eb = ((sums[0].double() - ref_b).abs() / (2e-5 * du.abs().sum(0)).clamp_min(1e-300)).max()
    eg = ((sums[1].double() - ref_g).abs() / (2e-5 * (du * xhat).abs().sum(0)).clamp_min(1e-300)).max() if bn else 0.0
    if not bn:
        assert float(sums[1].abs().max()) == 0.0  # no BatchNorm: no xhat sums
    assert torch.equal(dbet, sums[0]) and torch.equal(dgam, sums[1])  # the parameter gradients are the sums
    eb, eg = float(eb), float(eg)
    assert eb <= 1 and eg <= 1, (mode, "dbeta / dgamma", eb, eg)
    ea = 0.0
    if mode != "bn_tanh":
        gate = 1e-6 * float((up * u64 * (u64 <= 0)).abs().sum())
        ea = abs(float(dal) - float(a64.grad)) / gate
        assert ea <= 1, (mode, "dalpha", float(dal), float(a64.grad), gate)
    return (bufx, dx), eb, eg, ea
