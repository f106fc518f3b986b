"""Full-Cholesky heads, total correlation and the device-step optimizer (csrc/latent.hip, csrc/elementwise.hip) kernel by kernel
against the fp64 restatements of tests/latent_checks.py.

Inputs are drawn in fp64 and rounded to fp32 once; truth, yardstick and kernel see the rounded values.  Buffers have the leading
dimensions model/residual.py gives them (h: pad16(z) + pad16(z(z+1)/2), mu / sigma: pad16(z), z: pad16(z + conditional_dim)) with
the padding columns holding a sentinel that must survive.  Every compared quantity has to meet

    |kernel - fp64|_inf / |fp64|_inf  <=  max(8 e32, 8 2^-24),   e32 = |fp32 restatement on the CPU - fp64|_inf / |fp64|_inf

(latent_checks.gate; the reasoning for the factor is at latent_checks.FACTOR).  Where the truth vanishes identically (B = 1: loss_j
and both TC gradients) the denominator is the size of the terms that cancel (|lse_a|, the weight w).  Each gate prints its figures
(run with -s to see how much of the factor 8 a kernel uses)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import latent_checks as LC
from tests.latent_checks import SENTINEL, gate, ntri, pad16

pytestmark = pytest.mark.gpu

COND = 3  # conditional_dim: the z buffer carries a non-zero tail behind the latent columns
W_TC = 0.7


@pytest.fixture(scope="module")
def ops():
    from scrubvae_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def padded(t, ld, off=0):
    """[B, n] values -> [B, ld] float32 device buffer, columns off .. off + n, the rest holding the sentinel"""
    out = torch.full((t.shape[0], ld), SENTINEL, dtype=torch.float32)
    out[:, off:off + t.shape[1]] = t.float()
    return out.cuda()


def sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def only_sentinel(t):
    return t.numel() == 0 or bool((t == SENTINEL).all())


def finite(d):
    return all(bool(torch.isfinite(v).all()) for v in d.values() if isinstance(v, torch.Tensor))


# ------------------------------------------------------------------------------------------------ full-Cholesky heads
def heads_fwd(ops, d, B, z, with_eps=True):
    zp, hw, zcp = d["zp"], d["hw"], pad16(z + COND)
    buf = dict(h=d["h"].float().cuda(), eps=d["eps"].float().cuda() if with_eps else None, mu=sentinel(B, zp), L=sentinel(B, z, z),
               zc=sentinel(B, zcp), klp=sentinel(ops.heads_blocks(B, z)), zcp=zcp)
    ops.heads_tril_fwd(buf["h"], hw, buf["eps"], buf["mu"], zp, buf["L"], buf["zc"], zcp, buf["klp"], B, z, d["raw_off"])
    torch.cuda.synchronize()
    return buf


def check_heads_fwd(ops, d, B, z, tag):
    for with_eps in (True, False):
        t64, t32 = (LC.heads_truth(d, z, dt, 0.5, (), with_eps) for dt in (torch.float64, torch.float32))
        assert finite(t64)
        b = heads_fwd(ops, d, B, z, with_eps)
        name = f"heads_fwd {tag} eps={with_eps}"
        assert torch.equal(b["mu"][:, :z].cpu().double(), t64["mu"])  # a copy
        gate(name + " L", b["L"], t64["L"], t32["L"])
        assert float(torch.triu(b["L"], 1).abs().max()) == 0.0  # the sentinel above the diagonal is overwritten by exact zeros
        gate(name + " z", b["zc"][:, :z], t64["z"], t32["z"])
        if not with_eps:
            assert torch.equal(b["zc"][:, :z], b["mu"][:, :z])  # eval: z == mu
        gate(name + " kl", b["klp"].double().sum(), t64["kl"], t32["kl"])
        assert only_sentinel(b["mu"][:, z:]) and only_sentinel(b["zc"][:, z:])
        assert torch.equal(b["h"].cpu().double(), d["h"])


def check_heads_bwd(ops, d, B, z, tag):
    zp, hw, ro = d["zp"], d["hw"], d["raw_off"]
    for use, with_eps in ((("dz", "dmu", "dlv"), True), ((), True), (("dlv",), True), (("dz", "dmu", "dlv"), False), (("dz",), True)):
        kl_scale = 0.5
        t64, t32 = (LC.heads_truth(d, z, dt, kl_scale, use, with_eps) for dt in (torch.float64, torch.float32))
        assert finite(t64)
        b = heads_fwd(ops, d, B, z, with_eps)
        dz = padded(d["dz"], b["zcp"]) if "dz" in use else None
        dmu = padded(d["dmu"], zp) if "dmu" in use else None
        dlv = d["dlv"].float().cuda() if "dlv" in use else None
        dh = sentinel(B, hw)
        ops.heads_tril_bwd(b["h"], hw, b["eps"], b["L"], dz, b["zcp"], dmu, zp, kl_scale, dlv, dh, B, z, ro)
        torch.cuda.synchronize()
        cols = torch.cat([torch.arange(z), torch.arange(ro, ro + ntri(z))])
        gate(f"heads_bwd {tag} use={'+'.join(use) or 'kl'} eps={with_eps} dh", dh.cpu()[:, cols], t64["dh"][:, cols], t32["dh"][:, cols])
        rest = torch.ones(hw, dtype=torch.bool)
        rest[cols] = False
        assert only_sentinel(dh.cpu()[:, rest])


@pytest.mark.parametrize("B,z", LC.HEADS_SHAPES)
def test_heads_tril_fwd(ops, B, z):
    check_heads_fwd(ops, LC.heads_inputs(B, z), B, z, f"({B},{z})")


@pytest.mark.parametrize("B,z", LC.HEADS_SHAPES)
def test_heads_tril_bwd(ops, B, z):
    check_heads_bwd(ops, LC.heads_inputs(B, z), B, z, f"({B},{z})")


def test_heads_tril_range(ops):
    """raw diagonal entries on both sides of softplus's threshold and down to d = softplus(-30) ~ 1e-13"""
    B, z = LC.RANGE_SHAPE
    d = LC.range_inputs()
    check_heads_fwd(ops, d, B, z, "range")
    check_heads_bwd(ops, d, B, z, "range")


# ------------------------------------------------------------------------------------------------ total correlation
def check_tc(ops, d, B, z, full, tag):
    t64, t32 = (LC.tc_truth(d, W_TC, dt) for dt in (torch.float64, torch.float32))
    assert finite(t64) and finite(t32)
    zp, zcp = pad16(z), pad16(z + COND)
    mu, zc = padded(d["mu"], zp), padded(d["z"], zcp)
    sig = None if full else padded(d["sigma"], zp)
    L = d["L"].float().cuda().contiguous() if full else None
    lv, lse_l, lse_a, loss = sentinel(B, z), sentinel(B, z), sentinel(B), sentinel(B)
    ops.tc_logvar(sig, zp, L, lv, B, z)
    ops.tc_fwd(zc, zcp, mu, zp, lv, B, z, lse_l, lse_a, loss)
    torch.cuda.synchronize()
    gate(f"tc_logvar {tag} lv", lv, t64["lv"], t32["lv"])
    gate(f"tc_fwd {tag} lse_l", lse_l, t64["lse_l"], t32["lse_l"])
    gate(f"tc_fwd {tag} lse_a", lse_a, t64["lse_a"], t32["lse_a"])
    cancel = float(t64["lse_a"].abs().max()) if B == 1 else None  # B = 1: loss_j is lse_a - sum_l lse_l = 0
    gate(f"tc_fwd {tag} loss", loss, t64["loss"], t32["loss"], cancel)

    # backward: d_mu accumulates into what is there, the second output is overwritten
    zero = B == 1  # both gradients vanish identically
    g0 = LC.r32(torch.randn(B, z, generator=torch.Generator().manual_seed(B * 131 + z), dtype=torch.float64)
                * (W_TC if zero else float(t64["dmu"].abs().max())))
    d_mu = padded(g0, zp)
    if full:
        d2, ldv, key = sentinel(B, z), z, "dlv"
    else:
        d2, ldv, key = sentinel(B, zp), zp, "dsigma"
    ops.tc_bwd(zc, zcp, mu, zp, lv, B, z, lse_l, lse_a, W_TC, d_mu, zp, d2, ldv, sig, zp if sig is not None else 0)
    torch.cuda.synchronize()
    gate(f"tc_bwd {tag} g0+dmu", d_mu[:, :z], g0 + t64["dmu"], g0.float() + t32["dmu"], W_TC if zero else None)
    gate(f"tc_bwd {tag} {key}", d2[:, :z], t64[key], t32[key], W_TC if zero else None)
    assert only_sentinel(d_mu[:, z:]) and only_sentinel(d2[:, z:]) and only_sentinel(mu[:, z:]) and only_sentinel(zc[:, z:])


@pytest.mark.parametrize("full", [False, True], ids=["diag", "fullL"])
@pytest.mark.parametrize("B,z", LC.TC_SHAPES)
def test_tc_fwd_bwd(ops, B, z, full):
    check_tc(ops, LC.tc_inputs(B, z, full), B, z, full, f"({B},{z}) {'fullL' if full else 'diag'}")


@pytest.mark.parametrize("full", [False, True], ids=["diag", "fullL"])
@pytest.mark.parametrize("B,z", LC.SPREAD_SHAPES)
def test_tc_spread_out(ops, B, z, full):
    """mu scaled by 6, sigma by 0.2: most exp(q - max) terms underflow, the softmax weights are nearly one-hot"""
    check_tc(ops, LC.tc_inputs(B, z, full, spread=True), B, z, full, f"spread ({B},{z}) {'fullL' if full else 'diag'}")


@pytest.mark.parametrize("B,z", [(64, 32), (257, 33)])
def test_tc_bwd_into_heads_tril_bwd(ops, B, z):
    """train/losses.py's full-L path: tc_bwd -> dlv -> heads_tril_bwd, against autograd through lv = log diag(L L^T) down to h"""
    d = LC.heads_inputs(B, z)
    zp, hw, ro = d["zp"], d["hw"], d["raw_off"]
    t64, t32 = (LC.compose_truth(d, z, dt, W_TC) for dt in (torch.float64, torch.float32))
    assert bool(torch.isfinite(t64).all())
    b = heads_fwd(ops, d, B, z)
    lv, lse_l, lse_a, loss, dlv = sentinel(B, z), sentinel(B, z), sentinel(B), sentinel(B), sentinel(B, z)
    ops.tc_logvar(None, zp, b["L"], lv, B, z)
    ops.tc_fwd(b["zc"], b["zcp"], b["mu"], zp, lv, B, z, lse_l, lse_a, loss)
    d_mu = padded(torch.zeros(B, z), zp)
    ops.tc_bwd(b["zc"], b["zcp"], b["mu"], zp, lv, B, z, lse_l, lse_a, W_TC, d_mu, zp, dlv, z)
    dh = sentinel(B, hw)
    ops.heads_tril_bwd(b["h"], hw, b["eps"], b["L"], None, b["zcp"], d_mu, zp, 0.0, dlv, dh, B, z, ro)
    torch.cuda.synchronize()
    cols = torch.cat([torch.arange(z), torch.arange(ro, ro + ntri(z))])
    gate(f"tc->heads ({B},{z}) dh", dh.cpu()[:, cols], t64[:, cols], t32[:, cols])


def test_tc_rejects_z_dim_129(ops):
    """the argument check returns before any launch: nothing is written"""
    B, z = 4, 129
    zp, zcp = pad16(z), pad16(z + COND)
    mu, zc, sig, lv = (torch.ones(B, n, device="cuda") for n in (zp, zcp, zp, z))
    lse_l, lse_a, loss, d_mu, d2 = sentinel(B, z), sentinel(B), sentinel(B), sentinel(B, zp), sentinel(B, zp)
    with pytest.raises(RuntimeError, match="z_dim must be <= 128"):
        ops.tc_fwd(zc, zcp, mu, zp, lv, B, z, lse_l, lse_a, loss)
    with pytest.raises(RuntimeError, match="z_dim must be <= 128"):
        ops.tc_bwd(zc, zcp, mu, zp, lv, B, z, lse_l, lse_a, W_TC, d_mu, zp, d2, zp, sig, zp)
    torch.cuda.synchronize()
    assert all(only_sentinel(t) for t in (lse_l, lse_a, loss, d_mu, d2))


# ------------------------------------------------------------------------------------------------ device-step optimizer
def ulps32(got, want):
    want32 = np.float32(want)
    return abs(float(got) - float(want32)) / float(np.spacing(want32))


@pytest.mark.parametrize("n", LC.OPT_SIZES)
@pytest.mark.parametrize("name,decoupled,wd,gs", LC.OPT_CONFIGS)
def test_adam_advance_and_step_dev(ops, n, name, decoupled, wd, gs):
    """eight adam_advance + adam_step_dev from hyper = {lr, 0, 0, 0} against the fp64 optimizer (checked against torch.optim in
    test_latent_cpu.py); the yardstick is torch.optim in fp32 on the CPU.  The hyper-parameters are the fp32 values the C ABI
    receives (0.999 as a float is 0.99900001..: 1 - beta2 differs by 1.3e-5 relative from 0.001, which is a different beta2, not
    an error of the arithmetic)."""
    steps = 8
    lr, b1, b2, eps, wd = LC.adam_hyper(LC.LR, LC.BETA1, LC.BETA2, LC.ADAM_EPS, wd)
    p0, grads = LC.opt_inputs(n, steps)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t, g in enumerate(grads, 1):
        p64, m64, v64 = LC.adam_ref(p64, m64, v64, g.double(), t, lr, b1, b2, eps, wd, decoupled, gs)
    p32, m32, v32 = LC.torch_optim_run(p0, grads, torch.float32, lr, b1, b2, eps, wd, decoupled, gs)
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    hyper = torch.tensor([lr, 0.0, 0.0, 0.0], device="cuda")
    for g in grads:
        ops.adam_advance(hyper, b1, b2)
        ops.adam_step_dev(p, g.cuda(), m, v, hyper, b1, b2, eps, wd, decoupled, gs)
    torch.cuda.synchronize()
    hy = hyper.cpu()
    assert float(hy[0]) == lr and float(hy[3]) == steps
    u1, u2 = ulps32(hy[1], lr / (1 - b1 ** steps)), ulps32(hy[2], 1 / math.sqrt(1 - b2 ** steps))
    print(f"GATE adam {name} n={n} hyper ulps {u1:.1f} {u2:.1f}")
    assert u1 <= 2 and u2 <= 2
    for key, got, a, b in (("p", p, p64, p32), ("m", m, m64, m32), ("v", v, v64, v32)):
        gate(f"adam {name} n={n} {key}", got, a, b)


@pytest.mark.parametrize("n", [4160, 2_097_152 + 4])
@pytest.mark.parametrize("name,decoupled,wd,gs", LC.OPT_CONFIGS)
def test_adam_step_and_step_dev_bit_identical(ops, n, name, decoupled, wd, gs):
    """the host-scalar and the device-hyper kernel call one compiled body (adam_span): same step, same scalars -> same bits (as two
    copies of the same source lines they did not: the compiler fused different multiply-adds in each, and an eager and a captured
    step differed in the last bit of p and v)"""
    t = 3
    lr, b1, b2, eps, wd = LC.adam_hyper(LC.LR, LC.BETA1, LC.BETA2, LC.ADAM_EPS, wd)
    p0, (g, m0, v0) = LC.opt_inputs(n, 3, seed=1)
    m0, v0 = 0.1 * m0, 0.01 * v0 * v0
    a = [x.clone().cuda() for x in (p0, m0, v0)]
    b = [x.clone().cuda() for x in (p0, m0, v0)]
    ops.adam_step(a[0], g.cuda(), a[1], a[2], lr, b1, b2, eps, wd, t, decoupled, gs)
    hyper = torch.tensor(list(LC.host_scalars(lr, b1, b2, t)) + [float(t)], device="cuda")
    ops.adam_step_dev(b[0], g.cuda(), b[1], b[2], hyper, b1, b2, eps, wd, decoupled, gs)
    torch.cuda.synchronize()
    assert not torch.equal(a[0].cpu(), p0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n", LC.OPT_SIZES)
def test_clip_grads_and_sumsq(ops, n):
    """torch.nn.utils.clip_grad_norm_: g *= min(1, max_norm / (norm + 1e-6)); the squared norm comes from sumsq_partial + reduce_rows"""
    _, (g,) = LC.opt_inputs(n, 1, seed=2)
    g64 = g.double()
    ss64, ss32 = (g64 * g64).sum(), (g * g).sum()
    norm64, norm32 = ss64.sqrt(), torch.linalg.vector_norm(g)
    part = sentinel(ops.sumsq_blocks(n))
    ss = sentinel(1)
    ops.sumsq_partial(g.cuda(), part)
    ops.reduce_rows(part, part.numel(), 1, 1.0, ss)
    gate(f"clip n={n} sumsq", ss, ss64.reshape(1), ss32.reshape(1))
    # the clip bites
    max_norm = LC.f32(0.5 * float(norm64))
    gd, norm_out = g.clone().cuda(), sentinel(1)
    ops.clip_grads(gd, ss, max_norm, norm_out)
    torch.cuda.synchronize()
    gate(f"clip n={n} norm_out", norm_out, norm64.reshape(1), norm32.reshape(1))
    gate(f"clip n={n} g", gd, g64 * (max_norm / (norm64 + 1e-6)), g * (torch.tensor(max_norm) / (norm32 + torch.tensor(1e-6))))
    # it does not: the gradients keep their bits, the norm is still reported
    gd2, norm_out2 = g.clone().cuda(), sentinel(1)
    ops.clip_grads(gd2, ss, LC.f32(2.0 * float(norm64)), norm_out2)
    ops.clip_grads(gd2, ss, LC.f32(2.0 * float(norm64)), None)
    torch.cuda.synchronize()
    assert torch.equal(gd2.cpu(), g) and torch.equal(norm_out2, norm_out)


def test_reduce_rows_scaled(ops):
    rows, k = 700, 5
    part = LC.r32(torch.randn(rows, k, generator=torch.Generator().manual_seed(3), dtype=torch.float64) + 2.0)
    scales = [LC.f32(s) for s in (1.0 / rows, 0.25, 3.0, 1.0 / (rows * 54), 1e-3)]
    out = sentinel(8)
    ops.reduce_rows_scaled(part.float().cuda(), rows, scales, out)
    s64 = torch.tensor(scales, dtype=torch.float64)
    gate("reduce_rows_scaled", out[:k], part.sum(0) * s64, part.float().sum(0) * s64.float())
    assert only_sentinel(out[k:])


def test_loss_total(ops):
    """the reported total: sum_i w_i term_i in index order, terms with weight 0 left out (their slots may hold anything)"""
    terms = LC.r32(torch.rand(7, generator=torch.Generator().manual_seed(4), dtype=torch.float64) * 10 + 0.1)
    weights = [LC.f32(w) for w in (1.0, 0.5, 0.0, 0.1, 0.7, 0.0, 3.0)]
    dev = terms.float().cuda()
    dev[2] = float("nan")
    out = sentinel(2)
    ops.loss_total(dev, weights, out[:1])
    w64 = torch.tensor(weights, dtype=torch.float64)
    t32 = torch.zeros((), dtype=torch.float32)
    for w, t in zip(weights, terms.float()):
        t32 = t32 + torch.tensor(w, dtype=torch.float32) * t
    gate("loss_total", out[:1], (w64 * terms).sum().reshape(1), t32.reshape(1))
    assert only_sentinel(out[1:])


# ------------------------------------------------------------------------------------------------ the remaining uncalled wrappers
def test_relu_axpy_fill(ops):
    n = 4096 * 256 + 13  # past one trip of the capped grid, ragged
    x = torch.randn(n, generator=torch.Generator().manual_seed(5))
    xd, y = x.cuda(), sentinel(n + 3)
    ops.relu_fwd(xd, y[:n])
    assert torch.equal(y[:n].cpu(), x.clamp(min=0)) and only_sentinel(y[n:])
    dy, dx = torch.randn(n, generator=torch.Generator().manual_seed(6)), sentinel(n + 3)
    ops.relu_bwd(dy.cuda(), y[:n], dx[:n])
    assert torch.equal(dx[:n].cpu(), torch.where(x > 0, dy, torch.zeros(()))) and only_sentinel(dx[n:])
    acc = dy.clone().cuda()
    ops.axpy(0.375, xd, acc)
    gate("axpy", acc, dy.double() + 0.375 * x.double(), dy + 0.375 * x)
    ops.fill(y[:n], -2.5)
    assert bool((y[:n] == -2.5).all()) and only_sentinel(y[n:])


@pytest.mark.parametrize("rows,Cc", [(700, 48), (70000, 256)])
def test_bn_stats_finalize_and_eval_coeffs(ops, rows, Cc):
    """the single-launch reduce + finalize of the training pass and the eval-mode coefficients against fp64 BatchNorm statistics"""
    g = torch.Generator().manual_seed(rows)
    x = LC.r32(torch.randn(rows, Cc, generator=g, dtype=torch.float64) * 2 + 0.7)
    gamma, beta = LC.r32(1 + 0.1 * torch.randn(Cc, generator=g, dtype=torch.float64)), LC.r32(0.1 * torch.randn(Cc, generator=g, dtype=torch.float64))
    eps, mom = LC.f32(1e-4), LC.f32(0.1)
    rm0, rv0 = LC.r32(0.3 * torch.randn(Cc, generator=g, dtype=torch.float64)), LC.r32(1 + torch.rand(Cc, generator=g, dtype=torch.float64))

    def truth(dt):
        xx, rm, rv = x.to(dt), rm0.to(dt).clone(), rv0.to(dt).clone()
        F.batch_norm(xx, rm, rv, gamma.to(dt), beta.to(dt), True, mom, eps)
        mean, rstd = xx.mean(0), 1 / torch.sqrt(xx.var(0, unbiased=False) + eps)
        sc = gamma.to(dt) * rstd
        esc = gamma.to(dt) / torch.sqrt(rv + eps)
        return dict(mean=mean, rstd=rstd, scale=sc, shift=beta.to(dt) - mean * sc, rm=rm, rv=rv, escale=esc, eshift=beta.to(dt) - rm * esc)

    t64, t32 = truth(torch.float64), truth(torch.float32)
    dev = lambda t: t.float().cuda().contiguous()
    nch = ops.bn_chunks(rows)
    part = sentinel(nch, 2, Cc)
    ops.bn_stats_partial(dev(x), rows, Cc, Cc, part)
    rm, rv, nbt = dev(rm0), dev(rv0), torch.full((1,), 41, dtype=torch.int64, device="cuda")
    o = {k: sentinel(Cc) for k in ("mean", "rstd", "scale", "shift", "escale", "eshift")}
    ops.bn_stats_finalize(part, nch, rows, Cc, dev(gamma), dev(beta), eps, mom, rm, rv, nbt, o["mean"], o["rstd"], o["scale"], o["shift"])
    ops.bn_eval_coeffs(Cc, dev(gamma), dev(beta), eps, rm, rv, o["escale"], o["eshift"])
    torch.cuda.synchronize()
    assert int(nbt) == 42
    o.update(rm=rm, rv=rv)
    for k, got in o.items():
        gate(f"bn ({rows},{Cc}) {k}", got, t64[k], t32[k])
