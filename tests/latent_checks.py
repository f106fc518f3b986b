"""Plain-torch restatements of the latent-head, total-correlation and optimizer arithmetic, used by test_latent_cpu.py (against
oracle/scvae_oracle.py and torch.optim) and test_gpu_latent.py (against csrc/latent.hip and csrc/elementwise.hip).

Every function is dtype-generic: run on float64 tensors it is the truth, run on the same values as float32 tensors it is the
yardstick -- the error the reference's own fp32 arithmetic makes at these inputs.  `gate` turns the two into the bound a kernel
has to meet.  The input generators draw in fp64 and round to fp32 once, so the truth, the yardstick and the kernel all see the
same numbers."""
import math

import torch

from oracle import scvae_oracle as O

SENTINEL = 7.0
FLOOR = 8.0 * 2.0 ** -24  # keeps a lucky e32 ~ 0 (it is exactly 0 at B = 1) from demanding bit-equality
FACTOR = 8.0  # sequential 512-term merges against torch's pairwise sums, 1-2 ulp device expf / logf / log1pf

HEADS_SHAPES = [(1, 1), (5, 8), (37, 31), (64, 32), (257, 33), (129, 64), (4096, 32)]
TC_SHAPES = [(1, 1), (5, 8), (7, 32), (12, 8), (37, 31), (64, 32), (257, 33), (300, 64), (129, 100), (512, 128), (4096, 32)]
SPREAD_SHAPES = [(64, 32), (257, 33), (512, 128)]
RANGE_DIAG = (-30.0, -8.0, 0.0, 8.0, 19.9, 20.1, 60.0)  # both sides of softplus's threshold 20; tiny d: 1 / d and log d are large
RANGE_SHAPE = (7, 8)
OPT_SIZES = [4, 4160, 2_097_152 + 4, 8_388_608 + 1028]  # below, at and well past one trip of a 2048 x 256 x float4 grid
OPT_CONFIGS = [  # name, decoupled, weight decay, grad_scale
    ("adamw", True, 0.01, 1.0),
    ("adam_coupled", False, 0.01, 0.25),
    ("adam", False, 0.0, 1.0),
]
LR, BETA1, BETA2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8


def pad16(c):
    return (int(c) + 15) // 16 * 16


def ntri(z):
    return z * (z + 1) // 2


def r32(t):
    """round an fp64 tensor to fp32 once (the value every side sees), returned as fp64"""
    return t.float().double()


def f32(x):
    """a Python float rounded to fp32: the C ABI takes its scalars as `float`, so both sides use the rounded value"""
    return float(torch.tensor(x, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ the bound
def errs(got, t64, t32, denom=None):
    """(kernel error, e32, bound): max-norm errors of `got` and of the fp32 restatement against the fp64 truth, both relative to
    `denom` (default: the truth's max-norm), and the bound max(8 e32, 8 2^-24)"""
    t64 = torch.as_tensor(t64, dtype=torch.float64)
    d = float(t64.abs().max()) if denom is None else float(denom)
    assert d > 0 and math.isfinite(d), d
    e32 = float((torch.as_tensor(t32).double() - t64).abs().max()) / d
    err = float((torch.as_tensor(got).double().cpu() - t64).abs().max()) / d
    return err, e32, max(FACTOR * e32, FLOOR)


def gate(name, got, t64, t32, denom=None):
    """print the figures, then assert  |kernel - fp64| / |fp64|  <=  max(8 e32, 8 2^-24)"""
    err, e32, bound = errs(got, t64, t32, denom)
    print(f"GATE {name}: err {err:.3e} e32 {e32:.3e} bound {bound:.3e} err/e32 {err / max(e32, 2.0 ** -24):.2f}")
    assert math.isfinite(err) and err <= bound, (name, err, e32, bound)
    return err, e32


# ------------------------------------------------------------------------------------------------ full-Cholesky heads
def tril_heads(h, eps, z, raw_off):
    """h [B, >= raw_off + z(z+1)/2] = [mu | .. | raw (torch.tril_indices order)] -> mu, L, z = L eps + mu (eps None: z = mu) and the
    un-divided KL sum (prior_loss times B)"""
    mu = h[:, :z]
    L = O.cholesky_L(h[:, raw_off:raw_off + ntri(z)], z, False)
    zz = mu if eps is None else torch.matmul(L, eps[:, :, None])[:, :, 0] + mu
    return mu, L, zz, O.prior_loss(mu, L) * h.shape[0]


def logvar(L=None, sigma=None):
    """log of the posterior's marginal variances: log diag(L L^T), or 2 log sigma for the diagonal posterior"""
    if L is not None:
        return torch.log(torch.matmul(L, L.transpose(-2, -1)).diagonal(dim1=-1, dim2=-2))
    return 2 * torch.log(sigma)


def tc_rows(zz, mu, lv, block=128, parts=False):
    """per-sample loss_j of oracle.total_correlation (z detached; its mean is the loss), evaluated in blocks of `block` rows j so that
    no [B, B, z] tensor is needed.  parts: also logsumexp_i lq[j, i, l] [B, z] and logsumexp_i sum_l lq[j, i, l] [B]"""
    zz = zz.detach()
    loss, lse_l, lse_a = [], [], []
    for j0 in range(0, zz.shape[0], block):
        lq = -0.5 * (torch.exp(-lv)[None] * (zz[j0:j0 + block, None] - mu[None]) ** 2 + lv[None] + O.LN2PI)
        ll, la = torch.logsumexp(lq, dim=1), torch.logsumexp(lq.sum(dim=2), dim=1)
        loss.append(la - ll.sum(dim=1))
        lse_l.append(ll)
        lse_a.append(la)
    if parts:
        return torch.cat(loss), torch.cat(lse_l), torch.cat(lse_a)
    return torch.cat(loss)


def tc_grads(zz, mu, lv, w, block=128):
    """d (w sum_j loss_j) / d mu and / d lv by autograd, one block of rows at a time (the graph of a block is freed before the next)"""
    mu, lv = mu.detach().clone().requires_grad_(True), lv.detach().clone().requires_grad_(True)
    for j0 in range(0, zz.shape[0], block):
        (w * tc_rows(zz[j0:j0 + block], mu, lv, block).sum()).backward()
    return mu.grad, lv.grad


# ------------------------------------------------------------------------------------------------ optimizer
def adam_ref(p, m, v, g, t, lr, b1, b2, eps, wd, decoupled, grad_scale=1.0):
    """one step of torch.optim.Adam (wd added to the gradient) / AdamW (decoupled: p *= 1 - lr wd) as documented, t = 1, 2, ..;
    returns the new p, m, v"""
    g = g * grad_scale
    if decoupled:
        p = p * (1 - lr * wd)
    elif wd != 0:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    return p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps), m, v


def torch_optim_run(p0, grads, dtype, lr, b1, b2, eps, wd, decoupled, grad_scale=1.0):
    """the same steps through torch.optim itself in `dtype` -> p, m, v"""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for g in grads:
        p.grad = g.to(dtype) * grad_scale
        opt.step()
    st = opt.state[p]
    return p.detach(), st["exp_avg"], st["exp_avg_sq"]


def adam_hyper(lr, b1, b2, eps, wd):
    """the hyper-parameters as the kernels see them (C `float` arguments)"""
    return f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)


def host_scalars(lr, b1, b2, t):
    """the three scalars svae_adam_step computes in double from its float arguments and hands to the kernel as float"""
    lr, b1, b2 = f32(lr), f32(b1), f32(b2)
    return lr, f32(lr / (1.0 - math.pow(b1, t))), f32(1.0 / math.sqrt(1.0 - math.pow(b2, t)))


# ------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def heads_inputs(B, z, seed=0):
    """h [B, pad16(z) + pad16(z(z+1)/2)] with h ~ N(0, 1), the raw Cholesky columns scaled by 0.3 and the padding columns holding the
    sentinel; eps, dz, dmu, dlv ~ N(0, 1).  All fp64 holding fp32 values."""
    g = _gen(B, z, seed, 1)
    zp, hw = pad16(z), pad16(z) + pad16(ntri(z))
    h = torch.full((B, hw), SENTINEL, dtype=torch.float64)
    h[:, :z] = torch.randn(B, z, generator=g, dtype=torch.float64)
    h[:, zp:zp + ntri(z)] = 0.3 * torch.randn(B, ntri(z), generator=g, dtype=torch.float64)
    rn = lambda *s: r32(torch.randn(*s, generator=g, dtype=torch.float64))
    return dict(h=r32(h), eps=rn(B, z), dz=rn(B, z), dmu=rn(B, z), dlv=rn(B, z), zp=zp, hw=hw, raw_off=zp)


def range_inputs():
    """heads_inputs at RANGE_SHAPE with the raw diagonal entry of (sample b, row i) set to RANGE_DIAG[(b + i) % 7]"""
    B, z = RANGE_SHAPE
    d = heads_inputs(B, z, seed=5)
    for b in range(B):
        for i in range(z):
            d["h"][b, d["raw_off"] + ntri(i) + i] = RANGE_DIAG[(b + i) % len(RANGE_DIAG)]
    d["h"] = r32(d["h"])
    return d


def tc_inputs(B, z, full, spread=False, seed=0):
    """mu, z and the posterior scale -- sigma [B, z] (full = False) or a lower-triangular L [B, z, z] -- of a TC case.
    spread: mu = 6 N(0, 1), sigma = 0.2 U(0.5, 1.5), z = mu + sigma N(0, 1): most exp(q - max) terms underflow and the softmax
    weights are nearly one-hot.  Otherwise mu, eps ~ N(0, 1), raw ~ N(0, 1) (x 0.3 for the Cholesky columns), z = mu + scale eps."""
    g = _gen(B, z, seed, 2 + int(full) + 2 * int(spread))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    mu, eps = rn(B, z) * (6.0 if spread else 1.0), rn(B, z)
    if spread:
        sigma = 0.2 * (0.5 + torch.rand(B, z, generator=g, dtype=torch.float64))
        L = torch.diag_embed(sigma) + 0.02 * torch.tril(rn(B, z, z), -1)
    else:
        sigma = torch.nn.functional.softplus(rn(B, z))
        L = O.cholesky_L(0.3 * rn(B, ntri(z)), z, False)
    mu = r32(mu)
    if full:
        L = r32(L)
        return dict(mu=mu, L=L, sigma=None, z=r32(torch.matmul(L, eps[:, :, None])[:, :, 0] + mu))
    sigma = r32(sigma)
    return dict(mu=mu, L=None, sigma=sigma, z=r32(mu + sigma * eps))


def tc_truth(d, w, dtype, block=128, want_grads=True):
    """restatement of a TC case in `dtype`: lv, loss_j, lse_l, lse_a and (want_grads) d/d mu, d/d lv, d/d sigma (None for full L) of
    w sum_j loss_j"""
    c = lambda t: None if t is None else t.to(dtype)
    mu, L, sigma, zz = c(d["mu"]), c(d["L"]), c(d["sigma"]), c(d["z"])
    if sigma is not None:
        sigma = sigma.clone().requires_grad_(True)
    lv = logvar(L, sigma)
    with torch.no_grad():
        loss, lse_l, lse_a = tc_rows(zz, mu, lv, block, parts=True)
    out = dict(lv=lv.detach(), loss=loss, lse_l=lse_l, lse_a=lse_a)
    if want_grads:
        out["dmu"], out["dlv"] = tc_grads(zz, mu, lv, w, block)
        out["dsigma"] = None
        if sigma is not None:
            lv.backward(out["dlv"])
            out["dsigma"] = sigma.grad
    return out


def heads_truth(d, z, dtype, kl_scale, use, with_eps=True):
    """restatement of a heads case in `dtype`: mu, L, z, KL sum and dh = d/dh of
    kl_scale KL_sum + sum dz z + sum dmu mu + sum dlv logvar(L) over the seeds named in `use` (subset of dz, dmu, dlv)"""
    h = d["h"].to(dtype).clone().requires_grad_(True)
    eps = d["eps"].to(dtype) if with_eps else None
    mu, L, zz, kl = tril_heads(h, eps, z, d["raw_off"])
    obj = kl_scale * kl
    if "dz" in use:
        obj = obj + (d["dz"].to(dtype) * zz).sum()
    if "dmu" in use:
        obj = obj + (d["dmu"].to(dtype) * mu).sum()
    if "dlv" in use:
        obj = obj + (d["dlv"].to(dtype) * logvar(L)).sum()
    obj.backward()
    return dict(mu=mu.detach(), L=L.detach(), z=zz.detach(), kl=kl.detach(), dh=h.grad)


def compose_truth(d, z, dtype, w, block=128):
    """train/losses.py's full-L path: d/dh of w sum_j loss_j through mu and lv = log diag(L L^T), z detached"""
    h = d["h"].to(dtype).clone().requires_grad_(True)
    mu, L, zz, _ = tril_heads(h, d["eps"].to(dtype), z, d["raw_off"])
    lv = logvar(L)
    dmu, dlv = tc_grads(zz.detach(), mu, lv, w, block)
    torch.autograd.backward([mu, lv], [dmu, dlv])
    return h.grad


def opt_inputs(n, steps, seed=0):
    g = _gen(n, steps, seed, 9)
    p0 = torch.randn(n, generator=g, dtype=torch.float32)
    return p0, [torch.randn(n, generator=g, dtype=torch.float32) for _ in range(steps)]
