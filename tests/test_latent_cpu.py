"""Pins the helpers of tests/latent_checks.py against oracle/scvae_oracle.py and torch.optim, checks that every input generator of
test_gpu_latent.py yields finite fp64 truths (a GPU case can never pass or fail on NaN == NaN), and that every public function of
scrubvae_amd/ops.py is called by some test."""
import ast
import glob
import os
import re

import pytest
import torch

from oracle import scvae_oracle as O
from tests import latent_checks as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 300  # the CPU suite evaluates truths up to this batch; the larger cases are evaluated by the GPU tests on the GPU box's CPUs


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("B,z", [(1, 1), (5, 8), (12, 8), (37, 31), (64, 32)])
@pytest.mark.parametrize("full", [False, True])
def test_tc_rows_equals_oracle_total_correlation(B, z, full):
    d = LC.tc_inputs(B, z, full)
    L = d["L"] if full else torch.diag_embed(d["sigma"])
    ref = O.total_correlation(d["z"], d["mu"], L)
    lv = LC.logvar(d["L"], d["sigma"])
    rows, _, lse_a = LC.tc_rows(d["z"], d["mu"], lv, parts=True)
    scale = float(lse_a.abs().max()) if B == 1 else float(ref.abs())  # B = 1: the loss is 0, the difference of two equal terms
    assert abs(float(rows.mean() - ref)) <= 1e-12 * scale
    for block in (1, 7, 1000):
        assert float((LC.tc_rows(d["z"], d["mu"], lv, block) - rows).abs().max()) <= 1e-13 * scale


@pytest.mark.parametrize("B,z", [(12, 8), (37, 31)])
@pytest.mark.parametrize("full", [False, True])
def test_tc_grads_equal_oracle_autograd(B, z, full):
    """the blockwise gradients equal autograd through oracle.total_correlation (times B: the oracle takes the mean)"""
    d = LC.tc_inputs(B, z, full)
    mu = d["mu"].clone().requires_grad_(True)
    s = (d["L"] if full else d["sigma"]).clone().requires_grad_(True)
    (0.7 * B * O.total_correlation(d["z"], mu, s if full else torch.diag_embed(s))).backward()
    for block in (5, 128):
        t = LC.tc_truth(d, 0.7, torch.float64, block)
        assert rel(t["dmu"], mu.grad) <= 1e-12
        if full:  # chain d/d lv through lv = log diag(L L^T) to compare with the oracle's d/d L
            Lg = d["L"].clone().requires_grad_(True)
            LC.logvar(L=Lg).backward(t["dlv"])
            assert rel(Lg.grad, s.grad) <= 1e-12
        else:
            assert rel(t["dsigma"], s.grad) <= 1e-12


def test_tril_heads_equals_oracle():
    B, z = 5, 8
    d = LC.heads_inputs(B, z)
    mu, L, zz, kl = LC.tril_heads(d["h"], d["eps"], z, d["raw_off"])
    raw = d["h"][:, d["raw_off"]:d["raw_off"] + LC.ntri(z)]
    assert torch.equal(L, O.cholesky_L(raw, z, False)) and torch.equal(L, torch.tril(L))
    assert rel(zz, torch.einsum("bij,bj->bi", L, d["eps"]) + mu) <= 1e-15
    assert abs(float(kl / B - O.prior_loss(mu, L))) <= 1e-15 * float(kl)
    assert torch.equal(LC.tril_heads(d["h"], None, z, d["raw_off"])[2], mu)
    assert rel(LC.logvar(sigma=L.diagonal(dim1=1, dim2=2)), LC.logvar(L=torch.diag_embed(L.diagonal(dim1=1, dim2=2)))) <= 1e-14


@pytest.mark.parametrize("name,decoupled,wd,gs", LC.OPT_CONFIGS)
def test_adam_ref_equals_torch_optim(name, decoupled, wd, gs):
    lr, b1, b2, eps, wd = LC.adam_hyper(LC.LR, LC.BETA1, LC.BETA2, LC.ADAM_EPS, wd)
    p0, grads = LC.opt_inputs(4160, 5)
    p, m, v = p0.double(), torch.zeros(4160, dtype=torch.float64), torch.zeros(4160, dtype=torch.float64)
    for t, g in enumerate(grads, 1):
        p, m, v = LC.adam_ref(p, m, v, g.double(), t, lr, b1, b2, eps, wd, decoupled, gs)
    tp, tm, tv = LC.torch_optim_run(p0, grads, torch.float64, lr, b1, b2, eps, wd, decoupled, gs)
    assert rel(p, tp) <= 1e-14 and rel(m, tm) <= 1e-14 and rel(v, tv) <= 1e-14
    assert float((p - p0.double()).abs().max()) > 1e-3  # the steps moved the parameters


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts if t is not None)


@pytest.mark.parametrize("B,z", [s for s in LC.HEADS_SHAPES if s[0] <= SMALL] + [LC.RANGE_SHAPE])
def test_heads_generators_finite(B, z):
    for d in ([LC.range_inputs()] if (B, z) == LC.RANGE_SHAPE else []) + [LC.heads_inputs(B, z)]:
        for use in (("dz", "dmu", "dlv"), (), ("dlv",)):
            for dtype in (torch.float64, torch.float32):
                t = LC.heads_truth(d, z, dtype, 0.5, use)
                assert _finite(*t.values()), (B, z, use, dtype)
        assert _finite(LC.compose_truth(d, z, torch.float64, 0.7))


@pytest.mark.parametrize("B,z", [s for s in LC.TC_SHAPES if s[0] <= SMALL])
@pytest.mark.parametrize("full", [False, True])
def test_tc_generators_finite(B, z, full):
    cases = [LC.tc_inputs(B, z, full)] + ([LC.tc_inputs(B, z, full, spread=True)] if (B, z) in LC.SPREAD_SHAPES else [])
    for d in cases:
        for dtype in (torch.float64, torch.float32):
            t = LC.tc_truth(d, 0.7, dtype)
            assert _finite(*t.values()), (B, z, full, dtype)


def test_large_generators_finite_inputs():
    """the B = 4096 and (512, 128) truths are left to the GPU tests (which assert their finiteness before comparing); here only
    that their inputs are finite and sigma / diag(L) positive"""
    for B, z in [s for s in LC.TC_SHAPES if s[0] > SMALL]:
        for full in (False, True):
            for spread in {False, (B, z) in LC.SPREAD_SHAPES}:
                d = LC.tc_inputs(B, z, full, spread)
                assert _finite(*d.values())
                s = d["L"].diagonal(dim1=1, dim2=2) if full else d["sigma"]
                assert float(s.min()) > 0
    for B, z in [s for s in LC.HEADS_SHAPES if s[0] > SMALL]:
        d = LC.heads_inputs(B, z)
        assert _finite(d["h"], d["eps"], d["dz"], d["dmu"], d["dlv"])


# ------------------------------------------------------------------------------------------------ "every C-ABI op"
# Public functions of scrubvae_amd/ops.py that need no test of their own, each with the reason.
ALLOWED_UNTESTED = {
    "pad16": "pure helper (rounds a width up to 16)",
    "check_current_device": "host-side guard, no kernel",
    "up2_supported": "host-side predicate, no kernel",
    "split_weights_batched": "driven through every model pass (ResVAE forward) by the test_gpu_model.py parity tests",
    "linear_weight_to_tio": "weight-layout converter (host tensor ops), no kernel",
    "linear_weight_from_tio": "weight-layout converter (host tensor ops), no kernel",
    "kde_mi": "driven through model/disentangle.py's MutInfoEstimator by test_kde_mi_vs_fp64",
    "kde_mi_autograd": "driven through model/disentangle.py's MutInfoEstimator by test_kde_mi_vs_fp64",
}


def _public_ops():
    tree = ast.parse(open(os.path.join(ROOT, "scrubvae_amd", "ops.py")).read())
    return [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and not n.name.startswith("_")]


def test_every_public_op_is_called_by_a_test():
    me = os.path.abspath(__file__)
    text = "\n".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True))
                     if os.path.abspath(f) != me)
    names = _public_ops()
    assert len(names) > 50 and "tc_fwd" in names and "adam_step_dev" in names
    missing = [n for n in names if n not in ALLOWED_UNTESTED and not re.search(r"\bops\." + n + r"\b", text)]
    assert not missing, f"ops.py functions no test calls: {missing}"
    stale = [n for n in ALLOWED_UNTESTED if n not in names]
    assert not stale, f"allow-list names that ops.py no longer defines: {stale}"
