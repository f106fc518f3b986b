"""The fused scrubber ensemble (csrc/ensemble.hip), the row losses and the diagonal latent heads (csrc/elementwise.hip) on a real
MI355X against the fp64 truth of tests/ensemble_checks.py, view by view: member outputs and input gradients per row, weight gradients
per row of the matrix, loss partials per block, each within max(FACTOR * E32, FLOOR) of the truth (E32: the reference's own fp32
error in the same view).  Run with -s for the GATE lines the header table of ensemble_checks.py was taken from."""
import math

import pytest
import torch

from tests import ensemble_checks as EC
from tests.ensemble_checks import SENTINEL, gate, pad16

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def ops():
    from scrubvae_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


def cu(t):
    return t.float().cuda().contiguous()


def only(t, v):
    """every entry is bit-equal to v"""
    return bool((t == v).all())


def filled(rows, cols, v=SENTINEL):
    return torch.full((rows, cols), v, dtype=F32, device="cuda")


def padded(t, width, fill):
    """[R, C] fp64 -> [R, width] cuda fp32, the extra columns holding `fill`"""
    o = torch.full((t.shape[0], width), fill, dtype=F32)
    o[:, :t.shape[1]] = t.float()
    return o.cuda()


def same(a, b):
    """two result dicts of device tensors / nested lists are bit-identical"""
    fa, fb = EC.ens_views(a), EC.ens_views(b)
    return [n for n, _ in fa] == [n for n, _ in fb] and all(torch.equal(x, y) for (_, x), (_, y) in zip(fa, fb))


# ------------------------------------------------------------------------------------------------ through the runners
def run_fused(D, c, shuffle):
    """one forward and backward of case c through FusedEnsembleRunner -> what it produced (live parts), after the padding checks.
    shuffle: "perm" or "vals" (halves = 2)."""
    d = c["d"]
    B, n0, ind, outd, halves = d["B"], d["n0"], d["ind"], d["outd"], d["halves"]
    ens = EC.StubEns(d, "cuda")
    r = D.FusedEnsembleRunner(ens, B, "cuda", halves)
    assert r.fits()
    ld0 = pad16(n0) + EC.SRC_PAD
    src0 = padded(d["x"], ld0, float("nan"))  # columns >= n0 are never read
    kw = {}
    if halves == 2:
        var = cu(d["var"])
        kw = dict(src1=var, shuf_col=d["shuf_col"])
        if shuffle == "perm":
            kw["perm"] = d["perm"].cuda()
        else:
            kw["shuf_vals"] = var[d["perm"].cuda(), d["shuf_col"]].contiguous()
    outs = r.forward(src0, n0, **kw)
    for t, g in zip(r.d_outs, d["d_outs"]):
        t.zero_()
        t[:, :outd] = cu(g)
    d_src0 = filled(B, ld0)
    raw = r.backward(d_src0, EC.COEF, param_grads=True, accumulate=False, want_raw=True)
    torch.cuda.synchronize()
    assert all(only(o[:, outd:], 0.0) for o in outs)  # padded output columns
    assert only(d_src0[:, n0:], SENTINEL) and only(raw[:, ind:], 0.0)
    for mem in ens.m:
        for l in mem:  # the stale values are overwritten, the padding by exact zeros
            wg, bg = l.weight.grad[0].clone(), l.bias.grad.clone()
            wg[:l.in_f, :l.out_f] = 0
            bg[:l.out_f] = 0
            assert only(wg, 0.0) and only(bg, 0.0)
    return dict(outs=[o[:, :outd].clone() for o in outs], gx=raw[:, :ind].clone(), dsrc=d_src0[:, :n0].clone(),
                dW=[[l.weight.grad[0, :l.in_f, :l.out_f].clone() for l in mem] for mem in ens.m],
                db=[[l.bias.grad[:l.out_f].clone() for l in mem] for mem in ens.m])


def seeded(t, base=SENTINEL, coef=EC.COEF):
    """the truth / yardstick of a d_src0 that held `base`: base + coef * gradient, in the dict's own precision"""
    g = t["dsrc"]
    return dict(t, dsrc=torch.tensor(base, dtype=g.dtype) + torch.tensor(coef, dtype=g.dtype) * g)


def check_fused(D, case, tag):
    c = EC.ens_case(*case)
    halves = case[3]
    got = run_fused(D, c, "perm")
    gate(f"ens {tag} {case}", EC.ens_records(got, seeded(c["t64"]), seeded(c["t32"])))
    if halves == 2:
        assert same(got, run_fused(D, c, "vals"))  # the shuffled values themselves instead of the permutation: bit for bit


@pytest.fixture
def D(monkeypatch):
    from scrubvae_amd.model import disentangle
    monkeypatch.setattr(disentangle, "LinearP", EC.StubLin)  # the runners pick the Linear layers of a member by isinstance
    return disentangle


@pytest.mark.parametrize("case", EC.RUNNER_H1, ids=str)
def test_fused_one_half(ops, D, case):
    check_fused(D, case, "h1")


@pytest.mark.parametrize("case", EC.RUNNER_H2, ids=str)
def test_fused_two_halves(ops, D, case):
    check_fused(D, case, "h2")


@pytest.mark.parametrize("case", EC.GEOMETRY, ids=str)
def test_fused_geometry(ops, D, case):
    check_fused(D, case, "geom")


def test_lds_ceiling_and_the_gemm_path_beyond_it(ops, D):
    """(64, 16) is the widest ensemble that fits; (65, 16) is refused for its LDS and runs Linear by Linear on the GEMM kernels"""
    from scrubvae_amd import _lib
    ind, outd = EC.TOO_WIDE
    B, halves = 33, 2
    c = EC.ens_case(ind, outd, B, halves)
    d, rows = c["d"], B * halves
    assert D.FusedEnsembleRunner(EC.StubEns(EC.ens_case(*EC.CEILING, 65, 1)["d"], "cuda"), 65, "cuda", 1).fits()
    ens = EC.StubEns(d, "cuda")
    assert not D.FusedEnsembleRunner(ens, B, "cuda", halves).fits()
    assert "LDS" in _lib.last_error()
    r = D.EnsembleRunner(ens, rows, "cuda")
    outs = r.forward(padded(EC.assemble(d, F64), pad16(ind), 0.0))
    gin = r.backward([padded(g, pad16(outd), 0.0) for g in d["d_outs"]], param_grads=True, accumulate=False)
    torch.cuda.synchronize()
    got = dict(outs=[o[:, :outd] for o in outs], gx=gin[:, :ind],
               dW=[[l.weight.grad[0, :l.in_f, :l.out_f] for l in mem] for mem in ens.m],
               db=[[l.bias.grad[:l.out_f] for l in mem] for mem in ens.m])
    gate(f"ens gemm ({ind}, {outd}, {B}, {halves})", EC.ens_records(got, c["t64"], c["t32"]))


# ------------------------------------------------------------------------------------------------ on the descriptor itself
class Dev:
    """device tensors and the svae_ens_desc of one case.  grads[m]: member m gets dw / db pointers.  Every output (out, dw, db, gx_raw,
    d_src0) starts as SENTINEL; base: what d_src0 holds instead."""

    def __init__(self, c, grads=None):
        from scrubvae_amd import _lib
        d = self.d = c["d"]
        self.c = c
        B, n0, halves = d["B"], d["n0"], d["halves"]
        self.nm = len(d["W"])
        self.grads = grads or [True] * self.nm
        self.w = [[cu(w) for w, _ in mem] for mem in d["W"]]
        self.b = [[cu(b) for _, b in mem] for mem in d["W"]]
        self.dw = [[torch.full_like(w, SENTINEL) for w in mem] for mem in self.w]
        self.db = [[torch.full_like(b, SENTINEL) for b in mem] for mem in self.b]
        self.out = [filled(d["rows"], d["outd"]) for _ in range(self.nm)]
        self.d_out = [cu(g) for g in d["d_outs"]]
        self.ld0 = pad16(n0) + EC.SRC_PAD
        self.src0 = padded(d["x"], self.ld0, float("nan"))
        self.var, self.perm = cu(d["var"]), d["perm"].cuda()
        self.gx = filled(d["rows"], pad16(d["ind"]))
        self.d_src0 = filled(B, self.ld0)
        D = self.desc = _lib.EnsDesc()
        D.n_members, D.batch, D.halves = self.nm, B, halves
        D.src0, D.ld0, D.n0 = self.src0.data_ptr(), self.ld0, n0
        if halves == 2:
            D.src1, D.ld1, D.n1 = self.var.data_ptr(), EC.N1, EC.N1
            D.perm, D.shuf_col = self.perm.data_ptr(), d["shuf_col"]
        for mi in range(self.nm):
            M = D.member[mi]
            M.n_layers, M.out, M.d_out = len(self.w[mi]), self.out[mi].data_ptr(), self.d_out[mi].data_ptr()
            for li, w in enumerate(self.w[mi]):
                L = M.layer[li]
                L.w, L.b, L.K, L.N = w.data_ptr(), self.b[mi][li].data_ptr(), w.shape[0], w.shape[1]
                if self.grads[mi]:
                    L.dw, L.db = self.dw[mi][li].data_ptr(), self.db[mi][li].data_ptr()

    def workspace(self, ops, fill=float("nan")):
        need = ops.ens_bwd_workspace(self.desc)
        assert need > 0
        return torch.full((need // 4 + 64,), fill, dtype=F32, device="cuda")

    def run(self, ops, d_src0=True, gx=True, accumulate=False, ws_fill=float("nan"), base=SENTINEL, fwd=True):
        """forward and backward -> the result dict (clones); the outputs not asked for stay None and their tensors untouched"""
        if fwd:
            ops.ens_fwd(self.desc)
        self.d_src0.fill_(base)
        ops.ens_bwd(self.desc, self.d_src0 if d_src0 else None, self.ld0, EC.COEF, self.gx if gx else None, self.workspace(ops, ws_fill),
                    accumulate)
        torch.cuda.synchronize()
        n0, ind = self.d["n0"], self.d["ind"]
        assert only(self.d_src0[:, n0:], base) and (d_src0 or only(self.d_src0, base)) and (gx or only(self.gx, SENTINEL))
        g = lambda ts: [[t.clone() for t in mem] if self.grads[mi] else None for mi, mem in enumerate(ts)]
        return dict(outs=[o.clone() for o in self.out], gx=self.gx[:, :ind].clone() if gx else None,
                    dsrc=self.d_src0[:, :n0].clone() if d_src0 else None, dW=g(self.dw), db=g(self.db))

    def outputs(self):
        return self.out + [self.gx, self.d_src0] + [t for mem in self.dw + self.db for t in mem]

    def untouched(self):
        torch.cuda.synchronize()
        return all(only(t, SENTINEL) for t in self.outputs())


def direct(name):
    return EC.ens_case(*EC.DIRECT[name])


def grads_only(t, keep):
    """the truth dict with the parameter gradients of the members not in `keep` removed"""
    return dict(t, dW=[m if i in keep else None for i, m in enumerate(t["dW"])], db=[m if i in keep else None for i, m in enumerate(t["db"])])


@pytest.mark.parametrize("name", ["m1", "m2", "m3", "one_layer", "h2"])
def test_descriptor_members_and_layers(ops, name):
    """fewer than four members, a member that is a single Linear, and both halves with parameter gradients; d_src0 starts at 0, so
    the view is the input gradient itself"""
    c = direct(name)
    got = Dev(c).run(ops, base=0.0)
    gate(f"ens direct {name}", EC.ens_records(got, seeded(c["t64"], 0.0), seeded(c["t32"], 0.0)))


def test_descriptor_mixed_parameter_gradients(ops):
    """member 1 without dw / db: every later member's workspace offset moves up"""
    c = direct("full")
    v = Dev(c, grads=[True, False, True, True])
    got = v.run(ops)
    gate("ens direct mixed", EC.ens_records(got, seeded(grads_only(c["t64"], (0, 2, 3))), seeded(grads_only(c["t32"], (0, 2, 3)))))
    assert all(only(t, SENTINEL) for t in v.dw[1] + v.db[1])


def test_descriptor_accumulate(ops):
    """accumulate = 1 adds onto what every layer's dw / db hold, accumulate = 0 overwrites it"""
    c = direct("full")
    v = Dev(c)
    add = lambda t: dict(t, dW=[[w + torch.tensor(SENTINEL, dtype=w.dtype) for w in m] for m in t["dW"]],
                         db=[[b + torch.tensor(SENTINEL, dtype=b.dtype) for b in m] for m in t["db"]])
    gate("ens direct accumulate=1", EC.ens_records(v.run(ops, accumulate=True), seeded(add(c["t64"])), seeded(add(c["t32"]))))
    gate("ens direct accumulate=0", EC.ens_records(v.run(ops, accumulate=False), seeded(c["t64"]), seeded(c["t32"])))


@pytest.mark.parametrize("name", ["full", "h2"])
def test_descriptor_workspace_hygiene_and_repeatability(ops, name):
    """the finish kernel reads only partials written in the same launch (a NaN-filled and a zeroed workspace give the same bits), and
    two consecutive passes are bit-identical (fixed-order sums, no atomics)"""
    c = direct(name)
    a = Dev(c).run(ops, ws_fill=float("nan"))
    assert all(bool(torch.isfinite(t).all()) for _, t in EC.ens_views(a))
    assert same(a, Dev(c).run(ops, ws_fill=0.0))
    v = Dev(c)
    first, second = v.run(ops), v.run(ops)
    assert same(first, second) and same(first, a)


def test_descriptor_optional_outputs(ops):
    c = direct("full")
    t64, t32 = seeded(c["t64"]), seeded(c["t32"])
    gate("ens direct gx only", EC.ens_records(Dev(c).run(ops, d_src0=False), t64, t32))
    gate("ens direct d_src0 only", EC.ens_records(Dev(c).run(ops, gx=False), t64, t32))
    gate("ens direct params only", EC.ens_records(Dev(c).run(ops, d_src0=False, gx=False), t64, t32))


def _set(path, value):
    def f(v):
        o = v.desc
        for p in path[:-1]:
            o = o[p] if isinstance(p, int) else getattr(o, p)
        setattr(o, path[-1], value(o) if callable(value) else value)
    return f


DESC_REJECTS = [  # name, case, what to break in the descriptor; both passes and the workspace query have to refuse it
    ("0 members", "full", _set(("n_members",), 0)),
    ("5 members", "full", _set(("n_members",), 5)),
    ("halves=3", "full", _set(("halves",), 3)),
    ("no perm, no shuf_vals", "h2", _set(("perm",), None)),
    ("shuf_col >= n1", "h2", _set(("shuf_col",), EC.N1)),
    ("K < n0 + n1", "full", _set(("n0",), 33)),
    ("K % 16", "full", _set(("member", 0, "layer", 0, "K"), 40)),
    ("K != previous N", "full", _set(("member", 0, "layer", 1, "K"), 48)),
    ("weight pointer + 4 B", "full", _set(("member", 3, "layer", 1, "w"), lambda L: L.w + 4)),
]


@pytest.mark.parametrize("name,case,breaker", DESC_REJECTS, ids=[r[0] for r in DESC_REJECTS])
def test_descriptor_rejections(ops, name, case, breaker):
    """none of these launches a kernel: each raises and leaves every output untouched"""
    v = Dev(direct(case))
    ws = v.workspace(ops)
    breaker(v)
    assert ops.ens_bwd_workspace(v.desc) == 0
    with pytest.raises(RuntimeError):
        ops.ens_fwd(v.desc)
    with pytest.raises(RuntimeError):
        ops.ens_bwd(v.desc, v.d_src0, v.ld0, EC.COEF, v.gx, ws, False)
    assert v.untouched()


def test_pass_rejections(ops):
    from scrubvae_amd import _lib
    v = Dev(direct("full"))
    ws = v.workspace(ops)
    exact = (ops.ens_bwd_workspace(v.desc) - 256) // 4  # the floats the backward itself asks for
    with pytest.raises(RuntimeError) as e:
        ops.ens_bwd(v.desc, v.d_src0, v.ld0, EC.COEF, v.gx, ws[:exact - 1], False)
    assert e.value.status == _lib.ERR_WORKSPACE
    with pytest.raises(RuntimeError):
        ops.ens_bwd(v.desc, v.d_src0, v.d["n0"] - 1, EC.COEF, v.gx, ws, False)  # ld_d < n0
    v.desc.member[2].d_out = None
    with pytest.raises(RuntimeError):
        ops.ens_bwd(v.desc, v.d_src0, v.ld0, EC.COEF, v.gx, ws, False)
    v.desc.member[2].d_out = v.d_out[2].data_ptr()
    v.desc.member[1].out = None
    with pytest.raises(RuntimeError):
        ops.ens_fwd(v.desc)
    assert v.untouched()
    v.desc.member[1].out = v.out[1].data_ptr()
    c = v.c
    gate("ens direct after rejections", EC.ens_records(v.run(ops), seeded(c["t64"]), seeded(c["t32"])))  # the exact size is enough
    v2 = Dev(c)
    ops.ens_fwd(v2.desc)
    ops.ens_bwd(v2.desc, v2.d_src0, v2.ld0, EC.COEF, v2.gx, ws[:exact], False)
    torch.cuda.synchronize()
    assert torch.equal(v2.gx, v.gx) and torch.equal(v2.d_src0, v.d_src0)


# ------------------------------------------------------------------------------------------------ row losses
def loss_device(d, ld_t):
    outs = [padded(o, EC.LOSS_LD, SENTINEL) for o in d["outs"]]
    tgt = padded(d["target"], ld_t, float("nan")) if d["kind"] == 0 else None
    lab = d["labels"].int().cuda() if d["kind"] == 1 else None
    return outs, tgt, lab


@pytest.mark.parametrize("case", EC.LOSS_CASES, ids=str)
def test_ens_loss(ops, case):
    """all members in one launch: part[m nb + block] = lw[m] * the block's sum, dpred[m] = gs[m] * gradient; one member without dpred"""
    kind, C, rows, scale = case
    nb = ops.rowloss_blocks(rows)
    assert nb == (rows + EC.LOSS_BLOCK - 1) // EC.LOSS_BLOCK
    for n in (4, 1) if rows in (2, 258) else (4,):
        c = EC.loss_case(kind, C, rows, scale, n)
        d = c["d"]
        for ld_t in ((C, C + 5) if kind == 0 else (C,)):
            outs, tgt, lab = loss_device(d, ld_t)
            skip = 1 if n == 4 else None
            dp = [None if m == skip else filled(rows, EC.LOSS_LD) for m in range(n)]
            part = torch.full((n * nb,), SENTINEL, dtype=F32, device="cuda")
            ops.ens_loss(kind, outs, dp, EC.LW[:n], EC.GS[:n], tgt, ld_t, lab, rows, C, EC.LOSS_LD, part)
            torch.cuda.synchronize()
            assert all(t is None or only(t[:, C:], SENTINEL) for t in dp)
            got = [None if t is None else t[:, :C] for t in dp]
            gate(f"ens_loss {case} n={n} ld_t={ld_t}", EC.loss_records(part, got, c["t64"], c["t32"], d))


@pytest.mark.parametrize("case", EC.LOSS_CASES, ids=str)
def test_member_losses(ops, case):
    """mse_sum / ce_sum / double_softmax_ce_sum: the partials are the plain block sums, dpred = scale * gradient"""
    kind, C, rows, scale = case
    c = EC.loss_case(kind, C, rows, scale)
    d = c["d"]
    nb = ops.rowloss_blocks(rows)
    for ld_t in ((C, C + 5) if kind == 0 else (C,)):
        outs, tgt, lab = loss_device(d, ld_t)
        rec = []
        for m in (0, 3):
            dp, part = filled(rows, EC.LOSS_LD), torch.full((nb,), SENTINEL, dtype=F32, device="cuda")
            if kind == 0:
                ops.mse_sum(outs[m], EC.LOSS_LD, tgt, ld_t, rows, C, EC.GS[m], part, dp)
            elif kind == 1:
                ops.ce_sum(outs[m], EC.LOSS_LD, lab, rows, C, EC.GS[m], part, dp)
            else:
                ops.double_softmax_ce_sum(outs[m], EC.LOSS_LD, rows, EC.GS[m], part, dp)
            torch.cuda.synchronize()
            assert only(dp[:, C:], SENTINEL)
            rec.append(EC.per_block(f"part{m}", part, c["t64"]["raw"][m], c["t32"]["raw"][m], EC.LOSS_BLOCK))
            rec += EC.dpred_records(f"dpred{m}", dp[:, :C], c["t64"]["dpred"][m], c["t32"]["dpred"][m], scale)
        gate(f"member_loss {case} ld_t={ld_t}", rec)


def test_loss_rejections(ops):
    """kind 2 with odd rows or C = 3, kind 0 without a target, ld < C: refused before any launch"""
    rows, ld = 6, EC.LOSS_LD
    outs = [filled(rows, ld, 0.5) for _ in range(2)]
    dp = [filled(rows, ld) for _ in range(2)]
    part = torch.full((2,), SENTINEL, dtype=F32, device="cuda")
    tgt, lab = filled(rows, ld, 0.25), torch.zeros(rows, dtype=torch.int32, device="cuda")
    lw, gs = EC.LW[:2], EC.GS[:2]
    bad = [
        lambda: ops.ens_loss(2, outs, dp, lw, gs, None, 0, None, rows - 1, 2, ld, part),
        lambda: ops.ens_loss(2, outs, dp, lw, gs, None, 0, None, rows, 3, ld, part),
        lambda: ops.ens_loss(0, outs, dp, lw, gs, None, ld, None, rows, 3, ld, part),
        lambda: ops.ens_loss(0, outs, dp, lw, gs, tgt, ld, None, rows, 3, 2, part),
        lambda: ops.ens_loss(0, outs, dp, lw, gs, tgt, 2, None, rows, 3, ld, part),
        lambda: ops.ens_loss(1, outs, dp, lw, gs, None, 0, lab, rows, 3, 2, part),
        lambda: ops.double_softmax_ce_sum(outs[0], ld, rows - 1, 1.0, part, dp[0]),
        lambda: ops.mse_sum(outs[0], ld, None, ld, rows, 3, 1.0, part, dp[0]),
        lambda: ops.mse_sum(outs[0], 2, tgt, ld, rows, 3, 1.0, part, dp[0]),
        lambda: ops.mse_sum(outs[0], ld, tgt, 2, rows, 3, 1.0, part, dp[0]),
        lambda: ops.ce_sum(outs[0], 2, lab, rows, 3, 1.0, part, dp[0]),
    ]
    for f in bad:
        with pytest.raises(RuntimeError):
            f()
    torch.cuda.synchronize()
    assert only(part, SENTINEL) and all(only(t, SENTINEL) for t in dp)


# ------------------------------------------------------------------------------------------------ diagonal heads
def check_diag(ops, B, z, ranged, tag):
    c = EC.diag_case(B, z, ranged)
    d, ks = c["d"], EC.diag_kl_scale(B)
    nb = ops.heads_blocks(B, z)
    assert nb == (B * z + EC.DIAG_BLOCK - 1) // EC.DIAG_BLOCK
    for wide in (False, True):
        ld, raw_off, ldm, ldz, lddz = EC.diag_layout(z, wide)
        args = dict(raw_off=raw_off, ldm=ldm) if wide else {}  # the narrow layout is the wrapper's default
        for fill in ((SENTINEL, float("nan")) if wide else (SENTINEL,)):
            h = torch.full((B, ld), fill, dtype=F32)
            h[:, :z], h[:, raw_off:raw_off + z] = d["mu"].float(), d["raw"].float()
            h = h.cuda()
            h0 = h.clone()
            live = torch.zeros(ld, dtype=torch.bool, device="cuda")
            live[:z], live[raw_off:raw_off + z] = True, True
            eps = cu(d["eps"])
            for with_eps in (True, False):
                mu, sig, zz, klp = filled(B, ldm), filled(B, ldm), filled(B, ldz), torch.full((nb,), SENTINEL, dtype=F32, device="cuda")
                ops.heads_diag_fwd(h, ld, eps if with_eps else None, mu, sig, zz, ldz, klp, B, z, **args)
                torch.cuda.synchronize()
                assert only(mu[:, z:], SENTINEL) and only(sig[:, z:], SENTINEL) and only(zz[:, z:], SENTINEL)
                assert torch.equal(h.view(torch.int32), h0.view(torch.int32))
                for use in EC.DIAG_USES:
                    t64, t32 = c["t64"][(use, with_eps)], c["t32"][(use, with_eps)]
                    seed = lambda k, w: padded(d[k], w, fill) if k in use else None
                    dh = filled(B, ld)
                    ops.heads_diag_bwd(h, ld, eps if with_eps else None, sig, seed("dz", lddz), lddz, seed("dmu", ldm), seed("dsigma", ldm),
                                       ks, dh, B, z, **args)
                    torch.cuda.synchronize()
                    assert only(dh[:, ~live], SENTINEL)
                    got = dict(mu=mu[:, :z], sigma=sig[:, :z], z=zz[:, :z], kl_part=klp, dh=torch.cat([dh[:, :z], dh[:, raw_off:raw_off + z]], 1))
                    name = f"heads_diag {tag} ({B}, {z}) {'wide' if wide else 'default'} eps={int(with_eps)} {'+'.join(use)}"
                    gate(name, EC.diag_records(got, t64, t32))


@pytest.mark.parametrize("B,z", EC.DIAG_SHAPES, ids=str)
def test_heads_diag(ops, B, z):
    check_diag(ops, B, z, False, "shape")


def test_heads_diag_range(ops):
    """raw on both sides of softplus's threshold 20 and down to sigma = softplus(-30) ~ 1e-13"""
    check_diag(ops, *EC.RANGE_SHAPE, True, "range")
    assert math.isclose(math.log1p(math.exp(-30.0)), 9.357622968839299e-14, rel_tol=1e-12)
