"""The 16-byte epilogue path of the split forward / data-gradient kernels (tile_epilogue's LDS transposition, csrc/split_gather.h)
against the dword path: the same launch with the switch (ops.set_epilogue_wide) off and on must leave the SAME BITS in every buffer
it touches -- C, the BatchNorm partials, the slope-partial pairs, the up2 by-product -- and nothing outside [0, M) x [0, N): the
buffers are NaN-filled, wider (ld > N where stated) and longer than the launch needs.  The kernels with the wide path are the
8-wave gather kernels (tile variants 0 .. 3) and the 8-wave halo kernels (8, 9, 19, 29); the wave-specialised variants keep the
dword path, and so do launches whose epilogue only stores.  Per family, piece count and shape, launches that run the 16-byte path
(accumulating forward and data gradient, fused data gradient with its partials) are also held to torch fp64 (_fp64_checks), so the
comparison is not only of the code with itself."""
import math

import pytest
import torch

import tests.test_gpu_kernels as K
from scrubvae_amd._lib import BnBwdFuse

pytestmark = pytest.mark.gpu

_WIDE_VARIANTS = {"gather": (0, 1, 2, 3), "halo": (8, 9, 19, 29)}
_SLACK = 3 * 4096 + 8  # NaN floats behind every output's last row


def _pairs():
    """(code, pieces) of the kernels with the wide path, from the code lists of test_split_gather_kernels."""
    out = []
    for lists in (K._SPLIT_GATHER_LISTS, K._SPLIT_GATHER_TABLE):
        for pieces, codes in lists.items():
            for code in codes:
                if any(code // 1000000 in v for v in _WIDE_VARIANTS.values()) and (code, pieces) not in out:
                    out.append((code, pieces))
    return out


def _up2_pairs():
    for m in K.test_conv_behind_upsample_fused.pytestmark:
        if m.name == "parametrize" and m.args[0] == "fcode,pieces":
            return list(m.args[1])
    raise AssertionError("test_conv_behind_upsample_fused lost its (fcode, pieces) list")


def _family(code):
    return "halo" if code // 1000000 in _WIDE_VARIANTS["halo"] else "gather"


CASES = [
    # B, L, Cin, Cout, k, stride, pad, transposed, extra leading dimension
    ((2, 5, 40, 24, 5, 2, 2, False), 0),      # odd length, two parity phases of unequal length, N = 32 of which 24 real
    ((9, 4, 64, 48, 5, 2, 2, True), 0),       # N = 48: a half-filled second 32-column block; interleaved phase rows
    ((2, 49, 64, 141, 22, 1, 3, True), 0),    # N = 144 on 64-, 128- and 160-column tiles
    ((200, 1, 512, 64, 1, 1, 0, False), 0),   # M not a tile multiple
    ((33, 1, 40, 4096, 1, 1, 0, False), 0),   # many column tiles
    ((1, 1, 32, 48, 1, 1, 0, False), 0),      # M = 1
    ((65, 1, 32, 32, 1, 1, 0, False), 0),     # M = tile rows + 1 for the 64-,
    ((129, 1, 48, 32, 1, 1, 0, False), 0),    # the 128-
    ((257, 1, 32, 80, 1, 1, 0, False), 0),    # and the 256-row tiles
    ((9, 4, 64, 48, 5, 2, 2, True), 20),      # ld = N + 20: rows start 16-byte aligned, the columns [N, ld) belong to somebody else
]
UP2_GEO = (5, 7, 32, 64)


def _nan_buf(rows, ld):
    return torch.full((rows * ld + _SLACK,), float("nan"), device="cuda")


def _rows_view(buf, rows, ld):
    return buf[: rows * ld].view(rows, ld)


def _check_outside(buf, rows, ld, width, what):
    """Only [0, rows) x [0, width) of the [rows, ld] image at the head of buf was written; all of that was."""
    v = _rows_view(buf, rows, ld)
    assert not torch.isnan(v[:, :width]).any(), f"{what}: elements left unwritten"
    assert torch.isnan(v[:, width:]).all(), f"{what}: written into the columns [{width}, {ld})"
    assert torch.isnan(buf[rows * ld:]).all(), f"{what}: written behind the buffer's last row"


def _same_bits(a, b, what):
    ne = a.view(torch.int32) != b.view(torch.int32)
    if bool(ne.any()):
        i = int(ne.nonzero()[0])
        raise AssertionError(f"{what}: the 16-byte path differs from the dword path in {int(ne.sum())} of {ne.numel()} elements, "
                             f"first at {i}: {float(a[i])!r} / {float(b[i])!r}")


def _to_ld(t, ld):
    """[rows, C] -> [rows, ld] with NaN in the columns behind C (nobody may read them)."""
    out = torch.full((t.shape[0], ld), float("nan"), device="cuda")
    out[:, : t.shape[1]] = t
    return out.contiguous()


def _fuse_inputs(rows, Cp, ld, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    gamma = 1 + 0.2 * torch.randn(Cp, generator=g, device="cuda")
    beta = 0.3 * torch.randn(Cp, generator=g, device="cuda")
    mean = 0.5 * torch.randn(Cp, generator=g, device="cuda")
    rstd = 0.5 + torch.rand(Cp, generator=g, device="cuda")
    scale = gamma * rstd
    shift = beta - mean * scale
    x = _to_ld(torch.randn(rows, Cp, generator=g, device="cuda"), ld)
    old = torch.randn(rows, Cp, generator=g, device="cuda")
    return dict(scale=scale, shift=shift, mean=mean, rstd=rstd, alpha=torch.tensor([0.25], device="cuda"), x=x, old=old)


def _launches(ops, cvf, cvd, xd, dyd, wd, bd, fz, up2):
    """Every launch of the list in the module's docstring, into fresh NaN-filled buffers: [(name, buffer, rows, ld, width)]."""
    out = []
    rows_f, ldf, Nf = cvf.batch * cvf.l_out, cvf.desc.ld_out, cvf.c_out_p
    rows_d, ldd, Nd = cvd.batch * cvd.l_in, cvd.desc.ld_in, cvd.c_in_p
    g = torch.Generator(device="cuda").manual_seed(5)
    old_f = torch.randn(rows_f, Nf, generator=g, device="cuda")

    def fresh(rows, ld, width, old=None):
        buf = _nan_buf(rows, ld)
        if old is not None:
            _rows_view(buf, rows, ld)[:, :width] = old
        return buf

    # forward: plain, accumulate, with statistics (up2: with the upsampled rows as a by-product)
    y = fresh(rows_f, ldf, Nf)
    cvf.fwd(xd, wd, bd, y)
    out.append(("fwd", y, rows_f, ldf, Nf))
    y = fresh(rows_f, ldf, Nf, old_f)
    cvf.fwd(xd, wd, bd, y, accumulate=True)
    out.append(("fwd accumulate", y, rows_f, ldf, Nf))
    nt = cvf.stats_tiles()
    assert nt > 0
    for acc in (False, True):
        y = fresh(rows_f, ldf, Nf, old_f if acc else None)
        part = _nan_buf(nt * 2, Nf)
        upo = _nan_buf(cvf.batch * cvf.l_in, cvf.c_in_p) if up2 else None
        cvf.fwd(xd, wd, bd, y, accumulate=acc, stats=part, up_out=upo)
        out.append((f"fwd stats acc={acc}", y, rows_f, ldf, Nf))
        out.append((f"fwd stats acc={acc}: partials", part, nt * 2, Nf, Nf))
        if up2:
            out.append((f"fwd stats acc={acc}: upsampled rows", upo, cvf.batch * cvf.l_in, cvf.c_in_p, cvf.c_in_p))
    # data gradient: plain, accumulate, and with the fused BatchNorm + PReLU / BatchNorm + tanh / bare PReLU backward sums
    n, cb = cvd.dgrad_stats_tiles()
    assert n > 0
    for mode in (None, "bn_prelu", "bn_tanh", "bare"):
        for acc in (False, True):
            dx = fresh(rows_d, ldd, Nd, fz["old"] if acc else None)
            f = part = dap = None
            if mode:
                part, dap = _nan_buf(n * 2, Nd), _nan_buf(2 * n * cb, 1)
                f = BnBwdFuse()
                f.x, f.part = fz["x"].data_ptr(), part.data_ptr()
                if mode != "bare":
                    f.scale, f.shift, f.mean, f.rstd = (fz[k].data_ptr() for k in ("scale", "shift", "mean", "rstd"))
                if mode != "bn_tanh":
                    f.alpha, f.dalpha_part = fz["alpha"].data_ptr(), dap.data_ptr()
            cvd.dgrad(dyd, wd, dx, accumulate=acc, fuse=f)
            what = f"dgrad {mode} acc={acc}"
            out.append((what, dx, rows_d, ldd, Nd))
            if mode:
                out.append((what + ": partials", part, n * 2, Nd, Nd))
                if mode != "bn_tanh":
                    out.append((what + ": slope pairs", dap, 2 * n * cb, 1, 1))
    return out


def _conv_pair(ops, case, pad_ld, code, pieces, up2=False):
    """The forward's and the data gradient's Conv of one geometry on one tile code (pad_ld: floats added to the OUTPUT's leading
    dimension of each pass)."""
    B, L, Cin, Cout, k, s, p, tr = case
    cvs = []
    for kind in ("fwd", "dgrad"):
        c_in_p, c_out_p = (Cin + 15) // 16 * 16, (Cout + 15) // 16 * 16
        cv = ops.Conv(B, L, Cin, Cout, k, s, p, 1, tr, pieces=pieces, up2=up2 and kind == "fwd",
                      ld_in=c_in_p + (pad_ld if kind == "dgrad" else 0), ld_out=c_out_p + (pad_ld if kind == "fwd" else 0))
        if pieces == 22 or up2:  # fp16 pieces exist for the forward only
            cv.dgrad_pieces = cv.wgrad_pieces = 2
        cv.__dict__["_tuned"] = {"fwd", "dgrad", "wgrad"}
        cv.desc.tile[0] = cv.desc.tile[1] = code
        cvs.append(cv)
    return cvs


def _off_on(ops, cvf, cvd, xd, dyd, wd, bd, fz, up2, what):
    """The launches with the switch off and on; None when the tile code does not exist for the geometry."""
    res = []
    try:
        for wide in (False, True):
            ops.set_epilogue_wide(wide)
            try:
                res.append(_launches(ops, cvf, cvd, xd, dyd, wd, bd, fz, up2))
            except RuntimeError as e:
                if "does not fit" in str(e) or "do not fit" in str(e):
                    return None
                raise
    finally:
        ops.set_epilogue_wide(True)
    for (name, a, rows, ld, width), (_, b, *_r) in zip(*res):
        _check_outside(b, rows, ld, width, f"{what} {name}")
        _same_bits(a, b, f"{what} {name}")
    return res[1]


def _old_f(cvf):
    """The values _launches accumulates the forward onto."""
    g = torch.Generator(device="cuda").manual_seed(5)
    return torch.randn(cvf.batch * cvf.l_out, cvf.c_out_p, generator=g, device="cuda")


def _fp64_checks(res, cvf, cvd, fz, case, pieces, y_ref, dx_ref):
    """Launches that take the 16-byte path (switch on; their epilogue reads) against torch fp64 under the bounds of
    test_split_gather_kernels.  An accumulating launch stores fl(conv + old): the old values are taken off in fp64, and the one
    fp32 rounding of the stored sum (half an ulp, <= 2^-24 |sum|) is added to the bound as 2^-23 max |sum| / max |ref|.  The fused
    launch's partials, summed over the row tiles, are held to fp64 sums of the kernel's own written gradient under the gates of
    conv_checks.bn_bwd_fused_check (2e-5 of the sum of magnitudes)."""
    B, L, Cin, Cout, k, s, p, tr = case
    named = {n: (buf, rows, ld, width) for n, buf, rows, ld, width in res}
    tol = K._SPLIT_TOL[pieces]
    yb, rows, ld, width = named["fwd accumulate"]
    tot = _rows_view(yb, rows, ld)[:, :width].double()
    got = K.from_nlc(tot - _old_f(cvf).double(), B, cvf.l_out, Cout)
    slack = 2.0 ** -23 * float(tot.abs().max()) / float(y_ref.abs().max())
    assert K.relerr(got, y_ref) < tol * math.sqrt(Cin * k) + tol + slack, "fwd accumulate (16-byte path) against fp64"
    tol = K._SPLIT_TOL[2] if pieces == 22 else tol
    db, rows, ld, width = named["dgrad None acc=True"]
    tot = _rows_view(db, rows, ld)[:, :width].double()
    got = K.from_nlc(tot - fz["old"].double(), B, L, Cin)
    slack = 2.0 ** -23 * float(tot.abs().max()) / float(dx_ref.abs().max())
    assert K.relerr(got, dx_ref) < tol * math.sqrt(Cout * k) + tol + slack, "dgrad accumulate (16-byte path) against fp64"
    db, rows, ld, width = named["dgrad bn_prelu acc=False"]
    dx = _rows_view(db, rows, ld)[:, :width].double()
    assert K.relerr(K.from_nlc(dx, B, L, Cin), dx_ref) < tol * math.sqrt(Cout * k) + tol, "fused dgrad (16-byte path) against fp64"
    pb, prow, pld, _ = named["dgrad bn_prelu acc=False: partials"]
    sums = _rows_view(pb, prow, pld).double().view(prow // 2, 2, pld).sum(0)
    xs = _rows_view(fz["x"].reshape(-1), rows, ld)[:, :width].double()
    u = xs * fz["scale"].double() + fz["shift"].double()
    du = torch.where(u > 0, dx, float(fz["alpha"]) * dx)
    xhat = (xs - fz["mean"].double()) * fz["rstd"].double()
    eb = ((sums[0] - du.sum(0)).abs() / (2e-5 * du.abs().sum(0)).clamp_min(1e-300)).max()
    eg = ((sums[1] - (du * xhat).sum(0)).abs() / (2e-5 * (du * xhat).abs().sum(0)).clamp_min(1e-300)).max()
    assert float(eb) <= 1 and float(eg) <= 1, ("fused partials (16-byte path) against fp64", float(eb), float(eg))


@pytest.fixture(scope="module")
def ops():
    from scrubvae_amd import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _ops


@pytest.mark.parametrize("case,pad_ld", CASES)
def test_wide_epilogue_same_bits(ops, case, pad_ld):
    B, L, Cin, Cout, k, s, p, tr = case
    x, w, b, dy, y_ref, dx_ref = K._gather_ref(case)
    wd = ops.conv_weight_to_tio(w.detach().float(), tr).cuda().contiguous()
    ran, checked = set(), set()
    for code, pieces in _pairs():
        cvf, cvd = _conv_pair(ops, case, pad_ld, code, pieces)
        ops.bump_weight_epoch()
        bd = torch.zeros(cvf.c_out_p)
        bd[:Cout] = b.float()
        bd = bd.cuda()
        fz = _fuse_inputs(B * L, cvd.c_in_p, cvd.desc.ld_in, seed=7)
        # the operands keep their plain leading dimension: each Conv pads the side it WRITES
        res = _off_on(ops, cvf, cvd, K.to_nlc(x), K.to_nlc(dy), wd, bd, fz, False, f"{case} code {code} pieces {pieces}")
        if res is None:
            continue
        fam = _family(code)
        ran.add(fam)
        if (fam, pieces) not in checked:  # once per family and piece count: the launches that RUN the 16-byte path against torch fp64
            checked.add((fam, pieces))
            _fp64_checks(res, cvf, cvd, fz, case, pieces, y_ref, dx_ref)
    assert ran == set(_WIDE_VARIANTS), f"families that ran: {ran}"


def test_wide_epilogue_same_bits_up2(ops):
    """The forward behind the fused x2 upsample (halo kernels 8 / 9 / 29): C, statistics and the by-product rows."""
    B, L, Cin, Cout = UP2_GEO
    k, pad = 6, 2
    case = (B, 2 * L, Cin, Cout, k, 1, pad, False)
    g = torch.Generator().manual_seed(17 + sum(UP2_GEO))
    xh = torch.randn(B, Cin, L, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, k, generator=g, dtype=torch.float64) / math.sqrt(Cin * k)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    y_ref = torch.nn.functional.conv1d(torch.nn.functional.interpolate(xh, scale_factor=2, mode="linear", align_corners=False), w, b,
                                       padding=pad)
    dy = torch.randn(y_ref.shape, generator=g, dtype=torch.float64)
    wd = ops.conv_weight_to_tio(w.float()).cuda().contiguous()
    bd = torch.zeros((Cout + 15) // 16 * 16)
    bd[:Cout] = b.float()
    bd = bd.cuda()
    ran = 0
    for code, pieces in _up2_pairs():
        cvf, cvd = _conv_pair(ops, case, 0, code, pieces, up2=True)
        if code == 0:
            cvd.desc.tile[1] = 8128128
        ops.bump_weight_epoch()
        fz = _fuse_inputs(B * 2 * L, cvd.c_in_p, cvd.desc.ld_in, seed=9)
        res = _off_on(ops, cvf, cvd, K.to_nlc(xh), K.to_nlc(dy), wd, bd, fz, True, f"up2 {UP2_GEO} code {code} pieces {pieces}")
        if res is None:
            continue
        ran += 1
        name, yb, rows, ld, width = res[1]  # the accumulating forward: it runs the 16-byte path
        assert name == "fwd accumulate"
        tot = _rows_view(yb, rows, ld)[:, :width].double()
        tol = K._SPLIT_TOL[pieces]
        slack = 2.0 ** -23 * float(tot.abs().max()) / float(y_ref.abs().max())  # the fp32 rounding of the stored sum (_fp64_checks)
        assert K.relerr(K.from_nlc(tot - _old_f(cvf).double(), B, cvf.l_out, Cout), y_ref) < tol * math.sqrt(Cin * k) + tol + slack
    assert ran >= 4


def test_wide_epilogue_unaligned_saved_input(ops):
    """A saved BatchNorm input that is only 4-byte aligned sends the launch down the dword path: same bits as the aligned launch."""
    case = (9, 4, 64, 48, 5, 2, 2, True)
    B, L, Cin, Cout, k, s, p, tr = case
    x, w, b, dy, _, _ = K._gather_ref(case)
    wd = ops.conv_weight_to_tio(w.detach().float(), tr).cuda().contiguous()
    _, cvd = _conv_pair(ops, case, 0, 8128128, 2)
    ops.bump_weight_epoch()
    fz = _fuse_inputs(B * L, cvd.c_in_p, cvd.desc.ld_in, seed=7)
    n, cb = cvd.dgrad_stats_tiles()
    shifted = torch.empty(fz["x"].numel() + 1, device="cuda")[1:]
    shifted.copy_(fz["x"].reshape(-1))
    assert shifted.data_ptr() % 16 == 4
    outs = []
    for xs in (fz["x"], shifted):
        dx, part, dap = _nan_buf(B * L, cvd.c_in_p), _nan_buf(n * 2, cvd.c_in_p), _nan_buf(2 * n * cb, 1)
        f = BnBwdFuse()
        f.x, f.part, f.alpha, f.dalpha_part = xs.data_ptr(), part.data_ptr(), fz["alpha"].data_ptr(), dap.data_ptr()
        f.scale, f.shift, f.mean, f.rstd = (fz[key].data_ptr() for key in ("scale", "shift", "mean", "rstd"))
        cvd.dgrad(K.to_nlc(dy), wd, dx, fuse=f)
        outs.append((dx, part, dap))
    for a, b_ in zip(*outs):
        _same_bits(a, b_, "dgrad with a 4-byte aligned saved input")
