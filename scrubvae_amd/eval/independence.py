"""Kernel independence test of latents and a variable on the device: HSIC with a permutation null (csrc/hsic.hip).

    hsic_bandwidth(a)                                      the default bandwidth of a set of rows: the squared median distance
    hsic(z, y, *, hz=None, hy=None, estimator="biased")    the statistic, a float
    hsic_permutation_test(z, y, *, hz=None, hy=None, estimator="biased", n_permutations=1000, seed=0, permutations=None)
                                                           HSICPermutationResult(statistic, pvalue, null_distribution, hz, hy,
                                                           normalized)

The decodability probes of metrics.py each ask whether one family of decoders can predict a scrubbed variable from z.  The
Hilbert-Schmidt independence criterion (Gretton et al. 2008) is the model-free counterpart: it is zero (in the population, with
these kernels) exactly when z and y are independent, and the permutation test gives a p-value for that hypothesis.  It is the
dependence counterpart of mmd_permutation_test: that one asks whether two latent sets differ, this one whether the latents still
carry the variable.

z is [n, d], numpy or torch, host or device, any float dtype; the rows go to fp64 uncentred, as for mmd_*.  y is either
  - of a floating dtype, [n] or [n, q] with 1 <= q <= HSIC_MAX_Y = 4 (heading is 2 wide, avg_speed_3d is 3): the Gaussian kernel
    L_ij = exp(-|y_i - y_j|^2 / hy), or
  - of an integer dtype, [n] with at least two distinct values: the delta kernel L_ij = [y_i == y_j], no bandwidth.  Only equality
    of labels is read, so renumbering them changes no bit.
K_ij = exp(-|z_i - z_j|^2 / hz).  The squared distances are csrc/pair_tiles.h's (feature order, every operation rounded on its own);
hz and hy default to hsic_bandwidth of z and of y, the exact order statistic of csrc/mmd.hip on the one set.  With

    A = sum_{i<j} K_ij L_ij      k_i = sum_j K_ij, l_i = sum_j L_ij (diagonal included)      C = sum_ij K_ij, D = sum_ij L_ij

    estimator="biased":    (2 A + n) / n^2 - 2 sum_i k_i l_i / n^3 + C D / n^4  =  tr(K H L H) / n^2                      n >= 2
    estimator="unbiased":  [2 A + C~ D~ / ((n - 1)(n - 2)) - 2 sum_i k~_i l~_i / (n - 2)] / (n (n - 3))   (Song et al. 2012)   n >= 4
                           with k~ = k - 1, l~ = l - 1, C~ = C - n, D~ = D - n
    normalized:            HSIC_b(z, y) / sqrt(HSIC_b(z, z) HSIC_b(y, y)), the centred kernel alignment in 0..1: comparable
                           across epochs and models.  Always the biased form, of the observed pairing only.

Under permutation p the row y[permutations[p, i]] is paired with z_i: A and the middle sum change, everything else is constant.
The sums come from the device in a fixed order (bit-reproducible, no dependence on scheduling); the closing formulas run once, in
fp64 numpy on the host, for the statistic and every null value alike.  A null value depends on its permutation row alone, so
statistic == hsic(...) bit for bit, and an identity row reproduces the statistic bit for bit.  A zero bandwidth (median 0) gives nan
for the statistic, the p-value and the null, as in mmd_estimate.

ValueError, before any device work: mismatched row counts, n below the estimator's minimum, a non-positive or non-finite
bandwidth, an unknown estimator, y wider than HSIC_MAX_Y, hy given with labels, labels with one distinct value, non-finite rows,
and the permutation errors of mmd_permutation_test.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _clock, _on_device
from ._inputs import _feature_rows, _finite_rows, _is_number, _variable
from ._permutation import _given_or_count, _on_device_or_drawn, _pvalue

HSIC_MAX_Y = _lib.HSIC_MAX_Y      # the widest real y
HSIC_ESTIMATORS = {"biased": 2, "unbiased": 4}  # estimator -> the smallest n
_HSIC_LAUNCH = 256                # permutations per svae_hsic_cross launch: bounds the partials (26 MB at n = 10^5) and the int32 table
_HSIC_CALLS = {"select": 0, "moments": 0, "cross": 0, "dots": 0}  # launches of the entry points by this process

_device_of = functools.partial(_device._device_of, who="HSIC runs on the GPU (csrc/hsic.hip); no device is available")


class HSICPermutationResult:
    """statistic (float), pvalue (float), null_distribution (numpy [P] fp64), hz and hy (float; hy is None for labels) and
    normalized (float): scipy's permutation_test names."""
    __slots__ = ("statistic", "pvalue", "null_distribution", "hz", "hy", "normalized")

    def __init__(self, statistic, pvalue, null_distribution, hz, hy, normalized):
        self.statistic, self.pvalue, self.null_distribution = statistic, pvalue, null_distribution
        self.hz, self.hy, self.normalized = hz, hy, normalized

    def __repr__(self):
        return (f"HSICPermutationResult(statistic={self.statistic!r}, pvalue={self.pvalue!r}, "
                f"null_distribution=<{len(self.null_distribution)} values>, hz={self.hz!r}, hy={self.hy!r}, "
                f"normalized={self.normalized!r})")


def _hsic_bandwidth_arg(h, name):
    if h is not None and (not _is_number(h) or not h > 0):
        raise ValueError(f"{name} must be a finite positive number, got {h!r}")


def _hsic_check(z, y, hz, hy, estimator):
    """the argument errors of hsic*, before any device work -> (fp64 rows of z, kind, y as _variable gives it)"""
    if estimator not in HSIC_ESTIMATORS:
        raise ValueError(f"estimator must be one of {sorted(HSIC_ESTIMATORS)}, got {estimator!r}")
    x = _feature_rows(z, "z")
    kind, v = _variable(y)
    n = x.shape[0]
    if v.shape[0] != n:
        raise ValueError(f"z and y must have one row count, got {n} and {v.shape[0]}")
    if n < HSIC_ESTIMATORS[estimator]:
        raise ValueError(f"the {estimator} HSIC estimator needs at least {HSIC_ESTIMATORS[estimator]} rows, got {n}")
    _hsic_bandwidth_arg(hz, "hz")
    _hsic_bandwidth_arg(hy, "hy")
    if kind == "labels" and hy is not None:
        raise ValueError("hy belongs to a real y: the delta kernel on labels has no bandwidth")
    return x, kind, v


def _hsic_select(lib, rows, h, st):
    """hm = (med, h) on the device of rows [n, d]: the given bandwidth, or the squared median of the pairwise distances"""
    dev = rows.device
    hm = torch.full((2,), float("nan") if h is None else float(h), dtype=torch.float64, device=dev)
    if h is None:
        n, d = rows.shape
        work = torch.empty(_lib.MMD_WORK_WORDS, dtype=torch.int64, device=dev)
        _HSIC_CALLS["select"] += 1
        check(lib.svae_mmd_select(rows.data_ptr(), d, d, n, work.data_ptr(), hm.data_ptr(), st), "mmd_select")
    return hm


def hsic_biased(T, S, C, D, n):
    """tr(K H L H) / n^2 from T = tr(K L) = sum_ij K_ij L_ij, S = sum_i k_i l_i, C = sum K, D = sum L; fp64, elementwise"""
    n = np.float64(n)
    return (T / (n * n) - 2.0 * S / (n * n * n)) + C * D / (n * n * n * n)


def hsic_close(A, S, C, D, n, estimator):
    """The estimator from A = sum_{i<j} K_ij L_ij, S (sum_i k_i l_i for "biased", sum_i k~_i l~_i for "unbiased") and the totals
    C, D with the diagonal; fp64, elementwise over A and S: the one closing formula of the statistic and of every null value"""
    A, S = np.asarray(A, np.float64), np.asarray(S, np.float64)
    n = np.float64(n)
    if estimator == "biased":
        return hsic_biased(2.0 * A + n, S, C, D, n)
    Ct, Dt = C - n, D - n
    return ((2.0 * A + Ct * Dt / ((n - 1.0) * (n - 2.0))) - 2.0 * S / (n - 2.0)) / (n * (n - 3.0))


def _hsic_run(checked, hz, hy, estimator, perms=None, n_permutations=0, seed=0, info=None):
    """Everything on the device of z (or of y, or the current one) for checked = _hsic_check(...) -> a dict: values [1 + P] (the
    statistic, then the null), hz, hy, normalized and its parts num, den_z, den_y.  perms: what _given_or_count
    returned, None to draw n_permutations (0: none) by mmd_permutations.  info (a dict) receives synchronised host-clock times."""
    x, kind, v = checked
    n, d = x.shape
    P = n_permutations if perms is None else perms.shape[0]
    dev = _device_of(x, v)   # labels are a host array
    tilde = 1 if estimator == "unbiased" else 0
    with torch.cuda.device(dev):
        if P:
            perms = _on_device_or_drawn(perms, n, P, seed, dev)
        lib = _lib.lib()
        st = ops._stream()
        Z = _on_device(x, dev)
        clock = functools.partial(_clock, dev, info is not None)
        t0 = clock()
        hzm = _hsic_select(lib, Z, hz, st)
        if kind == "real":
            Y, lab, q = _on_device(v, dev), None, v.shape[1]
            hym = _hsic_select(lib, Y, hy, st)
            yp, lp, hyp = Y.data_ptr(), None, hym[1:].data_ptr()
        else:
            Y, lab, q, hym = None, torch.from_numpy(v).to(dev), 1, None
            yp, lp, hyp = None, lab.data_ptr(), None
        t1 = clock()
        work = torch.empty(lib.svae_hsic_work(n, max(1, min(P, _HSIC_LAUNCH))), dtype=torch.float64, device=dev)
        kz, ly = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
        mom = torch.empty(2, 3, dtype=torch.float64, device=dev)
        _HSIC_CALLS["moments"] += 2
        check(lib.svae_hsic_moments(Z.data_ptr(), d, d, None, n, hzm[1:].data_ptr(), work.data_ptr(), kz.data_ptr(), mom[0].data_ptr(), st),
              "hsic_moments")
        check(lib.svae_hsic_moments(yp, q, q, lp, n, hyp, work.data_ptr(), ly.data_ptr(), mom[1].data_ptr(), st), "hsic_moments")
        t2 = clock()
        # slot 0: the observed pairing (a null table is the identity); slots 1 .. P: the permutations.  S0b: the biased form's
        # middle sum of the observed pairing, which `normalized` takes whatever the estimator
        A, S = (torch.empty(1 + P, dtype=torch.float64, device=dev) for _ in range(2))
        S0b = torch.empty(1, dtype=torch.float64, device=dev)
        cross_s = dots_s = 0.0

        def launch(table, count, at):
            nonlocal cross_s, dots_s
            ta = clock()
            _HSIC_CALLS["cross"] += 1
            check(lib.svae_hsic_cross(Z.data_ptr(), d, d, n, hzm[1:].data_ptr(), yp, q, lp, hyp, table, count, work.data_ptr(),
                                      A[at:].data_ptr(), st), "hsic_cross")
            tb = clock()
            _HSIC_CALLS["dots"] += 1
            check(lib.svae_hsic_dots(kz.data_ptr(), ly.data_ptr(), n, table, count, tilde, S[at:].data_ptr(), st), "hsic_dots")
            cross_s, dots_s = cross_s + (tb - ta), dots_s + (clock() - tb)

        launch(None, 1, 0)
        _HSIC_CALLS["dots"] += 1
        check(lib.svae_hsic_dots(kz.data_ptr(), ly.data_ptr(), n, None, 1, 0, S0b.data_ptr(), st), "hsic_dots")
        for p0 in range(0, P, _HSIC_LAUNCH):
            count = min(_HSIC_LAUNCH, P - p0)
            table = perms[p0: p0 + count].to(torch.int32).contiguous()
            launch(table.data_ptr(), count, 1 + p0)
        if info is not None:
            info.update(select_s=t1 - t0, moments_s=t2 - t1, cross_s=cross_s, dots_s=dots_s)
        A, S, S0b, mom = A.cpu().numpy(), S.cpu().numpy(), float(S0b.cpu()[0]), mom.cpu().numpy()
        hzv = float(hzm.cpu()[1])
        hyv = None if hym is None else float(hym.cpu()[1])
    (C, K2, k2), (D, L2, l2) = mom[0], mom[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        values = hsic_close(A, S, C, D, n, estimator)
        num = hsic_biased(2.0 * A[0] + np.float64(n), S0b, C, D, n)
        den_z, den_y = hsic_biased(K2, k2, C, C, n), hsic_biased(L2, l2, D, D, n)
        normalized = num / np.sqrt(den_z * den_y)
    return dict(values=values, hz=hzv, hy=hyv, normalized=float(normalized), num=float(num), den_z=float(den_z), den_y=float(den_y))


def hsic_bandwidth(a):
    """The default bandwidth of the rows a ([n] or [n, q] of a floating dtype, n >= 2): np.median of the pairwise distances of
    the rows, squared -- exact, as mmd_bandwidth is for two sets."""
    if (torch.is_tensor(a) and a.dim() == 1) or (not torch.is_tensor(a) and np.ndim(a) == 1):
        a = a.reshape(-1, 1)
    x = _finite_rows(a, "a")
    if x.shape[0] < 2 or x.shape[1] < 1:
        raise ValueError(f"the bandwidth needs at least 2 rows of at least 1 feature, got shape {tuple(x.shape)}")
    dev = _device_of(x)
    with torch.cuda.device(dev):
        return float(_hsic_select(_lib.lib(), _on_device(x, dev), None, ops._stream()).cpu()[1])


def hsic(z, y, *, hz=None, hy=None, estimator="biased"):
    """The Hilbert-Schmidt independence criterion between the rows of z [n, d] and y (real [n] / [n, q], or integer labels [n]),
    Gaussian kernels with bandwidths hz and hy (default: hsic_bandwidth of each), the delta kernel on labels.  See the module
    docstring for the estimators."""
    return float(_hsic_run(_hsic_check(z, y, hz, hy, estimator), hz, hy, estimator)["values"][0])


def hsic_permutation_test(z, y, *, hz=None, hy=None, estimator="biased", n_permutations=1000, seed=0, permutations=None):
    """Permutation test of the hypothesis that z and y are independent, with hsic(z, y, ...) as the statistic (Gretton et al. 2008)
    -> HSICPermutationResult.

    statistic is hsic(z, y, hz=hz, hy=hy, estimator=estimator), bit for bit.  null_distribution[p] is the same estimator with
    y[permutations[p, i]] paired with z_i.  pvalue = (1 + #{p: null[p] >= statistic}) / (1 + P), compared in fp64.  The bandwidths
    belong to z and to y alone, so no permutation changes them.  normalized is the biased statistic of the observed pairing over
    sqrt(HSIC_b(z, z) HSIC_b(y, y)).

    permutations: [P, n] integers, numpy or torch; every row must be a permutation of range(n) (ValueError otherwise).  When it is
    None, P = n_permutations rows are drawn by mmd_permutations(n, n_permutations, seed, device): the result equals the call with
    those permutations bit for bit.  1 <= P <= MMD_MAX_PERMUTATIONS = 65 536."""
    checked = _hsic_check(z, y, hz, hy, estimator)
    perms, P = _given_or_count(permutations, n_permutations, checked[0].shape[0])
    r = _hsic_run(checked, hz, hy, estimator, perms, P, seed)
    statistic, null = float(r["values"][0]), np.ascontiguousarray(r["values"][1:])
    return HSICPermutationResult(statistic, _pvalue(statistic, null), null, r["hz"], r["hy"], r["normalized"])
