"""How much of a variable the latents still carry, in nats: the k-nearest-neighbour estimate of mutual information on the device
(csrc/mi.hip).

    mutual_information(z, y, *, n_neighbors=3, return_parts=False)     the estimate, a float (not clipped at 0)
    mutual_information_permutation_test(z, y, *, n_neighbors=3, n_permutations=200, seed=0, permutations=None)
                                                                        MIPermutationResult(statistic, pvalue, null_distribution)
    latent_mi_scores(z, y, *, discrete_target=False, n_neighbors=3, random_state=None)
                                                                        [d] fp64: one estimate per latent dimension, clipped at 0

The decodability probes of metrics.py give the score of one decoder family and HSIC (independence.py) a p-value; neither says how
much information is left in units that compare across models, epochs and variables.  This is the standard estimator for that:
Kraskov-Stoegbauer-Grassberger (2004, algorithm 1) for a real y, Ross (2014) for labels, the two that sklearn ships as
mutual_info_regression / mutual_info_classif one feature at a time.

z is [n, d], numpy or torch, host or device, any float dtype; the rows go to fp64 uncentred, as for mmd_*.  y is read as hsic reads
it: a floating [n] or [n, q] with 1 <= q <= MI_MAX_Y = 4 selects KSG, an integer [n] selects Ross.  s^z_ij and s^y_ij are the
squared distances of csrc/pair_tiles.h (feature order, every subtract, multiply and add rounded on its own, no FMA); every
comparison is on s, by its bit pattern, never on a square root.  With k = n_neighbors <= MI_MAX_K = 32:

  real y    m_ij = max(s^z_ij, s^y_ij);  rho2_i = the k-th smallest m_ij over j != i (the row is left out by index, so a duplicate
            row counts at 0);  nz_i = #{j != i : s^z_ij < rho2_i},  ny_i = #{j != i : s^y_ij < rho2_i}, both strict;
            I = psi(n) + psi(k) - mean_i psi(nz_i + 1) - mean_i psi(ny_i + 1)
  labels    rows whose label occurs once are dropped on the host first (sklearn's _compute_mi_cd); n counts the kept rows.
            c_i = the size of row i's class, k_i = min(k, c_i - 1);  rho2_i = the k_i-th smallest s^z_ij over j != i with
            lab_j == lab_i;  nz_i = #{j != i : s^z_ij < rho2_i} over all labels;
            I = psi(n) + mean psi(k_i) - mean psi(c_i) - mean psi(nz_i + 1)

The strict < is sklearn's nextafter(radius, 0) followed by <=.  A row with rho2 = 0 (duplicates) counts 0 where sklearn counts the
duplicates: that case is defined here and no equality with sklearn is claimed on it.

psi on a positive integer m is one recipe on the device and on the host (psi_int): for m < 16, -0.5772156649015329 + (1/1 + 1/2
+ ... + 1/(m - 1)) added in ascending order; from 16 on, with x = m and t = 1 / (x x), log(x) - 0.5 / x - t (1/12 - t (1/120 -
t (1/252 - t (1/240 - t / 132)))); within 2 x 2^-53 x max(1, |psi|) of the digamma function.  The two means over the rows come
from the device as fixed-order compensated sums; the closing formula runs once on the host in fp64.  The label-side class terms
are summed per class in ascending class order, exactly rounded (math.fsum), so renumbering the labels changes no bit.

The estimator is biased downwards when d is large: with few rows per unit of volume the k-th neighbour is far away, nz and ny
approach n, and the estimate falls towards (and below) zero whatever the dependence.  Read it next to its permutation null
(mutual_information_permutation_test: the same estimator on shuffled y has the same bias) or one dimension at a time
(latent_mi_scores), not as an absolute number at d = 32.  Estimates are not clipped at 0 for that reason: the null needs them.

ValueError, before any device work: mismatched row counts, non-finite rows, n_neighbors not an integer in 1 .. min(n - 1,
MI_MAX_K), a real y wider than MI_MAX_Y, labels where fewer than two classes have at least two members, fewer than 3 rows after
the singleton drop, and the permutation errors of mmd_permutation_test.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _on_device
from ._inputs import _feature_rows, _is_int, _variable
from ._permutation import _given_or_count, _on_device_or_drawn, _pvalue

MI_MAX_K, MI_MAX_Y = _lib.MI_MAX_K, _lib.MI_MAX_Y   # the caps on n_neighbors and on the width of a real y
_MI_READ = 64                                       # permutations per read-back of the device sums
_MI_CALLS = {"radius": 0, "counts": 0, "psi_sums": 0}  # launches of the entry points by this process

_device_of = functools.partial(_device._device_of, who="mutual information runs on the GPU (csrc/mi.hip); no device is available")


class MIPermutationResult:
    """statistic (float), pvalue (float) and null_distribution (numpy [P] fp64): scipy's permutation_test names."""
    __slots__ = ("statistic", "pvalue", "null_distribution")

    def __init__(self, statistic, pvalue, null_distribution):
        self.statistic, self.pvalue, self.null_distribution = statistic, pvalue, null_distribution

    def __repr__(self):
        return (f"MIPermutationResult(statistic={self.statistic!r}, pvalue={self.pvalue!r}, "
                f"null_distribution=<{len(self.null_distribution)} values>)")


def psi_int(m):
    """psi (digamma) of the positive integers m, elementwise in fp64: the module docstring's recipe, which csrc/mi.hip repeats"""
    m = np.asarray(m)
    if m.size and m.min() < 1:
        raise ValueError("psi_int takes positive integers")
    out = np.empty(m.shape, np.float64)
    small = m < 16
    h = np.zeros(16)                              # h[m] = 1/1 + ... + 1/(m - 1), ascending
    for j in range(1, 15):
        h[j + 1] = h[j] + 1.0 / np.float64(j)
    out[small] = -0.5772156649015329 + h[m[small]]
    x = m[~small].astype(np.float64)
    t = 1.0 / (x * x)
    out[~small] = np.log(x) - 0.5 / x - t * (1.0 / 12.0 - t * (1.0 / 120.0 - t * (1.0 / 252.0 - t * (1.0 / 240.0 - t / 132.0))))
    return out


def mi_close_real(n, k, sum_z, sum_y):
    """I of KSG from the two device sums; fp64, elementwise over the sums"""
    n_ = np.float64(n)
    return ((psi_int(n) + psi_int(k)) - np.asarray(sum_z, np.float64) / n_) - np.asarray(sum_y, np.float64) / n_


def mi_class_terms(count, k):
    """(mean psi(k_i), mean psi(c_i)) over the rows from the class sizes count [K] >= 2, in ascending class order"""
    count = np.asarray(count, np.int64)
    n_ = np.float64(count.sum())
    kc = np.minimum(k, count - 1)
    mk = math.fsum(count.astype(np.float64) * psi_int(kc)) / n_
    mc = math.fsum(count.astype(np.float64) * psi_int(count)) / n_
    return mk, mc


def mi_close_labels(n, mk, mc, sum_z):
    """I of Ross from the class terms and the device sum; fp64, elementwise over the sum"""
    return ((psi_int(n) + mk) - mc) - np.asarray(sum_z, np.float64) / np.float64(n)


def _mi_neighbors(n_neighbors, n):
    if not _is_int(n_neighbors):
        raise ValueError(f"n_neighbors must be an integer, got {n_neighbors!r}")
    if not 1 <= n_neighbors <= min(n - 1, MI_MAX_K):
        raise ValueError(f"n_neighbors must lie in [1, min(n - 1, {MI_MAX_K})] with n = {n} rows, got {n_neighbors}")
    return int(n_neighbors)


def _mi_check(z, y, n_neighbors):
    """the argument errors, before any device work -> a dict: x (fp64 rows of z where they are, all of them), kind, n (kept rows),
    k, kept (bool [rows of z] numpy) and v (fp64 rows [n, q] where they are) or lab (int32 [n] in 0..K-1), count [K], kk [n]"""
    x = _feature_rows(z, "z")
    kind, v = _variable(y)
    rows = x.shape[0]
    if v.shape[0] != rows:
        raise ValueError(f"z and y must have one row count, got {rows} and {v.shape[0]}")
    if rows >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 rows are supported, got {rows}")
    if kind == "real":
        return dict(x=x, kind=kind, n=rows, k=_mi_neighbors(n_neighbors, rows), kept=np.ones(rows, bool), v=v)
    size = np.bincount(v)
    kept = size[v] > 1
    if int((size > 1).sum()) < 2:
        raise ValueError("labels y need at least two classes with at least two members")
    n = int(kept.sum())
    if n < 3:
        raise ValueError(f"the estimate needs at least 3 rows after the labels that occur once are dropped, got {n}")
    k = _mi_neighbors(n_neighbors, n)
    _, lab, count = np.unique(v[kept], return_inverse=True, return_counts=True)
    lab = np.ascontiguousarray(lab.reshape(-1), dtype=np.int32)
    kk = np.minimum(k, count - 1)[lab].astype(np.int32)
    return dict(x=x, kind=kind, n=n, k=k, kept=kept, lab=lab, count=count, kk=kk)


class _MiRun:
    """The device side of one (z, y): the buffers, and run(), which queues the three launches for one pairing."""

    def __init__(self, c, dev):
        """c = _mi_check(...)"""
        self.c, self.dev, self.lib, self.st = c, dev, _lib.lib(), ops._stream()
        n, k = c["n"], c["k"]
        Z = _on_device(c["x"], dev)
        if not c["kept"].all():
            Z = Z[torch.from_numpy(c["kept"]).to(dev)].contiguous()
        self.Z, self.n, self.k, self.ld = Z, n, k, Z.shape[1]
        self.real = c["kind"] == "real"
        if self.real:
            self.Y = _on_device(c["v"], dev)
            self.q = self.Y.shape[1]
            self.lab = self.kk = None
        else:
            self.Y, self.q = None, 1
            self.lab, self.kk = torch.from_numpy(c["lab"]).to(dev), torch.from_numpy(c["kk"]).to(dev)
        self.work = torch.empty((self.lib.svae_mi_work(n, k) + 7) // 8, dtype=torch.int64, device=dev)
        self.rho2 = torch.empty(n, dtype=torch.float64, device=dev)
        self.nz = torch.empty(n, dtype=torch.int32, device=dev)
        self.ny = torch.empty(n, dtype=torch.int32, device=dev) if self.real else None

    def run(self, out, perm=None, column=None):
        """rho2, nz, ny of the pairing (z_i, y[perm[i]]) into the buffers and the psi sums into out [2] (device).  perm: int64 [n]
        on the device, or None for the observed pairing.  column: take that column of z as the rows (d = 1, stride ld)."""
        lib, st, n, k = self.lib, self.st, self.n, self.k
        zp, d = (self.Z.data_ptr(), self.ld) if column is None else (self.Z.data_ptr() + 8 * column, 1)
        Y, lab, kk = self.Y, self.lab, self.kk
        if perm is not None:
            if self.real:
                Y = Y.index_select(0, perm)
            else:
                lab, kk = lab.index_select(0, perm), kk.index_select(0, perm)
        _MI_CALLS["radius"] += 1
        check(lib.svae_mi_radius(zp, self.ld, d, n, ops._p(Y), self.q, ops._p(lab), ops._p(kk), k, self.work.data_ptr(),
                                 self.rho2.data_ptr(), st), "mi_radius")
        _MI_CALLS["counts"] += 1
        check(lib.svae_mi_counts(zp, self.ld, d, n, ops._p(Y), self.q, self.rho2.data_ptr(), self.nz.data_ptr(), ops._p(self.ny), st),
              "mi_counts")
        _MI_CALLS["psi_sums"] += 1
        check(lib.svae_mi_psi_sums(self.nz.data_ptr(), ops._p(self.ny), n, out.data_ptr(), st), "mi_psi_sums")

    def close(self, sums):
        """I [...] from the device sums [..., 2] read back to numpy"""
        sums = np.asarray(sums, np.float64)
        if self.real:
            return mi_close_real(self.n, self.k, sums[..., 0], sums[..., 1])
        mk, mc = mi_class_terms(self.c["count"], self.k)
        return mi_close_labels(self.n, mk, mc, sums[..., 0])

    def parts(self):
        c = self.c
        p = dict(rho2=self.rho2.cpu().numpy(), nz=self.nz.cpu().numpy(), kept=c["kept"].copy())
        if self.real:
            p["ny"] = self.ny.cpu().numpy()
        else:
            p.update(k=c["kk"].copy(), count=c["count"][c["lab"]].astype(np.int32))
        return p


def mutual_information(z, y, *, n_neighbors=3, return_parts=False):
    """The kNN estimate of the mutual information of the rows of z [n, d] and y (real [n] / [n, q <= 4]: KSG; integer labels [n]:
    Ross), in nats, not clipped at 0.  return_parts=True: (I, dict) with rho2 [n] fp64, nz [n] int32 and ny [n] int32 (real y) or
    k [n], count [n] int32 (labels: each row's k_i and class size), over the kept rows, and kept, the bool mask over the rows of z
    that survived the drop of labels that occur once.  See the module docstring for the definitions."""
    c = _mi_check(z, y, n_neighbors)
    dev = _device_of(c["x"], c.get("v"))
    with torch.cuda.device(dev):
        run = _MiRun(c, dev)
        out = torch.zeros(2, dtype=torch.float64, device=dev)
        run.run(out)
        value = float(run.close(out.cpu().numpy()))
        return (value, run.parts()) if return_parts else value


def mutual_information_permutation_test(z, y, *, n_neighbors=3, n_permutations=200, seed=0, permutations=None):
    """Permutation test of the hypothesis that z and y are independent, with mutual_information(z, y, n_neighbors=...) as the
    statistic -> MIPermutationResult.

    statistic is mutual_information(z, y, n_neighbors=n_neighbors), bit for bit.  null_distribution[p] is the same estimate with
    y[permutations[p, i]] paired with z_i (for labels, k_i and c_i follow the label), a value that depends on its permutation row
    alone: an identity row reproduces the statistic bit for bit.  pvalue = (1 + #{p: null[p] >= statistic}) / (1 + P), compared
    in fp64.  The estimator's bias is the same under every pairing, so the comparison is fair where the number itself is not.

    permutations: [P, n] integers, numpy or torch, n the number of rows kept (all of them for a real y); every row must be a
    permutation of range(n) (ValueError otherwise).  When it is None, P = n_permutations rows are drawn by
    mmd_permutations(n, n_permutations, seed, device).  1 <= P <= MMD_MAX_PERMUTATIONS.  A host loop over the permutations of the
    three launches of mutual_information on a device-side gather of y; the sums are read back once per 64 permutations."""
    c = _mi_check(z, y, n_neighbors)
    n = c["n"]
    perms, P = _given_or_count(permutations, n_permutations, n)
    dev = _device_of(c["x"], c.get("v"))
    with torch.cuda.device(dev):
        perms = _on_device_or_drawn(perms, n, P, seed, dev)
        run = _MiRun(c, dev)
        out = torch.zeros(_MI_READ, 2, dtype=torch.float64, device=dev)
        run.run(out[0])
        statistic = float(run.close(out[0].cpu().numpy()))
        null = np.empty(P, np.float64)
        for p0 in range(0, P, _MI_READ):
            count = min(_MI_READ, P - p0)
            for p in range(count):
                run.run(out[p], perms[p0 + p])
            null[p0: p0 + count] = run.close(out[:count].cpu().numpy())
    return MIPermutationResult(statistic, _pvalue(statistic, null), null)


def mi_scores_inputs(z, y, discrete_target, random_state):
    """sklearn's preprocessing of mutual_info_regression / mutual_info_classif with all features continuous, on host fp64 arrays:
    every column of z over its population standard deviation (0 read as 1), plus 1e-10 max(1, mean |x|) standard_normal noise from
    RandomState(random_state); the same for a real y [n], drawn after z's."""
    x = np.array(z, dtype=np.float64)
    n, d = x.shape
    rng = np.random.RandomState(random_state)
    sd = x.std(axis=0)
    sd[sd == 0.0] = 1.0
    x /= sd
    means = np.maximum(1, np.mean(np.abs(x), axis=0))
    x += 1e-10 * means * rng.standard_normal(size=(n, d))
    if discrete_target:
        return x, y
    t = np.array(y, dtype=np.float64)
    sd = t.std()
    t /= 1.0 if sd == 0.0 else sd
    t += 1e-10 * np.maximum(1, np.mean(np.abs(t))) * rng.standard_normal(size=n)
    return x, t


def latent_mi_scores(z, y, *, discrete_target=False, n_neighbors=3, random_state=None):
    """One estimate per latent dimension, [d] fp64 numpy, each clipped at 0: sklearn's mutual_info_regression(z, y) (a real y [n])
    or mutual_info_classif(z, y) (discrete_target=True: integer labels [n]) with all features continuous, including their scaling
    and their 1e-10 noise from RandomState(random_state).  Column c is handed to the kernels as a view of the scaled z (row stride
    d, one feature), so nothing is copied per column."""
    x = _feature_rows(z, "z")
    kind, v = _variable(y)
    if (kind == "labels") != bool(discrete_target):
        raise ValueError(f"discrete_target={discrete_target!r} takes {'integer labels' if discrete_target else 'a floating y'}, got {kind}")
    if kind == "real" and v.shape[1] != 1:
        raise ValueError(f"latent_mi_scores takes one real target [n], got {v.shape[1]} columns")
    if v.shape[0] != x.shape[0]:
        raise ValueError(f"z and y must have one row count, got {x.shape[0]} and {v.shape[0]}")
    host = (lambda a: a.cpu().numpy() if torch.is_tensor(a) else a)
    xs, ys = mi_scores_inputs(host(x), host(v).reshape(-1), kind == "labels", random_state)
    c = _mi_check(xs, ys, n_neighbors)
    dev = _device_of(x, v)   # the given arrays, not their scaled host copies; labels are a host array
    with torch.cuda.device(dev):
        run = _MiRun(c, dev)
        d = xs.shape[1]
        out = torch.zeros(d, 2, dtype=torch.float64, device=dev)
        for col in range(d):
            run.run(out[col], column=col)
        return np.maximum(run.close(out.cpu().numpy()), 0.0)
