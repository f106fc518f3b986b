"""How much of a variable the latents still carry beyond what a third variable already tells, in nats: the k-nearest-neighbour
estimate of the conditional mutual information I(z; y | c) on the device, with a local permutation null (csrc/mi.hip).

    conditional_mutual_information(z, y, c, *, n_neighbors=3, return_parts=False)      the estimate, a float (not clipped at 0)
    conditional_permutations(c, n_permutations, *, n_donors=8, seed=0, device=None)    int64 [P, n] on the device: the local null
    conditional_mutual_information_permutation_test(z, y, c, *, n_neighbors=3, n_donors=8, n_permutations=200, seed=0,
                                                    permutations=None)                 MIPermutationResult

mutual_information(z, y) and its permutation null are unconditional, and the recordings are confounded: the class changes how fast
an animal moves, the animal id changes speed and heading statistics.  After speed has been scrubbed, "does z still tell the class
beyond what speed tells" is I(z; class | speed), and its test needs a null that keeps the dependence of z and of y on c: y is
shuffled only among rows with a similar c (Runge 2018, "CMIknn").

z is [n, d], numpy or torch, host or device, any float dtype; the rows go to fp64 uncentred.  y and c are each read as hsic reads
its variable: a floating [n] or [n, q] with 1 <= q <= 4 is real, an integer [n] holds labels.  s^z, s^y and s^c are the squared
distances of csrc/pair_tiles.h (feature order, no FMA), compared by their bit patterns, never through a square root; the row
itself is left out by index.  With k = n_neighbors <= MI_MAX_K = 32:

  real y, real c    (Frenzel and Pompe 2007)  rho2_i = the k-th smallest max(s^z_ij, s^y_ij, s^c_ij) over j != i;
                    nzc_i = #{max(s^z_ij, s^c_ij) < rho2_i}, nyc_i = #{max(s^y_ij, s^c_ij) < rho2_i}, nc_i = #{s^c_ij < rho2_i},
                    all strict;  I = ((psi(k) + mean psi(nc_i + 1)) - mean psi(nzc_i + 1)) - mean psi(nyc_i + 1)
  real y, label c   (stratified)  rows whose class has at most k members are dropped first; n counts the kept rows.
                    rho2_i = the k-th smallest max(s^z_ij, s^y_ij) over the j != i of row i's class; nzc_i and nyc_i count s^z
                    and s^y below rho2_i inside the class; nc_i + 1 is the class size.  The same closing formula: the
                    class-weighted mean of the KSG estimate inside every class.
  label y, real c   (chain rule)  I([z, c]; y) - I(c; y), two estimates of mutual_information's label form (Ross 2014) on the
                    rows [z, c] (z's features first) and c.  The rows are compared in Euclidean distance, so the scale of c
                    against z is the caller's choice.
  label y, label c  not built: ValueError.

psi is psi_int of mutual_info.py; the three means come from the device as fixed-order compensated sums (the class-size term of a
label c is summed per class in ascending class order with math.fsum) and the closing formula runs once on the host in fp64.  A
row with rho2 = 0 (duplicates) counts 0.  Like the unconditional estimate this one is biased when d is large: read it next to its
null.

The local null.  Under a permutation row, y[perm[i]] is paired with (z_i, c_i).  For labels c the draw is a uniformly random
permutation inside every class.  For a real c every row has n_donors donors, itself and its n_donors - 1 nearest other rows in c
(svae_knn); the rows are visited in a random order, each takes its first unused donor in a random scan order and, when all are
used, the last one tried (a donor can then serve twice: a row of the result need not be a permutation).  With a label y such a
map changes the class sizes, so the chain-rule null takes the class sizes, every row's k_i and the drop of labels that occur once
from y[map], map by map: each null value is the plain estimate of (z, y[map], c).

ValueError, before any launch of this module (a given `permutations` that is a device tensor is range-checked where it lives):
mismatched row counts, non-finite rows, widths above the caps, n_neighbors not an integer in 1 .. min(n - 1, MI_MAX_K), labels for
both y and c, no class of a label c with more than k rows or fewer than 3 rows kept, n_donors outside 2 .. min(n,
CMI_MAX_DONORS), more than 2^19 rows in a local draw, a given permutation entry outside [0, n), and the permutation-argument
errors of mmd_permutation_test.  With a label y, an index map (given or drawn) under which y[map] has fewer than two classes of
two members, fewer than 3 rows in them or no more than n_neighbors is a ValueError before the first pairing is queued.
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
from ._permutation import _count, _given_or_count, _pvalue, mmd_permutations
from .mutual_info import _MI_CALLS, MIPermutationResult, _mi_check, _mi_neighbors, _MiRun, mi_class_terms, mi_close_labels, psi_int

CMI_MAX_C, CMI_MAX_DONORS = _lib.CMI_MAX_C, _lib.CMI_MAX_DONORS   # the caps on the width of a real c and on n_donors
CMI_MAX_LOCAL_ROWS = 2 ** 19                                      # rows of a local draw: the used-bitmap of svae_local_permutations
_CMI_READ = 64                                                    # permutations per read-back of the device sums and per local draw
_CMI_SCAN = 2 ** 25                                               # entries of `scan` drawn at once: its sort holds 13 bytes per entry
# pairings handed to svae_cmi_radius / svae_cmi_counts / the psi sums (svae_mi_psi_sums, twice per pairing with a real c) and
# calls of svae_local_permutations by this process
_CMI_CALLS = {"radius": 0, "counts": 0, "psi_sums": 0, "local_permutations": 0}

_device_of = functools.partial(_device._device_of, who="conditional mutual information runs on the GPU (csrc/mi.hip); no device is available")


def cmi_close(n, k, term_c, sum_zc, sum_yc):
    """I from term_c = mean psi(nc_i + 1) and the two device sums; fp64, elementwise over the sums"""
    n_ = np.float64(n)
    return ((psi_int(k) + np.asarray(term_c, np.float64)) - np.asarray(sum_zc, np.float64) / n_) - np.asarray(sum_yc, np.float64) / n_


def cmi_class_term(count):
    """mean psi(class size) over the rows from the class sizes count [K], in ascending class order, exactly rounded"""
    count = np.asarray(count, np.int64)
    return math.fsum(count.astype(np.float64) * psi_int(count)) / np.float64(count.sum())


def _cmi_condition(c):
    kind, w = _variable(c)
    if kind == "real" and w.shape[1] > CMI_MAX_C:
        raise ValueError(f"real c must be [n] or [n, p] with 1 <= p <= {CMI_MAX_C}, got p = {w.shape[1]}")
    return kind, w


def _cmi_check(z, y, c, n_neighbors):
    """the argument errors, before any device work -> a dict.  kind "real": x, v, w (fp64 rows of z, y, c where they are, all of
    them), n, k, kept (all True).  kind "strat": x, v, lab (int32 [n] in 0..K-1 over the kept rows), count [K], n (kept rows), k,
    kept (bool over the given rows).  kind "chain": joint, marginal (the checked arguments of the two label estimates), w, n, k,
    kept."""
    x = _feature_rows(z, "z")
    ykind, v = _variable(y)
    ckind, w = _cmi_condition(c)
    rows = x.shape[0]
    if v.shape[0] != rows or w.shape[0] != rows:
        raise ValueError(f"z, y and c must have one row count, got {rows}, {v.shape[0]} and {w.shape[0]}")
    if rows >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 rows are supported, got {rows}")
    if ykind == "labels":
        if ckind == "labels":
            raise ValueError("labels for both y and c are not supported: give one of them as a real variable")
        if torch.is_tensor(x) or torch.is_tensor(w):   # the rows [z, c] where z is (where c is, for a host z)
            home = x.device if torch.is_tensor(x) else w.device
            xc = torch.cat([_on_device(x, home), _on_device(w, home)], dim=1)
        else:
            xc = np.concatenate([x, w], axis=1)
        joint, marginal = _mi_check(xc, y, n_neighbors), _mi_check(w, y, n_neighbors)
        return dict(kind="chain", joint=joint, marginal=marginal, x=xc, w=w, n=joint["n"], k=joint["k"], kept=joint["kept"])
    k = _mi_neighbors(n_neighbors, rows)
    if ckind == "real":
        return dict(kind="real", x=x, v=v, w=w, n=rows, k=k, kept=np.ones(rows, bool))
    size = np.bincount(w)
    kept = size[w] > k
    n = int(kept.sum())
    if n == 0:
        raise ValueError(f"no class of c has more than n_neighbors = {k} rows")
    if n < 3:
        raise ValueError(f"the estimate needs at least 3 rows after the classes of at most {k} rows are dropped, got {n}")
    _, lab, count = np.unique(w[kept], return_inverse=True, return_counts=True)
    return dict(kind="strat", x=x, v=v, lab=np.ascontiguousarray(lab.reshape(-1), dtype=np.int32), count=count, n=n, k=k, kept=kept)


def _kept_rows(a, kept, dev):
    t = _on_device(a, dev)
    return t if kept.all() else t[torch.from_numpy(kept).to(dev)].contiguous()


class _CmiRun:
    """The device side of one (z, y, c) with a real y: the buffers, and run(), which queues the launches for one pairing."""
    SUMS = 3   # doubles of `out` per pairing

    def __init__(self, c, dev):
        """c = _cmi_check(...) of kind "real" or "strat" """
        self.c, self.dev, self.lib, self.st = c, dev, _lib.lib(), ops._stream()
        n, k, kept = c["n"], c["k"], c["kept"]
        self.n, self.k = n, k
        self.Z, self.Y = _kept_rows(c["x"], kept, dev), _kept_rows(c["v"], kept, dev)
        self.ld, self.q = self.Z.shape[1], self.Y.shape[1]
        self.real = c["kind"] == "real"
        new = functools.partial(torch.empty, n, dtype=torch.int32, device=dev)
        if self.real:
            self.C, self.clab, self.nc = _on_device(c["w"], dev), None, new()
            self.p = self.C.shape[1]
        else:
            self.C, self.clab, self.nc, self.p = None, torch.from_numpy(c["lab"]).to(dev), None, 1
            self.term_c = cmi_class_term(c["count"])
        self.work = torch.empty((self.lib.svae_mi_work(n, k) + 7) // 8, dtype=torch.int64, device=dev)
        self.rho2 = torch.empty(n, dtype=torch.float64, device=dev)
        self.nzc, self.nyc = new(), new()

    def maps(self, perms):
        """the index maps int64 [P, n] on the device as run() takes their rows"""
        return perms

    def run(self, out, perm=None):
        """rho2 and the counts of the pairing ((z_i, c_i), y[perm[i]]) into the buffers and the psi sums of nzc, nyc and (real c)
        nc into out [3] (device).  perm: int64 [n] on the device, or None for the observed pairing."""
        lib, st, n = self.lib, self.st, self.n
        Y = self.Y if perm is None else self.Y.index_select(0, perm)
        rows = (self.Z.data_ptr(), self.ld, self.ld, n, Y.data_ptr(), self.q, ops._p(self.C), self.p, ops._p(self.clab))
        _CMI_CALLS["radius"] += 1
        check(lib.svae_cmi_radius(*rows, self.k, self.work.data_ptr(), self.rho2.data_ptr(), st), "cmi_radius")
        _CMI_CALLS["counts"] += 1
        check(lib.svae_cmi_counts(*rows, self.rho2.data_ptr(), self.nzc.data_ptr(), self.nyc.data_ptr(), ops._p(self.nc), st), "cmi_counts")
        _CMI_CALLS["psi_sums"] += 1
        check(lib.svae_mi_psi_sums(self.nzc.data_ptr(), self.nyc.data_ptr(), n, out.data_ptr(), st), "mi_psi_sums")
        if self.real:
            check(lib.svae_mi_psi_sums(self.nc.data_ptr(), None, n, out[2:].data_ptr(), st), "mi_psi_sums")

    def close(self, sums):
        """I [...] from the device sums [..., 3] read back to numpy"""
        sums = np.asarray(sums, np.float64)
        term_c = sums[..., 2] / np.float64(self.n) if self.real else self.term_c
        return cmi_close(self.n, self.k, term_c, sums[..., 0], sums[..., 1])

    def parts(self):
        p = dict(rho2=self.rho2.cpu().numpy(), nzc=self.nzc.cpu().numpy(), nyc=self.nyc.cpu().numpy(), kept=self.c["kept"].copy())
        p["nc"] = self.nc.cpu().numpy() if self.real else (self.c["count"][self.c["lab"]] - 1).astype(np.int32)
        return p


class _ChainRun:
    """Label y against a real c: the two label estimates of mutual_info.py, I([z, c]; y) and I(c; y), under one pairing.  Under an
    index map the class sizes, every row's k_i and the rows dropped because their label occurs once are those of y[map], so the
    value is conditional_mutual_information(z, y[map], c) whether or not the map is a permutation."""
    SUMS = 4

    def __init__(self, c, dev):
        self.c, self.dev, self.n, self.k = c, dev, c["n"], c["k"]
        self.joint, self.marginal = _MiRun(c["joint"], dev), _MiRun(c["marginal"], dev)
        self.terms = []   # (n, mean psi(k_i), mean psi(c_i)) of the pairings queued since the last close()

    def maps(self, perms):
        """the index maps on the host, where the class sizes under a map are counted; a map that leaves y too few rows is a
        ValueError here, before the first pairing is queued"""
        perms = perms.cpu().numpy()
        for perm in perms:
            self._pairing(perm)
        return perms

    def _pairing(self, perm):
        """the labels y[perm] as _mi_check reads labels -> (keep bool [n], lab, kk int32 [kept], count [classes kept])"""
        lab, k = self.c["joint"]["lab"][perm], self.k
        size = np.bincount(lab)
        keep = size[lab] > 1
        n = int(keep.sum())
        if int((size > 1).sum()) < 2 or n < 3 or k > n - 1:
            raise ValueError(f"an index map leaves y too few rows for n_neighbors = {k}: {int((size > 1).sum())} classes with at least "
                             f"two members, {n} rows in them")
        lab = np.ascontiguousarray(lab[keep], dtype=np.int32)
        return keep, lab, np.minimum(k, size - 1)[lab].astype(np.int32), size[size > 1]

    def _launch(self, m, keep, rows, lab, kk, out):
        """the three launches of _MiRun.run for the rows `keep` of m under the labels lab and their kk (device int32 [n kept])"""
        Z, n, work = m.Z, m.n, m.work
        if not keep.all():   # fewer rows: a workspace of its own, because svae_mi_work(n, k) does not grow with n everywhere
            Z, n = m.Z.index_select(0, rows), lab.shape[0]
            work = torch.empty((m.lib.svae_mi_work(n, m.k) + 7) // 8, dtype=torch.int64, device=self.dev)
        _MI_CALLS["radius"] += 1
        check(m.lib.svae_mi_radius(Z.data_ptr(), m.ld, m.ld, n, None, 1, lab.data_ptr(), kk.data_ptr(), m.k, work.data_ptr(),
                                   m.rho2.data_ptr(), m.st), "mi_radius")
        _MI_CALLS["counts"] += 1
        check(m.lib.svae_mi_counts(Z.data_ptr(), m.ld, m.ld, n, None, 1, m.rho2.data_ptr(), m.nz.data_ptr(), None, m.st), "mi_counts")
        _MI_CALLS["psi_sums"] += 1
        check(m.lib.svae_mi_psi_sums(m.nz.data_ptr(), None, n, out.data_ptr(), m.st), "mi_psi_sums")

    def run(self, out, perm=None):
        """perm: int64 [n] numpy (a row of maps()), or None for the observed pairing"""
        if perm is None:
            self.terms.append((self.n,) + mi_class_terms(self.c["joint"]["count"], self.k))
            self.joint.run(out[:2])
            self.marginal.run(out[2:])
            return
        keep, lab, kk, count = self._pairing(perm)
        self.terms.append((int(count.sum()),) + mi_class_terms(count, self.k))
        rows = None if keep.all() else torch.from_numpy(np.flatnonzero(keep)).to(self.dev)
        lab, kk = torch.from_numpy(lab).to(self.dev), torch.from_numpy(kk).to(self.dev)
        self._launch(self.joint, keep, rows, lab, kk, out[:2])
        self._launch(self.marginal, keep, rows, lab, kk, out[2:])

    def close(self, sums):
        """I [...] from the device sums [..., 4] of the pairings queued since the last close(), in their order"""
        sums = np.asarray(sums, np.float64)
        terms, self.terms = self.terms, []
        flat = sums.reshape(-1, self.SUMS)
        assert len(terms) == len(flat)
        # one pairing at a time with scalars, so that a value does not depend on what it is batched with
        both = [(mi_close_labels(n, mk, mc, s[0]), mi_close_labels(n, mk, mc, s[2])) for (n, mk, mc), s in zip(terms, flat)]
        self.values = both[-1]
        return np.array([j - m for j, m in both], np.float64).reshape(sums.shape[:-1])

    def parts(self):
        return dict(joint=float(self.values[0]), marginal=float(self.values[1]), kept=self.c["kept"].copy())


def _cmi_run(c, dev):
    return _ChainRun(c, dev) if c["kind"] == "chain" else _CmiRun(c, dev)


def conditional_mutual_information(z, y, c, *, n_neighbors=3, return_parts=False):
    """The kNN estimate of the conditional mutual information I(z; y | c) of the rows of z [n, d], y and c, in nats, not clipped at
    0.  y and c are each real ([n] / [n, q <= 4]) or integer labels [n]:

      real y, real c    Frenzel and Pompe (2007).  Parts: rho2 [n] fp64 and nzc, nyc, nc [n] int32.
      real y, label c   the class-weighted mean of the KSG estimate inside every class of c; rows whose class has at most
                        n_neighbors members are dropped first.  Parts as above over the kept rows (nc + 1 is the class size).
      label y, real c   the chain rule I([z, c]; y) - I(c; y) with mutual_information's label estimate on the rows [z, c] (z's
                        features first) and on c.  The rows [z, c] are compared in Euclidean distance, so the scale of c against z
                        is the caller's choice (standardise both, or weight c, before the call).  Parts: the two values, joint
                        and marginal.
      label y, label c  ValueError: not built.

    return_parts=True: (I, dict) with those parts and kept, the bool mask over the given rows that entered the estimate.  See the
    module docstring for the definitions."""
    c_ = _cmi_check(z, y, c, n_neighbors)
    dev = _device_of(c_.get("x"), c_.get("v"), c_.get("w"))
    with torch.cuda.device(dev):
        run = _cmi_run(c_, dev)
        out = torch.zeros(run.SUMS, dtype=torch.float64, device=dev)
        run.run(out)
        value = float(run.close(out.cpu().numpy()))
        return (value, run.parts()) if return_parts else value


def _donor_count(n_donors, n):
    if not _is_int(n_donors):
        raise ValueError(f"n_donors must be an integer, got {n_donors!r}")
    if not 2 <= n_donors <= min(n, CMI_MAX_DONORS):
        raise ValueError(f"n_donors must lie in [2, min(n, {CMI_MAX_DONORS})] with n = {n} rows, got {n_donors}")
    if n > CMI_MAX_LOCAL_ROWS:
        raise ValueError(f"a local draw takes at most 2^19 rows, got {n}")
    return int(n_donors)


def _local_donors(C, kp):
    """nbr int32 [n, kp] on the device of C [n, p] (contiguous fp64): the row itself, then its kp - 1 nearest other rows"""
    from .neighbors import _knn_device
    n = C.shape[0]
    own = torch.arange(n, dtype=torch.int32, device=C.device).view(n, 1)
    if kp == 1:
        return own
    return torch.cat([own, _knn_device(C, kp - 1, None)[1]], dim=1).contiguous()


def _local_draw(nbr, order, scan):
    """svae_local_permutations on device tensors nbr int32 [n, kp], order int32 [P, n], scan uint8 [P, n, kp] -> int32 [P, n]"""
    (n, kp), P = nbr.shape, order.shape[0]
    out = torch.empty(P, n, dtype=torch.int32, device=nbr.device)
    _CMI_CALLS["local_permutations"] += 1
    check(_lib.lib().svae_local_permutations(nbr.data_ptr(), n, kp, order.data_ptr(), scan.data_ptr(), P, out.data_ptr(), ops._stream()),
          "local_permutations")
    return out


def _local_chunk(n, kp):
    """permutations per launch of the local draw: at most 64, and fewer where n * kp is large.  scan [count, n, kp] is the argsort
    of fp32 keys, which holds the keys and int64 indices next to the uint8 result, 13 bytes per entry and the sort's own workspace:
    at most _CMI_SCAN entries at once keeps that under 1 GiB (one permutation per launch at n = 2^19 and 64 donors)."""
    return max(1, min(_CMI_READ, _CMI_SCAN // (n * kp)))


def _local_inputs(n, kp, P, seed, dev):
    """(order int64 [P, n], a function p0, count -> scan uint8 [count, n, kp] to be called with ascending chunks): the random
    inputs of the local draw"""
    order = mmd_permutations(n, P, seed, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed) + 1)
    return order, lambda count: torch.rand(count, n, kp, generator=g, device=dev).argsort(dim=2).to(torch.uint8)


def _conditional_permutations(kind, w, P, n_donors, seed, dev):
    """kind, w: c as _variable gives it (the kept rows); checked arguments"""
    with torch.cuda.device(dev):
        if kind == "labels":
            lab = (torch.from_numpy(w) if not torch.is_tensor(w) else w).to(dev)
            g = torch.Generator(device=dev)
            g.manual_seed(int(seed))
            # inside every class a uniformly random order: the rows sorted by (label, uniform key) against the rows sorted by label.
            # The key is sorted in two stable steps, not as label + U, which can round up to the next label.
            drawn = torch.rand(P, lab.shape[0], generator=g, device=dev).argsort(dim=1)
            shuffled = drawn.gather(1, lab.to(torch.int64)[drawn].argsort(dim=1, stable=True))
            sorted_ = lab.argsort(stable=True)
            out = torch.empty_like(shuffled)
            out.scatter_(1, sorted_.view(1, -1).expand(P, -1), shuffled)
            return out
        C = _on_device(w, dev)
        n = C.shape[0]
        nbr = _local_donors(C, n_donors)
        order, scan_of = _local_inputs(n, n_donors, P, seed, dev)
        out = torch.empty(P, n, dtype=torch.int64, device=dev)
        chunk = _local_chunk(n, n_donors)
        for p0 in range(0, P, chunk):
            count = min(chunk, P - p0)
            out[p0: p0 + count] = _local_draw(nbr, order[p0: p0 + count].to(torch.int32).contiguous(), scan_of(count).contiguous())
        return out


def conditional_permutations(c, n_permutations, *, n_donors=8, seed=0, device=None):
    """The local null of the conditional test: int64 [n_permutations, n] on the device; row p maps every row i to the row whose y
    it receives, which has a c like c_i.

    Labels c (integer [n]): a uniformly random permutation inside every class, the rows ordered by (label, U[0, 1) key) with the
    keys from a torch.Generator seeded with `seed`; every result row is a permutation of range(n).
    Real c ([n] / [n, p <= 4]): the donors of row i are i itself and its n_donors - 1 nearest other rows in c (svae_knn).  The
    rows are visited in the order mmd_permutations(n, P, seed, device)[p]; each takes the first unused donor in its own scan order
    (the argsort of uniform keys from a generator seeded with seed + 1) and, when every donor is used, the last one scanned (Runge
    2018), so a donor can serve twice.  Drawn by svae_local_permutations, 64 permutations per launch, fewer where n * n_donors
    exceeds 2^19 so that the scan orders of one launch stay under 2^25 entries (_local_chunk).
    2 <= n_donors <= min(n, CMI_MAX_DONORS) and n <= 2^19 for a real c (ValueError otherwise); n_donors is not read for labels."""
    kind, w = _cmi_condition(c)
    P = _count(n_permutations)
    if kind == "real":
        _donor_count(n_donors, w.shape[0])
    dev = torch.device(device) if device is not None else _device_of(w)
    return _conditional_permutations(kind, w, P, n_donors, seed, dev)


def _cmi_given_permutations(t, n):
    """the further error of a given `permutations` that passed _given_or_count, where it lives: an entry outside [0, n)"""
    if int(t.min()) < 0 or int(t.max()) >= n:
        raise ValueError(f"permutations must hold row indices in [0, {n})")
    return t


def conditional_mutual_information_permutation_test(z, y, c, *, n_neighbors=3, n_donors=8, n_permutations=200, seed=0, permutations=None):
    """Local permutation test of the hypothesis that z and y are independent given c, with
    conditional_mutual_information(z, y, c, n_neighbors=...) as the statistic -> MIPermutationResult.

    statistic is that call's value, bit for bit.  null_distribution[p] is the same estimate with y[permutations[p, i]] paired with
    (z_i, c_i), a value that depends on its permutation row alone: an identity row reproduces the statistic bit for bit.
    pvalue = (1 + #{p: null[p] >= statistic}) / (1 + P), compared in fp64.

    permutations: [P, n] integers in [0, n), numpy or torch, n the number of rows kept (with a label c the rows of classes with at
    most n_neighbors members are dropped before anything is drawn; with a label y, the rows whose label occurs once).  A row need
    not be a permutation, because local draws repeat donors; an entry out of range is a ValueError.  With a label y a map that
    repeats rows changes the class sizes: the class sizes, every row's k_i and the rows dropped because their label occurs once
    are then those of y[map], counted on the host for every map, so that null_distribution[p] is
    conditional_mutual_information(z[kept], y[kept][map], c[kept]); a map that leaves fewer than two classes with two members, fewer
    than 3 rows or no more than n_neighbors rows is a ValueError, raised before the first pairing is queued.  When it is None,
    P = n_permutations rows are drawn by conditional_permutations(c[kept], n_permutations, n_donors=n_donors, seed=seed).
    1 <= P <= MMD_MAX_PERMUTATIONS.  A host loop over the permutations on a device-side gather of y; the sums are read back once
    per 64 permutations."""
    c_ = _cmi_check(z, y, c, n_neighbors)
    n = c_["n"]
    perms, P = _given_or_count(permutations, n_permutations, n)
    if perms is not None:
        _cmi_given_permutations(perms, n)
    elif c_["kind"] != "strat":
        _donor_count(n_donors, n)
    dev = _device_of(c_.get("x"), c_.get("v"), c_.get("w"))
    with torch.cuda.device(dev):
        if perms is not None:
            perms = perms.to(device=dev, dtype=torch.int64)
        elif c_["kind"] == "strat":
            perms = _conditional_permutations("labels", c_["lab"], P, n_donors, seed, dev)
        else:
            perms = _conditional_permutations("real", _kept_rows(c_["w"], c_["kept"], dev), P, n_donors, seed, dev)
        run = _cmi_run(c_, dev)
        perms = run.maps(perms)
        out = torch.zeros(_CMI_READ, run.SUMS, dtype=torch.float64, device=dev)
        run.run(out[0])
        statistic = float(run.close(out[0].cpu().numpy()))
        null = np.empty(P, np.float64)
        for p0 in range(0, P, _CMI_READ):
            count = min(_CMI_READ, P - p0)
            for p in range(count):
                run.run(out[p], perms[p0 + p])
            null[p0: p0 + count] = run.close(out[:count].cpu().numpy())
    return MIPermutationResult(statistic, _pvalue(statistic, null), null)
