"""Silhouette of a clustering of latents, exact over all rows, on the device (csrc/silhouette.hip).

    silhouette_samples(z, labels, *, noise_label=None, return_parts=False)   s [n] float64 numpy; with return_parts=True the
                                                                             namedtuple SilhouetteParts(s, a, b, nearest)
    silhouette_score(z, labels, *, noise_label=None)                         the mean of s, a float
    cluster_silhouette(z, labels, *, noise_label=None)                       (cluster_labels [K], mean s per cluster [K], sizes [K])
    cluster_medoids(z, labels, *, noise_label=None)                          (cluster_labels [K], row_index [K] int64)

z is [n, d], numpy or torch, host or device, any float dtype; the rows go to fp64 uncentred, as for mmd_*.  labels is [n], any
integer dtype, numpy or torch; every distinct value is a cluster, in np.unique order -- including -1, exactly as sklearn treats
it.  The labels are read on the host and mapped to 0..K-1 (the class set is a host decision, as for the decodability metrics).

With S[i, c] = the sum over the rows j of cluster c of the Euclidean distance dist(i, j), and m_c the size of cluster c:

    a_i = S[i, own] / (m_own - 1)                     mean distance to the other rows of the row's own cluster
    b_i = min over c != own of S[i, c] / m_c          mean distance to the rows of the nearest other cluster
    nearest_i = the label of that c                   on an exact tie the lowest c
    s_i = (b_i - a_i) / max(a_i, b_i)

What matches sklearn.metrics.silhouette_samples / silhouette_score (metric="euclidean"): these definitions, s_i = 0 for a row
alone in its cluster, s_i = 0 where max(a_i, b_i) == 0 (sklearn's nan_to_num), and the condition 2 <= K <= n - 1 on the number of
clusters.  The distances are scipy's cdist arithmetic (csrc/pair_tiles.h); the sums are taken in a different order from sklearn's,
in fp64, so s agrees with sklearn to a few units of roundoff of (a_i + b_i) / max(a_i, b_i).  Every result is bit-reproducible and
does not depend on how the clusters are numbered.  Nothing of size n^2 is stored: one pass over all n^2 distances per 256 clusters,
each 64 x 64 tile of distances multiplied with the 0 / 1 membership columns on the fp64 matrix cores.

Differences from sklearn, by design:
  - sample_size / random_state and metrics other than Euclidean are not supported: the point is that no subsample is needed.
  - noise_label=v leaves the rows labelled v out of every sum (HDBSCAN's -1): they get s = a = b = nan and nearest = v, and the
    score, the per-cluster means and the medoids are taken over the other rows.  sklearn has no such option: there -1 is a cluster.
  - a (with return_parts=True) is 0 for a row alone in its cluster; sklearn's internal value there is nan before its s becomes 0.
  - cluster_medoids is not in sklearn: per cluster the row with the smallest sum of distances to its own cluster, the lowest row
    index on an exact tie; a cluster of one row is its own medoid.  (The reference's plot.sample_clusters picks exemplars at random.)
  - ValueError for non-finite rows and for more than SIL_MAX_CLUSTERS = 4096 clusters.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _clock, _on_device
from ._inputs import _feature_rows, _int_labels

SIL_MAX_CLUSTERS = _lib.SIL_MAX_CLUSTERS  # the cap on the number of clusters
_SIL_ROWS_PER_LAUNCH = 32768              # rows per svae_silhouette launch: bounds the partials (64 MB at K <= 256, 1 GB at 4096)
_SIL_CALLS = {"silhouette": 0, "mean": 0, "medoids": 0}  # launches of svae_silhouette / _mean / _medoids by this process
_SIL_LAST = {"work": 0, "ranges": 0}      # doubles of work and row ranges of the last run

SilhouetteParts = namedtuple("SilhouetteParts", ["s", "a", "b", "nearest"])

_device_of = functools.partial(_device._device_of, who="the silhouette runs on the GPU (csrc/silhouette.hip); no device is available")


def _sil_check(z, labels, noise_label):
    """the argument errors, before any device work -> (fp64 rows kept, lab int32 [m] in 0..K-1, count int32 [K], cluster labels
    [K], keep: the positions of the kept rows among all n (None: all of them), n)"""
    x = _feature_rows(z, "z")
    n = x.shape[0]
    labels = _int_labels(labels, n)
    keep = None
    kept = labels
    if noise_label is not None:
        mask = labels != noise_label
        if not mask.all():
            keep = np.flatnonzero(mask)
            kept = labels[keep]
            x = x[torch.from_numpy(keep).to(x.device)] if torch.is_tensor(x) else x[keep]
    m = kept.shape[0]
    uniq, lab, count = np.unique(kept, return_inverse=True, return_counts=True)
    K = len(uniq)
    if not 2 <= K <= m - 1:
        raise ValueError(f"Number of labels is {K}. Valid values are 2 to n_samples - 1 (inclusive), n_samples = {m}")
    if K > SIL_MAX_CLUSTERS:
        raise ValueError(f"at most {SIL_MAX_CLUSTERS} clusters are supported, got {K}")
    return x, lab.reshape(-1).astype(np.int32), count.astype(np.int32), uniq, keep, n


def _sil_work_size(m, K, lib):
    """doubles of work for the row ranges of m rows: the largest any of the launches asks for"""
    sizes = {min(m, _SIL_ROWS_PER_LAUNCH)}
    if m > _SIL_ROWS_PER_LAUNCH and m % _SIL_ROWS_PER_LAUNCH:
        sizes.add(m % _SIL_ROWS_PER_LAUNCH)
    return max(lib.svae_silhouette_work(r, m, K) for r in sizes)


def _sil_device(x, lab, count, info=None):
    """(s, a, b fp64 [m], nearest int32 [m] in 0..K-1, lab int32 [m]) on the device of x (or the current one).  info (a dict)
    receives the synchronised host-clock time sil_s of the svae_silhouette launches."""
    dev = _device_of(x)
    m, d = x.shape
    K = len(count)
    with torch.cuda.device(dev):
        lib = _lib.lib()
        Z = _on_device(x, dev)
        labd = torch.from_numpy(lab).to(dev)
        cnt = torch.from_numpy(count).to(dev)
        st = ops._stream()
        words = _sil_work_size(m, K, lib)
        work = torch.empty(words, dtype=torch.float64, device=dev)
        s, a, b = (torch.empty(m, dtype=torch.float64, device=dev) for _ in range(3))
        nearest = torch.empty(m, dtype=torch.int32, device=dev)
        t0 = _clock(dev, info is not None)
        ranges = 0
        for row0 in range(0, m, _SIL_ROWS_PER_LAUNCH):
            rows = min(_SIL_ROWS_PER_LAUNCH, m - row0)
            _SIL_CALLS["silhouette"] += 1
            ranges += 1
            check(lib.svae_silhouette(Z.data_ptr(), d, d, m, labd.data_ptr(), cnt.data_ptr(), K, row0, rows, work.data_ptr(),
                                      s[row0:].data_ptr(), a[row0:].data_ptr(), b[row0:].data_ptr(), nearest[row0:].data_ptr(), st),
                  "silhouette")
        if info is not None:
            info.update(sil_s=_clock(dev) - t0)
        _SIL_LAST.update(work=words, ranges=ranges)
    return s, a, b, nearest, labd


def _spread(v, keep, n, fill):
    """the values of the kept rows at their positions among all n rows, `fill` elsewhere"""
    if keep is None:
        return v
    out = np.full(n, fill, dtype=v.dtype)
    out[keep] = v
    return out


def silhouette_samples(z, labels, *, noise_label=None, return_parts=False):
    """The silhouette coefficient of every row, s [n] float64 numpy (sklearn.metrics.silhouette_samples, Euclidean metric).  With
    return_parts=True the namedtuple (s, a, b, nearest): the mean distance to the row's own cluster, to the nearest other cluster,
    and that cluster's label.  Rows labelled noise_label are left out and get nan (nearest = noise_label).  sklearn's
    sample_size / random_state and other metrics are not supported."""
    x, lab, count, uniq, keep, n = _sil_check(z, labels, noise_label)
    s, a, b, nearest, _ = _sil_device(x, lab, count)
    s = _spread(s.cpu().numpy(), keep, n, np.nan)
    if not return_parts:
        return s
    near = uniq[nearest.cpu().numpy()]
    if keep is not None:
        near = _spread(near, keep, n, np.asarray(noise_label).astype(near.dtype))
    return SilhouetteParts(s, _spread(a.cpu().numpy(), keep, n, np.nan), _spread(b.cpu().numpy(), keep, n, np.nan), near)


def silhouette_score(z, labels, *, noise_label=None):
    """The mean of silhouette_samples over all rows (over the rows not labelled noise_label), reduced on the device in a fixed
    order with compensated sums (sklearn.metrics.silhouette_score without sample_size)."""
    x, lab, count, _, _, _ = _sil_check(z, labels, noise_label)
    s, _, _, _, _ = _sil_device(x, lab, count)
    with torch.cuda.device(s.device):
        out = torch.empty(1, dtype=torch.float64, device=s.device)
        _SIL_CALLS["mean"] += 1
        check(_lib.lib().svae_silhouette_mean(s.data_ptr(), s.numel(), out.data_ptr(), ops._stream()), "silhouette_mean")
        return float(out.cpu()[0])


def cluster_silhouette(z, labels, *, noise_label=None):
    """(cluster_labels [K] in np.unique order, the mean s of each cluster's rows [K] float64, sizes [K] int64): which clusters
    are tight and which are not.  Rows labelled noise_label belong to no cluster."""
    x, lab, count, uniq, _, _ = _sil_check(z, labels, noise_label)
    s = _sil_device(x, lab, count)[0].cpu().numpy()
    sizes = count.astype(np.int64)
    return uniq, np.bincount(lab, weights=s, minlength=len(uniq)) / sizes, sizes


def cluster_medoids(z, labels, *, noise_label=None):
    """(cluster_labels [K] in np.unique order, row_index [K] int64): per cluster the row of z with the smallest sum of distances
    to the rows of its cluster, the lowest row index on an exact tie, taken on the device from a (the cluster size is shared
    within a cluster).  A cluster of one row is its own medoid."""
    x, lab, count, uniq, keep, _ = _sil_check(z, labels, noise_label)
    _, a, _, _, labd = _sil_device(x, lab, count)
    K = len(uniq)
    with torch.cuda.device(a.device):
        key = torch.empty(K, dtype=torch.int64, device=a.device)
        row = torch.empty(K, dtype=torch.int64, device=a.device)
        _SIL_CALLS["medoids"] += 1
        check(_lib.lib().svae_silhouette_medoids(a.data_ptr(), labd.data_ptr(), a.numel(), K, key.data_ptr(), row.data_ptr(),
                                                 ops._stream()), "silhouette_medoids")
        row = row.cpu().numpy()
    return uniq, (row if keep is None else keep[row].astype(np.int64))
