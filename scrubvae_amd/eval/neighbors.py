"""Exact k nearest neighbours of every latent, on the device (csrc/knn.hip).

    kneighbors(z, n_neighbors, *, group=None, return_distance=True)    (dist [n, k] float64, idx [n, k] int64) numpy, or idx alone
    kneighbors_graph(z, n_neighbors, mode="connectivity")              scipy.sparse.csr_matrix [n, n]; mode="distance": the distances
    knn_label_purity(z, labels, n_neighbors)                           (share of the k neighbours with the row's own label [n], its mean)
    kneighbors_cross(z_ref, z_query, n_neighbors, *, return_distance=True)   (dist [m, k], idx [m, k]) of the queries among z_ref
    knn_transfer_labels(z_ref, labels_ref, z_query, n_neighbors, *, noise_label=None)   the majority label of those neighbours [m]

z is [n, d], numpy or torch, host or device, any float dtype; the rows go to fp64 uncentred, as for mmd_* and the silhouette.

The neighbours of row i are the k smallest keys (s_ij, j) over j != i: s_ij the squared distance in the arithmetic of
csrc/pair_tiles.h (feature order, every operation rounded on its own: sklearn's KD-tree metric), then the lower index.  The row
itself is left out by index, not by distance, so a duplicate of row i is a neighbour at distance 0, and exact ties come out in
index order.  Row i of the result holds its neighbours in ascending key order with dist = sqrt(s).  This is
sklearn.neighbors.NearestNeighbors(n_neighbors).fit(z).kneighbors() (the query point excluded), with the ties decided.  The key is
strict, so the result is unique: bit-reproducible, and independent of how the device splits the work.

group [n] (integers) keeps for row i only the candidates j with group[j] != group[i]: with group = the cross-validation fold, one
call gives every row's neighbours among the training rows of its fold (eval.metrics.knn_class_rand_cv / knn_reg_rand_cv).

kneighbors_cross searches a query set against a reference set with the same key over ALL reference rows (svae_knn_cross): nothing
is left out, a query equal to a reference row has it at distance 0.  It is NearestNeighbors(k).fit(z_ref).kneighbors(z_query), and
knn_transfer_labels is KNeighborsClassifier(k) with uniform weights: it carries the labels of a clustering to rows that were not
in it (a tie goes to the smallest label).

One pass over the n^2 (m n) distances, nothing of that size stored; n_neighbors <= KNN_MAX_K = 90 (what the kernel's LDS holds).
ValueError for non-finite rows and for every argument out of range, before any device work."""
from __future__ import annotations

import functools

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _clock, _on_device
from ._inputs import _feature_rows, _finite_rows, _int_labels, _is_int

KNN_MAX_K = _lib.KNN_MAX_K             # the cap on n_neighbors
_KNN_CALLS = {"knn": 0, "cross": 0}    # launches of svae_knn / svae_knn_cross by this process
_KNN_LAST = {"work": 0, "chunks": 0}   # bytes of work and column chunks per row tile of the last run

_device_of = functools.partial(_device._device_of, who="the neighbour search runs on the GPU (csrc/knn.hip); no device is available")


def _knn_check(z, n_neighbors, group=None):
    """the argument errors, before any device work -> (fp64 rows, k, group int32 [n] numpy or None)"""
    x = _feature_rows(z, "z")
    n = x.shape[0]
    if not _is_int(n_neighbors):
        raise ValueError(f"n_neighbors must be an integer, got {n_neighbors!r}")
    k = int(n_neighbors)
    if k < 1:
        raise ValueError(f"Expected n_neighbors > 0. Got {k}")
    if k > n - 1:
        raise ValueError(f"Expected n_neighbors <= n_samples - 1 (the row itself is not a neighbour), but n_neighbors = {k}, n_samples = {n}")
    if k > KNN_MAX_K:
        raise ValueError(f"at most {KNN_MAX_K} neighbours are supported, got {k}")
    if n >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 rows are supported, got {n}")
    grp = None
    if group is not None:
        _, grp, count = np.unique(_int_labels(group, n), return_inverse=True, return_counts=True)
        grp = grp.reshape(-1).astype(np.int32)
        if n - count.max() < k:
            raise ValueError(f"group {int(count.argmax())} (in np.unique order) holds {int(count.max())} of the {n} rows: its rows keep "
                             f"fewer than n_neighbors = {k} candidates")
    return x, k, grp


def _knn_device(x, k, grp, info=None):
    """(dist fp64 [n, k], idx int32 [n, k]) on the device of x (or the current one).  info (a dict) receives the synchronised
    host-clock time knn_s of the svae_knn call."""
    dev = _device_of(x)
    n, d = x.shape
    with torch.cuda.device(dev):
        lib = _lib.lib()
        Z = _on_device(x, dev)
        gd = None if grp is None else torch.from_numpy(grp).to(dev)
        nbytes = lib.svae_knn_work(n, k)
        work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        idx = torch.empty(n, k, dtype=torch.int32, device=dev)
        dist = torch.empty(n, k, dtype=torch.float64, device=dev)
        t0 = _clock(dev, info is not None)
        _KNN_CALLS["knn"] += 1
        check(lib.svae_knn(Z.data_ptr(), d, d, n, k, ops._p(gd), work.data_ptr(), idx.data_ptr(), dist.data_ptr(), ops._stream()), "knn")
        if info is not None:
            info.update(knn_s=_clock(dev) - t0)
        _KNN_LAST.update(work=nbytes, chunks=nbytes // (-(-n // 64) * 64 * k * 12))
    return dist, idx


def kneighbors(z, n_neighbors, *, group=None, return_distance=True):
    """The n_neighbors nearest other rows of every row of z: (dist [n, k] float64, idx [n, k] int64) as numpy arrays, or idx alone
    (sklearn's NearestNeighbors(n_neighbors).fit(z).kneighbors()).  group [n]: only rows of another group are candidates."""
    x, k, grp = _knn_check(z, n_neighbors, group)
    dist, idx = _knn_device(x, k, grp)
    idx = idx.cpu().numpy().astype(np.int64)
    return (dist.cpu().numpy(), idx) if return_distance else idx


def _knn_cross_check(z_ref, z_query, n_neighbors):
    """the argument errors of a query set against a reference set, before any device work -> (fp64 reference rows, query rows, k)"""
    x, q = _finite_rows(z_ref, "z_ref"), _finite_rows(z_query, "z_query")
    n, d = x.shape
    if d < 1:
        raise ValueError("z_ref must have at least one feature")
    if q.shape[1] != d:
        raise ValueError(f"z_query has {q.shape[1]} features, z_ref has {d}")
    if n < 1 or q.shape[0] < 1:
        raise ValueError(f"z_ref and z_query need at least one row each, got {n} and {q.shape[0]}")
    if not _is_int(n_neighbors):
        raise ValueError(f"n_neighbors must be an integer, got {n_neighbors!r}")
    k = int(n_neighbors)
    if k < 1:
        raise ValueError(f"Expected n_neighbors > 0. Got {k}")
    if k > n:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {n}")
    if k > KNN_MAX_K:
        raise ValueError(f"at most {KNN_MAX_K} neighbours are supported, got {k}")
    if n >= 2 ** 31 or q.shape[0] >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 rows are supported, got {n} and {q.shape[0]}")
    return x, q, k


def _knn_cross_device(X, Q, k):
    """(dist fp64 [m, k], idx int32 [m, k]) of the rows of Q among the rows of X, both contiguous fp64 on the current device"""
    lib = _lib.lib()
    (n, d), m = X.shape, Q.shape[0]
    nbytes = lib.svae_knn_cross_work(m, n, k)
    work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=X.device)
    idx = torch.empty(m, k, dtype=torch.int32, device=X.device)
    dist = torch.empty(m, k, dtype=torch.float64, device=X.device)
    _KNN_CALLS["cross"] += 1
    check(lib.svae_knn_cross(Q.data_ptr(), d, m, X.data_ptr(), d, n, d, k, work.data_ptr(), idx.data_ptr(), dist.data_ptr(), ops._stream()),
          "knn_cross")
    return dist, idx


def _knn_cross(x, q, k):
    dev = _device_of(q, x)
    with torch.cuda.device(dev):
        return _knn_cross_device(_on_device(x, dev), _on_device(q, dev), k)


def kneighbors_cross(z_ref, z_query, n_neighbors, *, return_distance=True):
    """The n_neighbors nearest rows of z_ref for every row of z_query: (dist [m, k] float64, idx [m, k] int64) as numpy arrays, or
    idx alone (sklearn's NearestNeighbors(n_neighbors).fit(z_ref).kneighbors(z_query)).  The key is kneighbors' (squared distance
    by bit pattern, then the lower reference index), and no row is left out: a query equal to a reference row has it at distance 0."""
    x, q, k = _knn_cross_check(z_ref, z_query, n_neighbors)
    dist, idx = _knn_cross(x, q, k)
    idx = idx.cpu().numpy().astype(np.int64)
    return (dist.cpu().numpy(), idx) if return_distance else idx


def _vote(labels_nb):
    """host glue: per row of labels_nb [m, k] the most frequent value, a tie going to the smallest (np.unique order)"""
    classes, code = np.unique(labels_nb, return_inverse=True)
    code = code.reshape(labels_nb.shape)
    votes = np.zeros((len(code), len(classes)), dtype=np.int64)
    for t in range(code.shape[1]):
        np.add.at(votes, (np.arange(len(code)), code[:, t]), 1)
    return classes[votes.argmax(1)]           # argmax takes the first maximum: the smallest label


def knn_transfer_labels(z_ref, labels_ref, z_query, n_neighbors, *, noise_label=None):
    """labels [m] for the rows of z_query: the majority label among each row's n_neighbors nearest rows of z_ref, a tie going to
    the smallest label in np.unique order (sklearn's KNeighborsClassifier(n_neighbors) with uniform weights).  This carries the
    labels of a clustering (GaussianMixture, HDBSCAN) of z_ref to new windows.  noise_label names the label that stands for "no
    cluster" (HDBSCAN's -1): reference rows that carry it still vote, so a query among noise is noise."""
    x, q, k = _knn_cross_check(z_ref, z_query, n_neighbors)
    lab = _int_labels(labels_ref, x.shape[0])
    if noise_label is not None and not _is_int(noise_label):
        raise ValueError(f"noise_label must be an integer or None, got {noise_label!r}")
    _, idx = _knn_cross(x, q, k)
    return _vote(np.asarray(lab).reshape(-1)[idx.cpu().numpy().astype(np.int64)])


def _graph(dist, idx, n, mode):
    """host glue: the csr_matrix [n, n] of idx [n, k] with 1.0 or dist [n, k] as data, each row in neighbour order"""
    from scipy.sparse import csr_matrix
    k = idx.shape[1]
    data = np.ones(n * k) if mode == "connectivity" else np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
    return csr_matrix((data, np.ascontiguousarray(idx).reshape(-1), np.arange(0, n * k + 1, k)), shape=(n, n))


def kneighbors_graph(z, n_neighbors, mode="connectivity"):
    """The k-neighbour graph as a scipy.sparse.csr_matrix [n, n] (sklearn.neighbors.kneighbors_graph, include_self=False): row i
    holds its neighbours in key order, with 1.0 (mode="connectivity") or the distance (mode="distance")."""
    if mode not in ("connectivity", "distance"):
        raise ValueError(f'Unsupported mode, must be one of "connectivity", or "distance" but got "{mode}" instead')
    x, k, _ = _knn_check(z, n_neighbors)
    dist, idx = _knn_device(x, k, None)
    return _graph(dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64), x.shape[0], mode)


def knn_label_purity(z, labels, n_neighbors):
    """(the share of each row's n_neighbors neighbours that carry the row's own label [n] float64, its mean as a float): do the
    windows of one animal or class still sit next to each other?  labels [n], any integer dtype, numpy or torch."""
    x, k, _ = _knn_check(z, n_neighbors)
    _, lab = np.unique(_int_labels(labels, x.shape[0]), return_inverse=True)
    _, idx = _knn_device(x, k, None)
    labd = torch.from_numpy(lab.reshape(-1).astype(np.int64)).to(idx.device)
    same = (labd[idx.long()] == labd[:, None]).sum(1)
    share = same.cpu().numpy().astype(np.float64) / k
    return share, float(share.mean())
