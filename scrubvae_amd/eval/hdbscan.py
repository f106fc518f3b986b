"""HDBSCAN clustering of latents on the device (reference: src/scrubvae/eval/cluster.py::dbscan, which runs sklearn's HDBSCAN).

    HDBSCAN(min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, max_cluster_size=None, metric="euclidean",
            metric_params=None, alpha=1.0, algorithm="auto", leaf_size=40, n_jobs=None, cluster_selection_method="eom",
            allow_single_cluster=False, store_centers=None, copy=False)

restates sklearn 1.7's HDBSCAN for euclidean feature arrays: the same arguments, fit / fit_predict / dbscan_clustering, and the
fitted attributes labels_, probabilities_, n_features_in_ and _single_linkage_tree_ (sklearn's field names), all host numpy.  A
fitted object pickles without a GPU.  sklearn is never imported.

Rows are the input converted to fp64 (exact for float32 latents), not centred.  csrc/hdbscan.hip computes, in fp64 and without
FMA, the core distances (the exact k-th smallest distance of each row, k = min_samples, itself included) and the minimum spanning
tree of the mutual-reachability graph max(core_i, core_j, d_ij / alpha) by Boruvka rounds; each round the host downloads one
edge per component and merges components.  Edges are ordered by the strict key (w, min(i, j), max(i, j)), so the tree is unique
and fits are bit-reproducible.  The single-linkage tree, the condensed tree, cluster selection, labels and probabilities follow
sklearn 1.7's semantics in host C++ (svae_hdb_tree).

Differences from sklearn, by design: where several spanning trees share the minimum weight, sklearn's pick depends on its
traversal order, this one on the key above; the single-linkage tree puts the root of the smaller endpoint on the left, so cluster
numbers can differ from sklearn's by a renumbering.  algorithm, leaf_size, n_jobs and copy are accepted and choose nothing: every
fit is the result of sklearn's default (KD-tree) path.  Up to ties, sklearn's algorithms agree at alpha = 1; at alpha != 1
sklearn's algorithm="brute" also divides the core distances by alpha, and that result is not reproduced here.  Only
metric="euclidean" is supported; store_centers raises.
Rows holding NaN or inf get sklearn's outlier encoding (label -3 / probability NaN for a row whose sum is NaN, -2 / 0 for one
whose sum is infinite) and the finite rows are clustered without them.
"""
from __future__ import annotations

import ctypes as C
import functools
import numbers
import time

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _clock

HIERARCHY_dtype = np.dtype([("left_node", np.intp), ("right_node", np.intp), ("value", np.float64), ("cluster_size", np.intp)])
_OUTLIER_ENCODING = {"infinite": {"label": -2, "prob": 0.0}, "missing": {"label": -3, "prob": np.nan}}
_SELECTION = ("eom", "leaf")
_ALGORITHMS = ("auto", "brute", "kd_tree", "ball_tree")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _rows(X):
    """X [n, d] -> (finite rows as fp64 (torch tensor where it is, or numpy), n_raw, finite, infinite, missing index arrays);
    a row is missing when its sum is NaN and infinite when its sum is infinite, as sklearn classifies them"""
    if torch.is_tensor(X):
        t = X.detach()
        if t.dim() != 2:
            raise ValueError(f"Expected 2D array, got {t.dim()}D tensor instead")
        t = t.to(torch.float64)
        sums = t.sum(1).cpu().numpy()
    else:
        t = np.asarray(X)
        if t.ndim != 2:
            raise ValueError(f"Expected 2D array, got {t.ndim}D array instead")
        t = np.ascontiguousarray(t, dtype=np.float64)
        sums = t.sum(axis=1)
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"Found array with shape {tuple(t.shape)} while a minimum of 1 sample and 1 feature is required.")
    missing = np.isnan(sums).nonzero()[0]
    infinite = np.isinf(sums).nonzero()[0]
    finite = np.isfinite(sums).nonzero()[0]
    if len(finite) < t.shape[0]:
        t = t[torch.from_numpy(finite).to(t.device)] if torch.is_tensor(t) else t[finite]
    return t, int(sums.shape[0]), finite, infinite, missing


_device_of = functools.partial(_device._device_of, who="HDBSCAN runs on the GPU (csrc/hdbscan.hip); no device is available")


def mst_device(x, min_samples, alpha=1.0):
    """(core [n], lo [n - 1], hi [n - 1], w [n - 1], timings): core distances and the minimum spanning tree of the mutual
    reachability graph of the fp64 rows x (numpy or torch, [n, d], n >= 2), edges in the order the Boruvka rounds found them.
    Runs on x's device (or the current one for host input), made current for the launches: the C ABI launches on the current
    device's stream."""
    device = _device_of(x)
    with torch.cuda.device(device):
        return _mst_on(x, min_samples, alpha, device)


def _mst_on(x, min_samples, alpha, device):
    lib = _lib.lib()
    X = (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(device=device, dtype=torch.float64).contiguous()
    n, d = X.shape
    f64 = dict(dtype=torch.float64, device=device)
    i64 = dict(dtype=torch.int64, device=device)
    st = ops._stream()
    t0 = _clock(device)
    core = torch.empty(n, **f64)
    check(lib.svae_hdb_core(X.data_ptr(), d, d, n, int(min_samples), core.data_ptr(), st), "hdb_core")
    t1 = _clock(device)
    order = torch.sort(core, stable=True).indices
    Xs = X.index_select(0, order).contiguous()
    cs = core.index_select(0, order).contiguous()
    ids = order.to(torch.int32).contiguous()
    comp_d = ids.clone()
    bw, bp = torch.empty(n, **f64), torch.empty(n, **i64)
    cw, cp = torch.empty(n, **i64), torch.empty(n, **i64)
    lo, hi, w = np.empty(n - 1, np.int32), np.empty(n - 1, np.int32), np.empty(n - 1, np.float64)
    comp_h, map_h = np.arange(n, dtype=np.int32), np.empty(n, np.int32)
    n_edges, n_new = C.c_int(0), C.c_int(0)
    n_comp, rounds = n, 0
    while n_comp > 1:
        check(lib.svae_hdb_boruvka(Xs.data_ptr(), d, d, n, cs.data_ptr(), ids.data_ptr(), comp_d.data_ptr(), float(alpha), n_comp,
                                   bw.data_ptr(), bp.data_ptr(), cw.data_ptr(), cp.data_ptr(), st), "hdb_boruvka")
        cw_h = np.ascontiguousarray(cw[:n_comp].cpu().numpy().view(np.uint64))
        cp_h = np.ascontiguousarray(cp[:n_comp].cpu().numpy().view(np.uint64))
        check(lib.svae_hdb_merge(n, n_comp, _ptr(cw_h), _ptr(cp_h), _ptr(comp_h), _ptr(map_h), _ptr(lo), _ptr(hi), _ptr(w),
                                 C.byref(n_edges), C.byref(n_new)), "hdb_merge")
        map_d = torch.from_numpy(map_h[:n_comp].copy()).to(device)
        check(lib.svae_hdb_relabel(comp_d.data_ptr(), n, map_d.data_ptr(), st), "hdb_relabel")
        n_comp = n_new.value
        rounds += 1
    t2 = _clock(device)
    if n_edges.value != n - 1:
        raise RuntimeError(f"hdb: {n_edges.value} MST edges for {n} rows")
    return core.cpu().numpy(), lo, hi, w, dict(core_s=t1 - t0, boruvka_s=t2 - t1, rounds=rounds)


def tree_labels(lo, hi, w, min_cluster_size, cluster_selection_method="eom", allow_single_cluster=False,
                cluster_selection_epsilon=0.0, max_cluster_size=None):
    """(single-linkage tree, labels, probabilities) from the n - 1 MST edges (host C++, svae_hdb_tree)"""
    n = len(lo) + 1
    lo = np.ascontiguousarray(lo, np.int32)
    hi = np.ascontiguousarray(hi, np.int32)
    w = np.ascontiguousarray(w, np.float64)
    sl = [np.empty(n - 1, np.int64), np.empty(n - 1, np.int64), np.empty(n - 1, np.float64), np.empty(n - 1, np.int64)]
    labels, prob = np.empty(n, np.int64), np.empty(n, np.float64)
    check(_lib.lib().svae_hdb_tree(n, _ptr(lo), _ptr(hi), _ptr(w), int(min_cluster_size), int(cluster_selection_method == "leaf"),
                                   int(bool(allow_single_cluster)), float(cluster_selection_epsilon),
                                   0 if max_cluster_size is None else int(max_cluster_size), *[_ptr(a) for a in sl], _ptr(labels),
                                   _ptr(prob)), "hdb_tree")
    tree = np.zeros(n - 1, dtype=HIERARCHY_dtype)
    for f, a in zip(HIERARCHY_dtype.names, sl):
        tree[f] = a
    return tree, labels.astype(np.intp), prob


def labelling_at_cut(tree, cut, min_cluster_size):
    """sklearn's labelling_at_cut over a single-linkage tree (host C++, svae_hdb_cut)"""
    left = np.ascontiguousarray(tree["left_node"], np.int64)
    right = np.ascontiguousarray(tree["right_node"], np.int64)
    value = np.ascontiguousarray(tree["value"], np.float64)
    labels = np.empty(len(tree) + 1, np.int64)
    check(_lib.lib().svae_hdb_cut(len(tree) + 1, _ptr(left), _ptr(right), _ptr(value), float(cut), int(min_cluster_size),
                                  _ptr(labels)), "hdb_cut")
    return labels.astype(np.intp)


def _remap_tree(tree, finite, non_finite):
    """sklearn's remap_single_linkage_tree: finite-row nodes back to raw row numbers, internal nodes shifted by the outlier
    count, then one row per outlier merging it at distance inf"""
    tree = tree.copy()
    fc, oc = len(finite), len(non_finite)
    for f in ("left_node", "right_node"):
        a = tree[f]
        tree[f] = np.where(a < fc, finite[np.minimum(a, fc - 1)], a + oc)
    out = np.zeros(oc, dtype=HIERARCHY_dtype)
    last_id = max(tree[-1]["left_node"], tree[-1]["right_node"])
    last_size = tree[-1]["cluster_size"]
    for i, o in enumerate(non_finite):
        out[i] = (o, last_id + 1, np.inf, last_size + 1)
        last_id += 1
        last_size += 1
    return np.concatenate([tree, out])


class HDBSCAN:
    """sklearn.cluster.HDBSCAN (1.7) on the device; see the module docstring"""

    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, max_cluster_size=None,
                 metric="euclidean", metric_params=None, alpha=1.0, algorithm="auto", leaf_size=40, n_jobs=None,
                 cluster_selection_method="eom", allow_single_cluster=False, store_centers=None, copy=False):
        self.min_cluster_size = min_cluster_size
        self.min_samples = min_samples
        self.cluster_selection_epsilon = cluster_selection_epsilon
        self.max_cluster_size = max_cluster_size
        self.metric = metric
        self.metric_params = metric_params
        self.alpha = alpha
        self.algorithm = algorithm
        self.leaf_size = leaf_size
        self.n_jobs = n_jobs
        self.cluster_selection_method = cluster_selection_method
        self.allow_single_cluster = allow_single_cluster
        self.store_centers = store_centers
        self.copy = copy

    def get_params(self, deep=True):
        return {k: getattr(self, k) for k in ("min_cluster_size", "min_samples", "cluster_selection_epsilon", "max_cluster_size",
                                              "metric", "metric_params", "alpha", "algorithm", "leaf_size", "n_jobs",
                                              "cluster_selection_method", "allow_single_cluster", "store_centers", "copy")}

    def _check_params(self):
        def integral(v, lo, name, none_ok=False):
            if v is None and none_ok:
                return
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < lo:
                raise ValueError(f"The '{name}' parameter of HDBSCAN must be an int in the range [{lo}, inf)"
                                 + (" or None" if none_ok else "") + f". Got {v!r} instead.")

        integral(self.min_cluster_size, 2, "min_cluster_size")
        integral(self.min_samples, 1, "min_samples", none_ok=True)
        integral(self.max_cluster_size, 1, "max_cluster_size", none_ok=True)
        integral(self.leaf_size, 1, "leaf_size")
        eps = self.cluster_selection_epsilon
        if isinstance(eps, bool) or not isinstance(eps, numbers.Real) or not eps >= 0.0:
            raise ValueError(f"The 'cluster_selection_epsilon' parameter of HDBSCAN must be a float in the range [0.0, inf). "
                             f"Got {eps!r} instead.")
        a = self.alpha
        if isinstance(a, bool) or not isinstance(a, numbers.Real) or not a > 0.0:
            raise ValueError(f"The 'alpha' parameter of HDBSCAN must be a float in the range (0.0, inf). Got {a!r} instead.")
        if self.cluster_selection_method not in _SELECTION:
            raise ValueError(f"The 'cluster_selection_method' parameter of HDBSCAN must be a str among {set(_SELECTION)}. "
                             f"Got {self.cluster_selection_method!r} instead.")
        if self.algorithm not in _ALGORITHMS:
            raise ValueError(f"The 'algorithm' parameter of HDBSCAN must be a str among {set(_ALGORITHMS)}. "
                             f"Got {self.algorithm!r} instead.")
        if self.metric != "euclidean":
            raise NotImplementedError(f"HDBSCAN on the device supports metric='euclidean' only, got {self.metric!r}")
        if self.store_centers is not None:
            raise NotImplementedError("HDBSCAN on the device does not compute store_centers")

    def fit(self, X, y=None):
        """Cluster X ([n, d] numpy or torch tensor, CPU or GPU) and return self"""
        self._check_params()
        x, n_raw, finite, infinite, missing = _rows(X)
        n, d = x.shape
        if n == 1:
            raise ValueError("n_samples=1 while HDBSCAN requires more than one sample")
        self._min_samples = self.min_cluster_size if self.min_samples is None else self.min_samples
        if self._min_samples > n:
            raise ValueError(f"min_samples ({self._min_samples}) must be at most the number of samples in X ({n})")
        self.n_features_in_ = int(d)
        core, lo, hi, w, timings = mst_device(x, self._min_samples, self.alpha)
        t0 = time.perf_counter()
        tree, labels, prob = tree_labels(lo, hi, w, self.min_cluster_size, self.cluster_selection_method, self.allow_single_cluster,
                                         self.cluster_selection_epsilon, self.max_cluster_size)
        timings["tree_s"] = time.perf_counter() - t0
        self._core_distances_ = core
        self._mst_ = (lo.astype(np.int64), hi.astype(np.int64), w)
        self._timings_ = timings
        self._single_linkage_tree_ = tree
        self.labels_, self.probabilities_ = labels, prob
        if n < n_raw:
            non_finite = set(np.hstack([infinite, missing]))
            self._single_linkage_tree_ = _remap_tree(tree, finite, list(non_finite))
            new_labels = np.empty(n_raw, dtype=np.int32)
            new_labels[finite] = labels
            new_labels[infinite] = _OUTLIER_ENCODING["infinite"]["label"]
            new_labels[missing] = _OUTLIER_ENCODING["missing"]["label"]
            new_prob = np.zeros(n_raw, dtype=np.float64)
            new_prob[finite] = prob
            new_prob[infinite] = _OUTLIER_ENCODING["infinite"]["prob"]
            new_prob[missing] = _OUTLIER_ENCODING["missing"]["prob"]
            self.labels_, self.probabilities_ = new_labels, new_prob
        return self

    def fit_predict(self, X, y=None):
        """fit(X) and return labels_"""
        return self.fit(X).labels_

    def dbscan_clustering(self, cut_distance, min_cluster_size=5):
        """DBSCAN* labels at a mutual-reachability cut of the fitted single-linkage tree (sklearn's dbscan_clustering)"""
        labels = labelling_at_cut(self._single_linkage_tree_, cut_distance, min_cluster_size)
        labels[self.labels_ == _OUTLIER_ENCODING["infinite"]["label"]] = _OUTLIER_ENCODING["infinite"]["label"]
        labels[self.labels_ == _OUTLIER_ENCODING["missing"]["label"]] = _OUTLIER_ENCODING["missing"]["label"]
        return labels
