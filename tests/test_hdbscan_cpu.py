"""HDBSCAN without a GPU: the restatement of tests/hdbscan_checks.py against sklearn's default path, the host tree steps of
csrc/hdbscan.hip against the restatement, argument errors and the C-ABI exports."""
import numpy as np
import pytest

from tests import hdbscan_checks as H

CASES = [
    ("blobs", 4000, dict(min_cluster_size=50)),
    ("leaf", 4000, dict(min_cluster_size=50, cluster_selection_method="leaf")),
    ("epsilon", 4000, dict(min_cluster_size=50, cluster_selection_epsilon=3.0)),
    ("max_cluster_size", 4000, dict(min_cluster_size=50, max_cluster_size=400)),
    ("single", 4000, dict(min_cluster_size=50, allow_single_cluster=True)),
    ("min_samples", 4000, dict(min_cluster_size=50, min_samples=20)),
    ("alpha", 3000, dict(min_cluster_size=50, alpha=0.7)),
    ("duplicates", 3000, dict(min_cluster_size=100)),
]


def _data(name, n, seed=1):
    x, _ = H.planted(n, 32, 6, seed)
    if name == "duplicates":
        x[:600] = x[700]
    return x.astype(np.float64)


def _restate(x, kw):
    return H.fit(x, kw["min_cluster_size"], kw.get("min_samples"), kw.get("alpha", 1.0), kw.get("cluster_selection_method", "eom"),
                 kw.get("allow_single_cluster", False), kw.get("cluster_selection_epsilon", 0.0), kw.get("max_cluster_size"))


@pytest.mark.parametrize("name,n,kw", CASES, ids=[c[0] for c in CASES])
def test_restatement_matches_sklearn(name, n, kw):
    sk_cluster = pytest.importorskip("sklearn.cluster")
    from sklearn.neighbors import NearestNeighbors
    x = _data(name, n)
    sk = sk_cluster.HDBSCAN(**kw).fit(x)
    # precondition: sklearn's own tie order is not canonical, so the data must not depend on it.  At alpha != 1 sklearn's brute
    # path scales the core distances too (its default path does not), so the data set is checked at alpha = 1 there.
    pre = {k: v for k, v in kw.items() if k != "alpha"}
    assert np.array_equal(sk_cluster.HDBSCAN(**pre).fit(x).labels_, sk_cluster.HDBSCAN(algorithm="brute", **pre).fit(x).labels_)
    ref = _restate(x, kw)
    k = kw.get("min_samples") or kw["min_cluster_size"]
    assert np.array_equal(ref["core"], NearestNeighbors(algorithm="kd_tree").fit(x).kneighbors(x, k)[0][:, -1])
    assert np.array_equal(np.sort(ref["w"]), np.sort(sk._single_linkage_tree_["value"]))
    assert H.same_partition(ref["labels"], sk.labels_)
    assert np.abs(ref["probabilities"] - sk.probabilities_).max() <= 1e-12
    assert len(np.unique(ref["labels"])) >= 2 or name == "max_cluster_size"
    if name == "blobs":
        for cut in (1.0, 3.0):
            assert H.same_partition(H.cut_labels(ref["tree"], cut, 5), sk.dbscan_clustering(cut, 5))


def test_non_finite_rows_match_sklearn():
    sk_cluster = pytest.importorskip("sklearn.cluster")
    from scrubvae_amd.eval import hdbscan as M
    x = _data("blobs", 2000)
    x[[5, 77]] = np.nan
    x[[10, 1999]] = np.inf
    x[300, 2] = -np.inf
    x[301, 3], x[301, 4] = np.inf, -np.inf
    sk = sk_cluster.HDBSCAN(min_cluster_size=30).fit(x)
    fin = np.isfinite(x.sum(1))
    ref = H.fit(x[fin], 30)
    assert H.same_partition(ref["labels"], sk.labels_[fin])
    assert (sk.labels_[[5, 77, 301]] == -3).all() and (sk.labels_[[10, 1999, 300]] == -2).all()
    # the host steps of the product on the restatement's tree: remapped tree and outlier encoding as sklearn's
    finite = np.nonzero(fin)[0]
    non_finite = list(set(np.hstack([np.nonzero(np.isinf(x.sum(1)))[0], np.nonzero(np.isnan(x.sum(1)))[0]])))
    tree = M._remap_tree(ref["tree"], finite, non_finite)
    assert np.array_equal(np.sort(tree["value"]), np.sort(sk._single_linkage_tree_["value"]))
    lab = M.labelling_at_cut(tree, 2.0, 5)
    assert H.same_partition(lab[fin], sk.dbscan_clustering(2.0, 5)[fin])


@pytest.mark.parametrize("name,n,kw", CASES, ids=[c[0] for c in CASES])
def test_host_tree_matches_restatement(name, n, kw):
    """svae_hdb_tree / svae_hdb_cut are host code: bit-equal to the restatement on the restatement's MST"""
    from scrubvae_amd.eval import hdbscan as M
    x = _data(name, min(n, 2500), seed=2)
    ref = _restate(x, kw)
    perm = np.random.default_rng(0).permutation(len(ref["w"]))  # the edge order must not matter
    tree, labels, prob = M.tree_labels(ref["lo"][perm], ref["hi"][perm], ref["w"][perm], kw["min_cluster_size"],
                                       kw.get("cluster_selection_method", "eom"), kw.get("allow_single_cluster", False),
                                       kw.get("cluster_selection_epsilon", 0.0), kw.get("max_cluster_size"))
    assert np.array_equal(tree, ref["tree"])
    assert np.array_equal(labels, ref["labels"])
    assert np.array_equal(prob, ref["probabilities"])
    for cut in (1.0, 3.0):
        assert np.array_equal(M.labelling_at_cut(tree, cut, 5), H.cut_labels(ref["tree"], cut, 5))


def test_host_merge_builds_the_tree():
    """svae_hdb_merge (host) fed with exact per-component minimum edges reproduces the restatement's MST"""
    import ctypes as C
    from scrubvae_amd import _lib
    x = _data("blobs", 600, seed=3)
    n = len(x)
    core = H.core_distances(x, 10)
    lo_r, hi_r, w_r = H.prim_mst(x, core)
    Xt = np.ascontiguousarray(x.T)
    W = np.maximum(np.maximum(core[:, None], core[None, :]), np.sqrt(H.sq_dists(Xt, x)))
    comp = np.arange(n, dtype=np.int32)
    lo, hi, w = np.empty(n - 1, np.int32), np.empty(n - 1, np.int32), np.empty(n - 1)
    mp = np.empty(n, np.int32)
    ne, nc = C.c_int(0), C.c_int(0)
    n_comp = n
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    while n_comp > 1:
        other = comp[:, None] != comp[None, :]
        cw = np.full(n_comp, np.inf)
        cp = np.full(n_comp, np.iinfo(np.uint64).max, np.uint64)
        key_w = np.where(other, W, np.inf)
        for c in range(n_comp):
            rows = comp == c
            kw_ = key_w[rows]
            m = kw_.min()
            sel = kw_ == m
            a = np.minimum(ii[rows], jj[rows])[sel].astype(np.uint64)
            b = np.maximum(ii[rows], jj[rows])[sel].astype(np.uint64)
            cw[c], cp[c] = m, ((a << np.uint64(32)) | b).min()
        cwb = np.ascontiguousarray(cw.view(np.uint64))
        _lib.check(_lib.lib().svae_hdb_merge(n, n_comp, cwb.ctypes.data, cp.ctypes.data, comp.ctypes.data, mp.ctypes.data,
                                             lo.ctypes.data, hi.ctypes.data, w.ctypes.data, C.byref(ne), C.byref(nc)))
        n_comp = nc.value
    assert ne.value == n - 1
    assert H.edge_set(lo, hi, w) == H.edge_set(lo_r, hi_r, w_r)


@pytest.mark.parametrize("kw,X,err", [
    (dict(min_samples=11), np.zeros((10, 3)), ValueError),
    (dict(), np.zeros((1, 3)), ValueError),
    (dict(), np.array([[0.0, 1.0], [np.nan, 1.0]]), ValueError),
    (dict(min_cluster_size=1), np.zeros((10, 3)), ValueError),
    (dict(alpha=0.0), np.zeros((10, 3)), ValueError),
    (dict(cluster_selection_method="x"), np.zeros((10, 3)), ValueError),
    (dict(metric="manhattan"), np.zeros((10, 3)), NotImplementedError),
    (dict(store_centers="centroid"), np.zeros((10, 3)), NotImplementedError),
])
def test_argument_errors_before_device_work(kw, X, err):
    from scrubvae_amd.eval import HDBSCAN
    with pytest.raises(err):
        HDBSCAN(**kw).fit(X)


def test_constructor_is_sklearns():
    import inspect
    from scrubvae_amd.eval import HDBSCAN
    params = inspect.signature(HDBSCAN.__init__).parameters
    want = dict(min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, max_cluster_size=None, metric="euclidean",
                metric_params=None, alpha=1.0, algorithm="auto", leaf_size=40, n_jobs=None, cluster_selection_method="eom",
                allow_single_cluster=False, store_centers=None, copy=False)
    assert [p for p in params if p != "self"] == list(want)
    assert all(params[k].default == v for k, v in want.items())
