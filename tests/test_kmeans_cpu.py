"""CPU checks of the k-means clustering: the fp64 restatement of tests/kmeans_checks.py against sklearn (whole fits, the relocation
of empty clusters, the random draws), the refusals that come before the device, the cached kmeans() path, the C ABI declarations
and the argument checks of the exports."""
import pickle

import numpy as np
import pytest

from tests import abi_header as ABI
from tests import kmeans_checks as KC


def _datasets():
    g = np.random.default_rng(0)
    a = g.normal(size=(1000, 8))
    b = a + (g.normal(size=(6, 8)) * 4.0)[g.integers(0, 6, 1000)]
    c = g.normal(size=(700, 5)).astype(np.float32).astype(np.float64)
    return {"normal": a, "planted": b, "fp32": c}


DATA = _datasets()


@pytest.mark.parametrize("init,n_init", [("k-means++", 1), ("random", 3)])
@pytest.mark.parametrize("K", [2, 5, 17])
@pytest.mark.parametrize("name", sorted(DATA))
def test_restatement_equals_sklearn(name, K, init, n_init):
    skc = pytest.importorskip("sklearn.cluster")
    X = DATA[name]
    for seed in range(4):
        ref = skc.KMeans(K, init=init, n_init=n_init, random_state=seed, algorithm="lloyd").fit(X)
        f = KC.fit(X, K, init=init, n_init=n_init, random_state=seed)
        assert np.array_equal(f["labels"], ref.labels_) and f["n_iter"] == ref.n_iter_, seed
        assert np.abs(f["centers"] - ref.cluster_centers_).max() <= KC.centre_gate(X), seed
        assert abs(f["inertia"] - ref.inertia_) <= KC.inertia_gate(len(X)) * ref.inertia_, seed


def _far_init(X, K, n_far, seed):
    """K init centres: rows of X, the last n_far of them moved far from every row (their clusters start empty)"""
    g = np.random.default_rng(seed)
    C = X[g.choice(len(X), K, replace=False)].copy()
    for i in range(n_far):
        C[K - 1 - i] += 1000.0 * (i + 1)
    return C


def test_one_empty_cluster_ends_with_sklearns_labels():
    skc = pytest.importorskip("sklearn.cluster")
    X = DATA["planted"]
    for seed in range(3):
        C = _far_init(X, 5, 1, seed)
        ref = skc.KMeans(5, init=C, n_init=1, algorithm="lloyd").fit(X)
        trace = []
        f = KC.fit(X, 5, init=C, trace=trace)
        assert trace[0]["n_empty"] == 1
        assert np.array_equal(f["labels"], ref.labels_) and f["n_iter"] == ref.n_iter_
        assert np.abs(f["centers"] - ref.cluster_centers_).max() <= KC.centre_gate(X)


def test_two_empty_clusters_follow_the_rule():
    X = DATA["planted"][:300]
    Xc = X - X.mean(0)
    C = _far_init(Xc, 6, 2, 1)
    st = KC.lloyd_step(Xc, C)
    assert st["n_empty"] == 2
    labels, dist = st["labels"], st["dist"]
    far = sorted(range(len(Xc)), key=lambda r: (-dist[r], r))[:2]
    assert list(KC.relocation_rows(dist, 2)) == far
    # the empty clusters, in ascending order, hold exactly those rows; their old clusters lost them
    assert np.array_equal(st["centers"][4], Xc[far[0]]) and np.array_equal(st["centers"][5], Xc[far[1]])
    counts = np.bincount(labels, minlength=6).astype(float)
    for r in far:
        counts[labels[r]] -= 1
    counts[4:] = 1
    assert np.array_equal(st["sums"][:, -1], counts)
    # equal distances: the lower row first
    tied = np.array([1.0, 3.0, 3.0, 2.0, 3.0])
    assert list(KC.relocation_rows(tied, 2)) == [1, 2]
    from scrubvae_amd.eval import cluster
    assert list(cluster._relocation_rows(tied, 2)) == [1, 2] and list(cluster._relocation_rows(dist, 2)) == far
    f = KC.fit(X, 6, init=C + X.mean(0))
    assert len(np.unique(f["labels"])) == 6


@pytest.mark.parametrize("init,n_init", [("k-means++", 1), ("random", 3)])
def test_random_state_consumption_equals_sklearn(init, n_init):
    skc = pytest.importorskip("sklearn.cluster")
    X = DATA["fp32"]
    r_ref, r_mine = np.random.RandomState(11), np.random.RandomState(11)
    skc.KMeans(5, init=init, n_init=n_init, random_state=r_ref, algorithm="lloyd").fit(X)
    KC.fit(X, 5, init=init, n_init=n_init, random_state=r_mine)
    assert r_ref.uniform() == r_mine.uniform()


def test_is_same_clustering():
    from scrubvae_amd.eval import cluster
    a = np.array([0, 0, 1, 2, 2, 1])
    for same in (cluster._is_same_clustering, KC.is_same_clustering):
        assert same(a, np.array([2, 2, 0, 1, 1, 0]), 3)
        assert not same(a, np.array([2, 1, 0, 1, 1, 0]), 3)


def _forbid_device(monkeypatch):
    import torch
    from scrubvae_amd.eval import cluster

    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(cluster, "_km_device_of", boom)
    monkeypatch.setattr(cluster, "_device_of", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)


@pytest.mark.parametrize("kwargs,x", [
    (dict(n_clusters=3), np.zeros((2, 4))),                                            # n < K
    (dict(n_clusters=0), None),
    (dict(n_clusters=1025), np.zeros((2000, 2))),
    (dict(n_clusters=2), np.zeros((10, 129))),
    (dict(n_clusters=2), np.array([[0.0, 1.0], [np.nan, 2.0], [1.0, 1.0]])),
    (dict(n_clusters=2), np.array([[0.0, 1.0], [np.inf, 2.0], [1.0, 1.0]])),
    (dict(n_clusters=2), np.array([[0.0, 1.0], [1e300, 2.0], [1.0, 1.0]])),            # overflows fp32
    (dict(n_clusters=2, init=np.zeros((3, 3))), None),                                 # wrong number of centres
    (dict(n_clusters=2, init=np.zeros((2, 4))), None),                                 # wrong width
    (dict(n_clusters=2, n_init=0), None),
    (dict(n_clusters=2, max_iter=0), None),
    (dict(n_clusters=2, init="kmeans"), None),
])
def test_value_errors_before_the_device(monkeypatch, kwargs, x):
    from scrubvae_amd.eval import KMeans
    _forbid_device(monkeypatch)
    if x is None:
        x = np.random.default_rng(0).normal(size=(50, 3))
    with pytest.raises(ValueError):
        KMeans(**kwargs).fit(x)


def test_without_device_raises_runtime_error(monkeypatch):
    import torch
    from scrubvae_amd.eval import KMeans
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.random.default_rng(0).normal(size=(50, 3))
    with pytest.raises(RuntimeError):
        KMeans(2).fit(x)
    m = KMeans(2)
    with pytest.raises(RuntimeError):
        m.predict(x)  # not fitted
    m.cluster_centers_, m.n_features_in_ = np.zeros((2, 3)), 3
    for method in (m.predict, m.transform, m.score):
        with pytest.raises(RuntimeError):
            method(x)


def test_kmeans_loads_both_cached_files_without_device(monkeypatch, tmp_path):
    from scrubvae_amd.eval import KMeans, kmeans
    _forbid_device(monkeypatch)
    m = KMeans(3, random_state=0)
    m.cluster_centers_, m.n_features_in_ = np.arange(6.0).reshape(3, 2), 2
    labels = np.array([0, 2, 1, 1])
    with open(tmp_path / "z_kmeans.p", "wb") as f:
        pickle.dump(m, f)
    np.save(tmp_path / "z_kmeans.npy", labels)
    k_pred, model = kmeans(np.zeros((4, 2), np.float32), label="z", path=str(tmp_path) + "/")
    assert np.array_equal(k_pred, labels)
    assert isinstance(model, KMeans) and np.array_equal(model.cluster_centers_, m.cluster_centers_)


def test_abi_names_and_exports():
    from scrubvae_amd import _lib, build
    import scrubvae_amd.eval as E
    assert ABI.declared("svae_kmeans_") == {"svae_kmeans_assign_blocks", "svae_kmeans_assign_f64", "svae_kmeans_chunks",
                                            "svae_kmeans_update_f64", "svae_kmeans_finish_f64"}
    assert _lib.KMEANS_MAX_CLUSTERS == 1024
    assert "kmeans.hip" in build.SOURCES
    for name in ("KMeans", "kmeans"):
        assert callable(getattr(E, name))


def test_block_and_chunk_helpers():
    from scrubvae_amd import _lib
    lib = _lib.lib()
    blocks, chunks = lib.svae_kmeans_assign_blocks, lib.svae_kmeans_chunks
    assert blocks(0) == 0 and blocks(-1) == 0 and blocks(1) == 1 and blocks(64) == 1 and blocks(65) == 2
    assert chunks(0, 4, 2) == 0 and chunks(10, 0, 2) == 0 and chunks(10, 129, 2) == 0 and chunks(10, 4, 0) == 0 and chunks(10, 4, 1025) == 0
    # units of 256 rows, one chunk per unit up to 1024 chunks
    assert chunks(256, 4, 2) == 1 and chunks(257, 4, 2) == 2 and chunks(512, 4, 2) == 2 and chunks(513, 4, 2) == 3
    assert chunks(1000000, 32, 100) == 977      # 3907 units in 1024 parts: 4 units each
    # at most 2^24 doubles of partials: 2^24 // (1024 * 129) = 127 chunks wanted, 40 units in chunks of 1
    assert chunks(10000, 128, 1024) == 40 and chunks(1000000, 128, 1024) == 127


def test_argument_errors():
    from scrubvae_amd import _lib
    lib = _lib.lib()
    fake = 4096
    E = _lib.ERR_ARG

    def assign(A=fake, lda=16, d=4, n=100, C=fake, ldc=4, K=3, prev=None, label=fake, dist=fake, gap=None, D=None, part=None, changed=None):
        return lib.svae_kmeans_assign_f64(A, lda, d, n, C, ldc, K, prev, label, dist, gap, D, part, changed, None)

    for bad in (dict(A=None), dict(C=None), dict(K=0), dict(K=1025), dict(d=129, lda=144, ldc=129), dict(d=0), dict(n=0), dict(n=-5),
                dict(lda=4), dict(ldc=3), dict(label=None, dist=None), dict(changed=fake), dict(prev=fake, label=fake)):
        assert assign(**bad) == E, bad
        assert "kmeans_assign_f64" in _lib.last_error()

    def update(A=fake, lda=16, d=4, n=100, label=fake, K=3, part=fake, sums=fake):
        return lib.svae_kmeans_update_f64(A, lda, d, n, label, K, part, sums, None)

    for bad in (dict(A=None), dict(label=None), dict(part=None), dict(sums=None), dict(K=0), dict(K=1025), dict(d=129, lda=144), dict(n=0)):
        assert update(**bad) == E, bad
        assert "kmeans_update_f64" in _lib.last_error()

    def finish(sums=fake, d=4, K=3, C_old=fake, C_new=2 * fake, ldc=4, changed=None, rec=fake):
        return lib.svae_kmeans_finish_f64(sums, d, K, C_old, C_new, ldc, changed, rec, None)

    for bad in (dict(sums=None), dict(C_old=None), dict(C_new=None), dict(rec=None), dict(C_new=fake), dict(K=0), dict(K=1025), dict(d=129),
                dict(d=0), dict(ldc=3)):
        assert finish(**bad) == E, bad
        assert "kmeans_finish_f64" in _lib.last_error()
