"""CPU checks of the Gaussian mixture clustering: the fp64 restatement of tests/gmm_checks.py against sklearn, cluster_entropy
against the reference loop, the C ABI declarations, the exports, argument checks and the cached gmm() path."""
import pickle

import numpy as np
import pytest

from tests import gmm_checks as GC


def planted64(n, d, K, seed, spread=5.0):
    g = np.random.default_rng(seed)
    centers = g.normal(size=(K, d)) * spread
    lab = g.integers(0, K, n)
    scale = np.exp(0.3 * g.normal(size=(K, d)))
    return centers[lab] + g.normal(size=(n, d)) * scale[lab]


@pytest.mark.parametrize("K", [2, 25, 64])
@pytest.mark.parametrize("seed", [0, 7, 123])
def test_kmeans_pp_seeds_equal_sklearn(K, seed):
    skc = pytest.importorskip("sklearn.cluster")
    x = planted64(3000, 8, 6, seed=K + seed)
    _, ref = skc.kmeans_plusplus(x, K, random_state=seed)
    mine = GC.kmeans_pp(x, K, GC.check_random_state(seed))
    assert np.array_equal(mine, ref)


@pytest.mark.parametrize("cov", ["full", "diag"])
@pytest.mark.parametrize("seed", [1, 2])
def test_em_restatement_equals_sklearn(cov, seed):
    skm = pytest.importorskip("sklearn.mixture")
    x = planted64(3000, 6, 5, seed=seed)
    ref = skm.GaussianMixture(5, covariance_type=cov, init_params="k-means++", random_state=seed).fit(x)
    ref_labels = skm.GaussianMixture(5, covariance_type=cov, init_params="k-means++", random_state=seed).fit_predict(x)
    f = GC.fit(x, 5, diag=cov == "diag", random_state=seed)
    assert f["n_iter"] == ref.n_iter_ and f["converged"] == ref.converged_
    assert abs(f["lower_bound"] - ref.lower_bound_) <= 1e-10 * abs(ref.lower_bound_)
    for mine, theirs in ((f["weights"], ref.weights_), (f["means"], ref.means_), (f["covariances"], ref.covariances_),
                         (f["precisions_cholesky"], ref.precisions_cholesky_)):
        assert np.abs(mine - theirs).max() <= 1e-8
    assert np.array_equal(f["labels"], ref_labels)
    assert np.array_equal(GC.predict(x, f, cov == "diag"), ref.predict(x))
    assert np.abs(GC.predict_proba(x, f, cov == "diag") - ref.predict_proba(x)).max() <= 1e-8
    assert np.abs(GC.score_samples(x, f, cov == "diag") - ref.score_samples(x)).max() <= 1e-8


def test_cluster_entropy_equals_reference_loop():
    from scrubvae_amd.eval import cluster_entropy
    g = np.random.default_rng(3)
    k0 = g.integers(2, 9, 5000)          # reference labels that do not start at 0
    k1 = g.integers(0, 6, 5000)
    k1[k1 == 4] = 5                     # cluster 4 is empty
    for n_components in (6, 7):
        got = cluster_entropy(k0, k1, n_components)
        ref = GC.cluster_entropy_literal(k0, k1, n_components)
        assert isinstance(got, float) and got == ref
    assert cluster_entropy(k0, k0 - 2, 7) == 0.0


def test_abi_names_and_exports():
    import scrubvae_amd.eval as E
    for name in ("gmm", "GaussianMixture", "cluster_entropy"):
        assert callable(getattr(E, name))


def _forbid_device(monkeypatch):
    import torch
    from scrubvae_amd.eval import cluster

    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(cluster, "_device_of", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)


@pytest.mark.parametrize("kwargs,x", [
    (dict(covariance_type="tied"), None),
    (dict(covariance_type="spherical"), None),
    (dict(init_params="kmeans"), None),
    (dict(init_params="random"), None),
    (dict(n_init=2), None),
    (dict(n_components=65), np.zeros((100, 4))),
    (dict(n_components=3), np.zeros((2, 4))),
    (dict(n_components=1), np.zeros((1, 4))),
    (dict(n_components=2), np.zeros((10, 129))),
    (dict(n_components=2), np.array([[0.0, 1.0], [np.nan, 2.0], [1.0, 1.0]])),
    (dict(n_components=2), np.array([[0.0, 1.0], [np.inf, 2.0], [1.0, 1.0]])),
    (dict(n_components=2), np.array([[0.0, 1.0], [1e300, 2.0], [1.0, 1.0]])),  # overflows fp32
])
def test_value_errors_before_the_device(monkeypatch, kwargs, x):
    from scrubvae_amd.eval import GaussianMixture
    _forbid_device(monkeypatch)
    if x is None:
        x = np.random.default_rng(0).normal(size=(50, 3))
    with pytest.raises(ValueError):
        GaussianMixture(**kwargs).fit(x)


def test_without_device_raises_runtime_error(monkeypatch):
    import torch
    from scrubvae_amd.eval import GaussianMixture
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.random.default_rng(0).normal(size=(50, 3))
    with pytest.raises(RuntimeError):
        GaussianMixture(2).fit(x)
    m = GaussianMixture(2)
    m.weights_, m.means_, m.precisions_cholesky_, m.n_features_in_ = np.ones(2) / 2, np.zeros((2, 3)), np.stack([np.eye(3)] * 2), 3
    with pytest.raises(RuntimeError):
        m.predict(x)


def test_gmm_loads_both_cached_files_without_device(monkeypatch, tmp_path):
    from scrubvae_amd.eval import GaussianMixture, gmm
    _forbid_device(monkeypatch)
    m = GaussianMixture(3, random_state=0)
    m.weights_, m.means_ = np.ones(3) / 3, np.arange(6.0).reshape(3, 2)
    labels = np.array([0, 2, 1, 1])
    with open(tmp_path / "z_gmm.p", "wb") as f:
        pickle.dump(m, f)
    np.save(tmp_path / "z_gmm.npy", labels)
    k_pred, model = gmm(np.zeros((4, 2), np.float32), label="z", path=str(tmp_path) + "/")
    assert np.array_equal(k_pred, labels)
    assert isinstance(model, GaussianMixture) and np.array_equal(model.means_, m.means_)
