"""Gaussian mixture clustering on the device (scrubvae_amd/eval/cluster.py, csrc/gmm.hip) against the fp64 restatement of
tests/gmm_checks.py."""
import pickle

import numpy as np
import pytest
import torch

from tests import gmm_checks as GC

pytestmark = pytest.mark.gpu


def planted(n, d, K, seed):
    """float32 latents: K clusters with column offsets |mean| >> std, a constant column, a duplicated column and one tight
    component (std 1e-3) about 30 units from the global mean"""
    g = np.random.default_rng(seed)
    centers = g.normal(size=(K, d)) * 3.0
    lab = g.integers(0, K, n)
    scale = np.exp(0.3 * g.normal(size=(K, d)))
    x = centers[lab] + g.normal(size=(n, d)) * scale[lab]
    t = lab == 0
    shift = g.normal(size=d)
    x[t] = 30.0 * shift / np.linalg.norm(shift) + 1e-3 * g.normal(size=(int(t.sum()), d))
    x += 50.0 * np.sign(g.normal(size=d))
    x[:, 0] = 3.0
    x[:, 1] = x[:, 2]
    return x.astype(np.float32)


def _bound(a):
    return np.abs(a).max()


@pytest.mark.parametrize("n,d,K", [(20011, 32, 25), (5003, 128, 64)])
def test_kmeans_pp_seeds_equal_restatement(n, d, K):
    from scrubvae_amd.eval import cluster as C
    x = planted(n, d, 6, seed=d)
    for seed in (0, 1):
        R = C._Rows(torch.from_numpy(x).cuda(), K, False, torch.device("cuda"))
        got = R.kmeans_pp(C.check_random_state(seed))
        ref = GC.kmeans_pp(x.astype(np.float64), K, GC.check_random_state(seed))
        assert np.array_equal(got, ref), (seed, got, ref)


def _compare_params(got, ref, x64, diag):
    scale = _bound(x64)
    assert np.abs(got[0] - ref[0]).max() <= 1e-9
    assert np.abs(got[1] - ref[1]).max() <= 1e-9 * scale
    for k in range(len(ref[0])):
        cov_r = ref[2][k]
        dmax = cov_r.max() if diag else np.diag(cov_r).max()
        assert np.abs(got[2][k] - cov_r).max() <= 1e-9 * dmax, k
        P_r = ref[3][k]
        pmax = P_r.max() if diag else np.diag(P_r).max()
        assert np.abs(got[3][k] - P_r).max() <= 1e-9 * pmax, k


@pytest.mark.parametrize("n,d,K,cov", [(20011, 32, 25, "full"), (20011, 32, 25, "diag"), (8009, 128, 8, "full")])
def test_fit_matches_restatement(n, d, K, cov):
    from scrubvae_amd.eval import GaussianMixture
    x = planted(n, d, 8, seed=n + d)
    x64 = x.astype(np.float64)
    diag = cov == "diag"
    m = GaussianMixture(K, covariance_type=cov, random_state=3)
    labels = m.fit_predict(torch.from_numpy(x).cuda())
    ref = GC.fit(x64, K, diag=diag, random_state=3)
    assert np.array_equal(GC.kmeans_pp(x64, K, GC.check_random_state(3)), ref["seeds"])
    assert m.n_iter_ == ref["n_iter"] and m.converged_ == ref["converged"]
    assert abs(m.lower_bound_ - ref["lower_bound"]) <= 1e-10 * abs(ref["lower_bound"])
    assert len(m.lower_bounds_) == m.n_iter_
    for a in (m.weights_, m.means_, m.covariances_, m.precisions_cholesky_):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64
    assert m.covariances_.shape == ((K, d) if diag else (K, d, d)) and m.means_.shape == (K, d) and m.n_features_in_ == d
    _compare_params((m.weights_, m.means_, m.covariances_, m.precisions_cholesky_),
                    (ref["weights"], ref["means"], ref["covariances"], ref["precisions_cholesky"]), x64, diag)
    clear = GC.top_gap(x64, ref, diag) > 1e-6
    assert clear.mean() > 0.99
    assert np.array_equal(labels[clear], ref["labels"][clear])


@pytest.mark.parametrize("cov", ["full", "diag"])
def test_one_em_step_at_large_n(cov):
    from scrubvae_amd.eval import cluster as C
    n, d, K = 262147, 64, 25
    diag = cov == "diag"
    x = planted(n, d, K, seed=5)
    x64 = x.astype(np.float64)
    g = np.random.default_rng(6)
    means = x64[g.choice(n, K, replace=False)] + 0.1 * g.normal(size=(K, d))
    weights = g.uniform(0.5, 1.5, K)
    weights /= weights.sum()
    if diag:
        P = 1.0 / np.sqrt(g.uniform(0.5, 2.0, (K, d)))
    else:
        P = np.triu(0.1 * g.normal(size=(K, d, d)), 1) + np.stack([np.diag(g.uniform(0.5, 2.0, d)) for _ in range(K)])
    got = C.em_step(torch.from_numpy(x).cuda(), weights, means, P, covariance_type=cov, reg_covar=1e-6)
    lpn, resp = GC.estep(x64, weights, means, P, diag)
    ref = GC.mstep(x64, resp, 1e-6, diag)
    assert abs(got[0] - lpn.mean()) <= 1e-10 * abs(lpn.mean())
    _compare_params(got[1:], ref, x64, diag)


def test_fit_is_bit_reproducible():
    from scrubvae_amd.eval import GaussianMixture
    x = torch.from_numpy(planted(20011, 32, 8, seed=9)).cuda()
    outs = []
    for _ in range(2):
        m = GaussianMixture(25, random_state=11)
        lab = m.fit_predict(x)
        outs.append((lab, m.weights_, m.means_, m.covariances_, m.precisions_cholesky_, m.lower_bounds_))
    for a, b in zip(*outs):
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("cov", ["full", "diag"])
def test_predict_paths_match_restatement(cov):
    from scrubvae_amd.eval import GaussianMixture
    diag = cov == "diag"
    x = planted(20011, 32, 8, seed=13)
    new = planted(7001, 32, 8, seed=13)[::-1].copy()
    m = GaussianMixture(12, covariance_type=cov, random_state=2).fit(x)
    f = dict(weights=m.weights_, means=m.means_, precisions_cholesky=m.precisions_cholesky_)
    new64 = new.astype(np.float64)
    clear = GC.top_gap(new64, f, diag) > 1e-6
    assert np.array_equal(m.predict(new)[clear], GC.predict(new64, f, diag)[clear])
    proba = m.predict_proba(torch.from_numpy(new).cuda())
    assert proba.shape == (len(new), 12)
    assert np.abs(proba.sum(1) - 1.0).max() <= 1e-12
    assert np.abs(proba - GC.predict_proba(new64, f, diag)).max() <= 1e-9
    ss = m.score_samples(new)
    ref_ss = GC.score_samples(new64, f, diag)
    assert np.abs(ss - ref_ss).max() <= 1e-9 * np.abs(ref_ss).max()
    assert abs(m.score(new) - ss.mean()) <= 1e-12 * abs(ss.mean())
    assert np.array_equal(GaussianMixture(12, covariance_type=cov, random_state=2).fit_predict(x), m.predict(x))
    m2 = pickle.loads(pickle.dumps(m))
    assert np.array_equal(m2.predict(new), m.predict(new))


class _SklearnLike:
    """carries only sklearn's fitted attribute names"""


def test_gmm_round_trip(tmp_path):
    from scrubvae_amd.eval import GaussianMixture, gmm
    x = planted(20011, 32, 8, seed=17)
    path = str(tmp_path) + "/"
    k1, m1 = gmm(x, label="a", path=path, n_components=10, random_state=4)
    assert (tmp_path / "a_gmm.p").exists() and (tmp_path / "a_gmm.npy").exists()
    assert isinstance(m1, GaussianMixture) and m1.n_iter_ <= 150
    k2, m2 = gmm(x, label="a", path=path, n_components=10, random_state=4)
    assert np.array_equal(k1, k2) and np.array_equal(m1.means_, m2.means_)
    assert np.array_equal(k1, m1.predict(x))
    x64 = x.astype(np.float64)
    ref = GC.fit(x64, 10, reg=1e-5, max_iter=150, random_state=4)
    stand_in = _SklearnLike()
    stand_in.covariance_type = "full"
    stand_in.weights_, stand_in.means_, stand_in.precisions_cholesky_ = ref["weights"], ref["means"], ref["precisions_cholesky"]
    with open(tmp_path / "b_gmm.p", "wb") as f:
        pickle.dump(stand_in, f)
    k3, m3 = gmm(x, label="b", path=path, n_components=10)
    assert isinstance(m3, _SklearnLike) and (tmp_path / "b_gmm.npy").exists()
    clear = GC.top_gap(x64, ref, False) > 1e-6
    assert np.array_equal(k3[clear], ref["labels"][clear])


@pytest.mark.parametrize("cov", ["full", "diag"])
def test_not_positive_definite_raises(cov):
    from scrubvae_amd.eval import GaussianMixture
    from scrubvae_amd.eval import cluster as C
    x = planted(5003, 16, 4, seed=21)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        GaussianMixture(4, covariance_type=cov, reg_covar=0.0, random_state=0).fit(x)
    # the M-step itself: the constant column's variance is exactly 0 in every component
    m = GaussianMixture(4, covariance_type=cov, random_state=0).fit(x)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        C.em_step(x, m.weights_, m.means_, m.precisions_cholesky_, covariance_type=cov, reg_covar=0.0)
