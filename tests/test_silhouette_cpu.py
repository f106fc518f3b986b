"""The silhouette without a GPU: the restatement of tests/silhouette_checks.py pinned to sklearn within the derived gate of the
long-double truth, the zero rules, argument errors raised before any device work, and the C-ABI exports."""
import numpy as np
import pytest
import torch

from tests import silhouette_checks as SC

needs_longdouble = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63,
                                      reason="np.longdouble is no wider than fp64 here: no truth to hold the value to")


def with_noise(y):
    """the labels with cluster 0 renamed -1: sklearn treats -1 as one more cluster"""
    return np.where(y == 0, -1, y)


@needs_longdouble
@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("n,d,K", SC.SIZES)
def test_restatement_and_sklearn_sit_inside_the_gate(n, d, K, noise):
    sm = pytest.importorskip("sklearn.metrics")
    x, y, p, g = SC.case(n, d, K)
    if noise:
        y = with_noise(y)
        p, g = SC.parts(x, y), SC.gate(x, y)
    sk = sm.silhouette_samples(x, y)
    e_own, e_sk = SC.err(p.s, g.truth.s), SC.err(sk, g.truth.s)
    print(f"silhouette n={n} d={d} K={K} noise={noise}: restatement {np.max(e_own / g.u):.2f} u, sklearn {np.max(e_sk / g.u):.2f} u, "
          f"gate {2 * (n + 4)} u, largest error / gate {max(np.max(e_own / g.tol_s), np.max(e_sk / g.tol_s)):.4f}")
    assert (e_own <= g.tol_s).all() and (e_sk <= g.tol_s).all()
    assert (np.abs(p.s - sk) <= 2 * g.tol_s).all()
    assert (SC.err(p.a, g.truth.a) <= g.tol_a).all() and (SC.err(p.b, g.truth.b) <= g.tol_b).all()
    assert np.array_equal(p.nearest, g.truth.nearest)
    score = sm.silhouette_score(x, y)
    assert abs(float(np.longdouble(score) - g.score)) <= g.tol_score
    assert abs(float(np.longdouble(p.s.mean()) - g.score)) <= g.tol_score


def test_the_700_case_is_the_one_described():
    _, y, p, _ = SC.case(700, 4, 300)
    assert len(p.uniq) == 262 and int((p.count == 1).sum()) == 63 and p.uniq.max() > 255


def test_a_row_alone_in_its_cluster_scores_zero():
    sm = pytest.importorskip("sklearn.metrics")
    x, y = SC.blobs(40, 3, 3, 1)
    y = y.copy()
    y[7] = 9
    p = SC.parts(x, y)
    assert p.s[7] == 0.0 and p.a[7] == 0.0 and p.b[7] > 0
    assert sm.silhouette_samples(x, y)[7] == 0.0
    assert SC.medoids(p)[list(p.uniq).index(9)] == 7


def test_all_rows_equal_score_zero():
    sm = pytest.importorskip("sklearn.metrics")
    x = np.tile(np.array([[1.5, -2.0, 0.25]]), (10, 1))
    y = np.array([0] * 6 + [1] * 4)
    p = SC.parts(x, y)
    assert (p.s == 0).all() and (p.a == 0).all() and (p.b == 0).all() and np.isfinite(p.s.mean())
    assert (sm.silhouette_samples(x, y) == 0).all()


XS, YS = SC.blobs(12, 2, 3, 0)


@pytest.mark.parametrize("z,labels,kwargs", [
    (XS[0], YS, {}),                                          # 1-D
    (XS[None], YS, {}),                                       # 3-D
    (np.where(np.arange(24).reshape(12, 2) == 5, np.nan, XS), YS, {}),
    (np.where(np.arange(24).reshape(12, 2) == 5, np.inf, XS), YS, {}),
    (XS, YS[:-1], {}),                                        # labels too short
    (XS, np.zeros((12, 1), dtype=np.int64), {}),              # labels not 1-D
    (XS, YS.astype(np.float64), {}),                          # labels not integers
    (XS, np.zeros(12, dtype=np.int64), {}),                   # one cluster
    (XS, np.arange(12), {}),                                  # n clusters
    (XS, np.where(np.arange(12) < 6, 0, -1), dict(noise_label=-1)),           # one cluster after the filter
    (XS, np.array([0, 1, 2] + [-1] * 9), dict(noise_label=-1)),               # as many clusters as kept rows
    (XS, np.full(12, -1), dict(noise_label=-1)),                              # nothing kept
    (torch.from_numpy(XS), torch.zeros(12, dtype=torch.int32), {}),
])
def test_argument_errors_before_device_work(z, labels, kwargs):
    """this machine has no device: a ValueError, not the "no device is available" RuntimeError, shows the order"""
    import scrubvae_amd.eval as E
    for fn in (E.silhouette_samples, E.silhouette_score, E.cluster_silhouette, E.cluster_medoids):
        with pytest.raises(ValueError):
            fn(z, labels, **kwargs)


def test_too_many_clusters_is_an_error():
    from scrubvae_amd.eval import silhouette as SM
    n = SM.SIL_MAX_CLUSTERS + 2
    z = np.zeros((n, 1))
    labels = np.arange(n)
    labels[-1] = 0                  # 4097 clusters among 4098 rows: sklearn's condition holds, the cap does not
    with pytest.raises(ValueError, match="4096"):
        SM.silhouette_samples(z, labels)


def test_check_maps_labels_and_filters_noise():
    from scrubvae_amd.eval import silhouette as SM
    x, y = SC.blobs(50, 3, 4, 3)
    y = np.array([-1, 7, 10 ** 9, 3])[y]
    rows, lab, count, uniq, keep, n = SM._sil_check(x.astype(np.float32), torch.from_numpy(y), None)
    assert rows.dtype == np.float64 and np.array_equal(rows, x) and keep is None and n == 50
    assert lab.dtype == np.int32 and count.dtype == np.int32 and np.array_equal(uniq, [-1, 3, 7, 10 ** 9])
    assert np.array_equal(uniq[lab], y) and np.array_equal(count, np.bincount(lab))
    rows, lab, count, uniq, keep, n = SM._sil_check(torch.from_numpy(x), y.astype(np.int64), -1)
    assert np.array_equal(keep, np.flatnonzero(y != -1)) and np.array_equal(rows.numpy(), x[keep])
    assert np.array_equal(uniq, [3, 7, 10 ** 9]) and np.array_equal(uniq[lab], y[keep]) and count.sum() == len(keep)


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import silhouette as SM
    lib = _lib.lib()
    work = lib.svae_silhouette_work
    assert work(2, 2, 2) == 0 and work(1, 0, 2) == 0            # n < 3
    assert work(10, 10, 1) == 0 and work(10, 10, 0) == 0        # K < 2
    assert work(5000, 5000, _lib.SIL_MAX_CLUSTERS + 1) == 0
    assert work(0, 10, 2) == 0 and work(-3, 10, 2) == 0         # rows < 1
    assert work(11, 10, 2) == 0                                 # more rows than there are
    # column chunks x rows padded to 64 x clusters padded to the 16, 64 or 256 columns of a block
    assert work(3, 3, 2) == 1 * 64 * 16
    assert work(301, 301, 5) == 5 * 320 * 16                    # 5 column tiles, one chunk each
    assert work(128, 1037, 4) == 6 * 128 * 16                   # 17 column tiles, at most 8 chunks: 6 of 3 tiles
    assert work(700, 700, 262) == 6 * 704 * 512                 # two chunks of 256 clusters, 11 column tiles in 6 chunks of 2
    assert work(32768, 131072, 25) == 1 * 32768 * 64            # 512 row tiles: the block's sums are final
    assert work(4096, 4096, _lib.SIL_MAX_CLUSTERS) == 1 * 4096 * 4096
    import scrubvae_amd.eval as E
    for name in ("silhouette_samples", "silhouette_score", "cluster_silhouette", "cluster_medoids"):
        assert callable(getattr(E, name))
    assert _lib.SIL_MAX_CLUSTERS == 4096
    assert SM._SIL_CALLS.keys() >= {"silhouette", "mean", "medoids"} and SM._SIL_ROWS_PER_LAUNCH % 64 == 0
    assert SM.SilhouetteParts._fields == ("s", "a", "b", "nearest")
