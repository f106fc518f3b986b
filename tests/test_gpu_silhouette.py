"""silhouette_samples / silhouette_score / cluster_silhouette / cluster_medoids (csrc/silhouette.hip) on the device against the numpy
restatement of tests/silhouette_checks.py.

Every s_i, a_i, b_i and the score are held to the derived gate of silhouette_checks (|s_i - truth_i| <= 2 (n + 4) u_i, truth in
np.longdouble, u_i = 2^-53 (a_i + b_i) / max(a_i, b_i)); the sizes are the smallest that reach each path of the kernels: the 16-,
64- and 256-column instantiations, two chunks of 256 clusters, partial tiles and feature chunks, rows not resident in LDS, several
column tiles per block, several row ranges per call."""
import numpy as np
import pytest
import torch

from tests import silhouette_checks as SC
from tests.test_gpu_mmd import needs_longdouble

pytestmark = pytest.mark.gpu

MINIMUM = (np.array([[0.0, 0.0], [3.0, 4.0], [1.0, 0.0]]), np.array([0, 1, 0]))


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same_parts(p, q):
    return all(bits(u) == bits(v) for u, v in zip(p, q))


def report(name, got, g, score):
    """the worst device error in u_i, then the largest error / gate of s, a, b and the score"""
    es, ea, eb = SC.err(got.s, g.truth.s), SC.err(got.a, g.truth.a), SC.err(got.b, g.truth.b)
    e_score = abs(float(np.longdouble(score) - g.score))
    worst = int(np.argmax(es / g.u))
    ratio = lambda e, t: float(np.max(np.where(t > 0, e / np.where(t > 0, t, 1), np.where(e > 0, np.inf, 0))))
    print(f"silhouette {name}: worst device error {es[worst] / g.u[worst]:.2f} u (gate {g.tol_s[worst] / g.u[worst]:.0f} u), largest "
          f"error / gate s {ratio(es, g.tol_s):.4f} a {ratio(ea, g.tol_a):.4f} b {ratio(eb, g.tol_b):.4f} "
          f"score {e_score / g.tol_score:.4f}")
    return es, ea, eb, e_score


def check_values(name, x, y):
    from scrubvae_amd.eval import silhouette_samples, silhouette_score
    g = SC.gate(x, y)
    got = silhouette_samples(x, y, return_parts=True)
    score = silhouette_score(x, y)
    n = len(y)
    assert isinstance(score, float) and all(v.shape == (n,) for v in got)
    assert got.s.dtype == got.a.dtype == got.b.dtype == np.float64
    assert bits(silhouette_samples(x, y)) == bits(got.s)
    es, ea, eb, e_score = report(name, got, g, score)
    assert (es <= g.tol_s).all(), (int(np.argmax(es - g.tol_s)), float((es / g.u).max()))
    assert (ea <= g.tol_a).all() and (eb <= g.tol_b).all()
    assert e_score <= g.tol_score
    return got


@needs_longdouble
@pytest.mark.parametrize("n,d,K", SC.SIZES)
def test_every_value_within_the_derived_gate(n, d, K):
    x, y, _, _ = SC.case(n, d, K)
    check_values(f"n={n} d={d} K={K}", x, y)


@needs_longdouble
def test_the_minimum():
    x, y = MINIMUM
    got = check_values("n=3 d=2 labels [0, 1, 0]", x, y)
    assert got.s[1] == 0.0 and got.a[1] == 0.0  # alone in its cluster
    assert np.array_equal(got.nearest, [1, 0, 1]) and got.a[0] == 1.0 and got.b[0] == 5.0


def within_twice_the_gate(values, n):
    """the entries of `values` (restated, fp64) within twice their gate of the minimum"""
    return values - values.min() <= 2 * (n + 4) * SC.EPS * values


@pytest.mark.parametrize("n,d,K", SC.SIZES)
def test_nearest_and_medoids_are_the_restated_choices(n, d, K):
    from scrubvae_amd.eval import cluster_medoids, silhouette_samples
    x, y, p, _ = SC.case(n, d, K)
    got = silhouette_samples(x, y, return_parts=True)
    uniq, med = cluster_medoids(x, y)
    assert np.array_equal(uniq, p.uniq) and med.dtype == np.int64 and med.shape == uniq.shape
    assert got.nearest.dtype == p.uniq.dtype
    # nearest: per row the restated means of the other clusters
    other = p.S / p.count[None, :]
    loose = 0
    dev_near = np.searchsorted(p.uniq, got.nearest)
    for i in range(n):
        v = np.delete(other[i], p.inv[i])
        ids = np.delete(np.arange(len(p.uniq)), p.inv[i])
        cand = ids[within_twice_the_gate(v, n)]
        if len(cand) == 1:
            assert dev_near[i] == p.nearest[i] == cand[0], i
        else:
            loose += 1
            assert dev_near[i] in cand, i
    # medoids: per cluster the restated a of its rows
    restated = SC.medoids(p)
    loose_med = 0
    for c in range(len(p.uniq)):
        rows = np.flatnonzero(p.inv == c)
        assert p.inv[med[c]] == c
        # the device's own rule, exactly: the lowest row among the smallest of the device's a
        assert med[c] == rows[np.argmin(got.a[rows])], c
        cand = rows[within_twice_the_gate(p.a[rows], n)]
        structural = len(rows) == 2 or (x[cand] == x[cand[0]]).all()   # d_ij == d_ji, or duplicated rows: bit-equal on the device
        if len(cand) == 1 or structural:
            assert med[c] == restated[c] == cand.min(), c
            if len(cand) > 1:
                assert len(set(bits(got.a[r]) for r in cand)) == 1, c
        else:
            loose_med += 1
            assert med[c] in cand, c
    share = (loose + loose_med) / (n + len(p.uniq))
    print(f"silhouette n={n} d={d} K={K}: {loose} of {n} nearest and {loose_med} of {len(p.uniq)} medoids decided within twice the "
          f"gate only ({100 * share:.1f} % of the cases)")
    assert share <= 0.25


def test_two_calls_give_the_same_bits():
    from scrubvae_amd.eval import cluster_medoids, cluster_silhouette, silhouette_samples, silhouette_score
    for size in [(301, 3, 5), (700, 4, 300)]:
        x, y, _, _ = SC.case(*size)
        assert same_parts(silhouette_samples(x, y, return_parts=True), silhouette_samples(x, y, return_parts=True))
        assert bits(silhouette_score(x, y)) == bits(silhouette_score(x, y))
        assert same_parts(cluster_silhouette(x, y), cluster_silhouette(x, y))
        assert same_parts(cluster_medoids(x, y), cluster_medoids(x, y))


@pytest.mark.parametrize("n,d,K", [(301, 3, 5), (600, 8, 70), (700, 4, 300)])
def test_renaming_the_clusters_changes_no_bit(n, d, K):
    """a column's sum does not depend on its position, its id or the chunk of 256 it falls in"""
    from scrubvae_amd.eval import silhouette_samples, silhouette_score
    x, y, p, _ = SC.case(n, d, K)
    base = silhouette_samples(x, y, return_parts=True)
    k = len(p.uniq)
    g = np.random.default_rng(k)
    names = np.unique(np.concatenate([[-1, 7, 10 ** 9], g.choice(10 ** 9 - 10, k - 3, replace=False) + 8]))  # a non-contiguous mix
    assert len(names) == k
    perm = g.permutation(k)          # cluster c becomes names[perm[c]]: the order of the columns changes too
    renamed = names[perm][p.inv]
    for labels in (renamed.astype(np.int64), torch.from_numpy(renamed.astype(np.int64)), torch.from_numpy(renamed).cuda()):
        got = silhouette_samples(x, labels, return_parts=True)
        assert bits(got.s) == bits(base.s) and bits(got.a) == bits(base.a) and bits(got.b) == bits(base.b)
        # nearest follows the renaming, except on an exact tie of b (the lowest new column wins): none occurs in these inputs
        assert np.array_equal(got.nearest, names[perm][np.searchsorted(p.uniq, base.nearest)])
    if renamed.max() < 2 ** 31:
        got = silhouette_samples(x, renamed.astype(np.int32), return_parts=True)
        assert same_parts(got[:3], base[:3]) and got.nearest.dtype == np.int32
    # the score sums the same s in the same order
    assert bits(silhouette_score(x, renamed)) == bits(silhouette_score(x, y))


def test_non_contiguous_ids_and_label_kinds():
    from scrubvae_amd.eval import silhouette_samples
    x, y, _, _ = SC.case(301, 3, 5)
    base = silhouette_samples(x, y, return_parts=True)
    names = np.array([-1, 7, 10 ** 9, 10 ** 9 + 1, 2 ** 40])
    got = silhouette_samples(x, names[y], return_parts=True)
    assert same_parts(got[:3], base[:3]) and np.array_equal(got.nearest, names[base.nearest])
    small = np.array([-1, 7, 9, 100, 2 ** 31 - 1], dtype=np.int32)
    for labels in (small[y], torch.from_numpy(small[y]), torch.from_numpy(small[y]).cuda(), small[y].astype(np.int64)):
        got = silhouette_samples(x, labels, return_parts=True)
        assert same_parts(got[:3], base[:3]) and np.array_equal(got.nearest, small[base.nearest])


def test_input_kinds_give_the_same_bits():
    from scrubvae_amd.eval import cluster_medoids, silhouette_samples, silhouette_score
    x, y, _, _ = SC.case(130, 37, 3)   # float32-representable values
    base = silhouette_samples(x, y, return_parts=True)
    x32 = torch.from_numpy(x.astype(np.float32)).cuda()
    xt = torch.from_numpy(x.copy())   # the cached case is read-only
    for z in (x32, x.astype(np.float32), xt, xt.cuda()):
        assert same_parts(silhouette_samples(z, y, return_parts=True), base)
    assert bits(silhouette_score(x32, y)) == bits(silhouette_score(x, y))
    assert same_parts(cluster_medoids(x32, torch.from_numpy(y.copy()).cuda()), cluster_medoids(x, y))


@pytest.mark.parametrize("n,d,K", [(301, 3, 5), (700, 4, 300)])
def test_row_ranges_change_no_bit(n, d, K, monkeypatch):
    from scrubvae_amd.eval import silhouette as SM
    x, y, _, _ = SC.case(n, d, K)
    base = SM.silhouette_samples(x, y, return_parts=True)
    score, medoids = SM.silhouette_score(x, y), SM.cluster_medoids(x, y)
    assert SM._SIL_LAST["ranges"] == 1
    monkeypatch.setattr(SM, "_SIL_ROWS_PER_LAUNCH", 128)
    before = dict(SM._SIL_CALLS)
    assert same_parts(SM.silhouette_samples(x, y, return_parts=True), base)
    assert SM._SIL_LAST["ranges"] == -(-n // 128) and SM._SIL_CALLS["silhouette"] == before["silhouette"] + SM._SIL_LAST["ranges"]
    assert bits(SM.silhouette_score(x, y)) == bits(score) and same_parts(SM.cluster_medoids(x, y), medoids)


def test_noise_label_filters_the_rows_of_hdbscan():
    from scrubvae_amd.eval import HDBSCAN, cluster_medoids, cluster_silhouette, silhouette_samples, silhouette_score
    x, _ = SC.blobs(600, 8, 6, 608)
    labels = HDBSCAN(min_cluster_size=10).fit_predict(x)
    keep = np.flatnonzero(labels != -1)
    k = len(np.unique(labels[keep]))
    print(f"HDBSCAN on 600 x 8: {k} clusters, {600 - len(keep)} noise rows")
    assert 0 < len(keep) < 600 and k >= 2, "the input is meant to give clusters and noise"
    got = silhouette_samples(x, labels, noise_label=-1, return_parts=True)
    sub = silhouette_samples(x[keep], labels[keep], return_parts=True)
    noise = np.setdiff1d(np.arange(600), keep)
    for full, part in zip(got, sub):
        assert bits(full[keep]) == bits(part)
    assert np.isnan(got.s[noise]).all() and np.isnan(got.a[noise]).all() and np.isnan(got.b[noise]).all()
    assert (got.nearest[noise] == -1).all() and (got.nearest[keep] != -1).all()
    score = silhouette_score(x, labels, noise_label=-1)
    assert bits(score) == bits(silhouette_score(x[keep], labels[keep]))
    # any fp64 order of m terms is within (m - 1) 2^-53 sum |s| of the exact sum; numpy's mean and the device's are two of them
    assert abs(score - got.s[keep].mean()) <= 2 * (len(keep) + 4) * SC.EPS * np.abs(got.s[keep]).mean()
    ids, means, sizes = cluster_silhouette(x, labels, noise_label=-1)
    assert np.array_equal(ids, np.unique(labels[keep])) and sizes.sum() == len(keep) and sizes.dtype == np.int64
    for c, mean, size in zip(ids, means, sizes):
        rows = labels == c
        assert size == rows.sum() and abs(mean - got.s[rows].mean()) <= 2 * (size + 4) * SC.EPS * np.abs(got.s[rows]).mean()
    ids_m, med = cluster_medoids(x, labels, noise_label=-1)
    _, med_sub = cluster_medoids(x[keep], labels[keep])
    assert np.array_equal(ids_m, ids) and np.array_equal(med, keep[med_sub]) and np.array_equal(labels[med], ids)
    # without noise_label, -1 is one more cluster, as in sklearn
    plain = silhouette_samples(x, labels)
    assert np.isfinite(plain).all() and len(cluster_silhouette(x, labels)[0]) == k + 1


def test_all_rows_equal():
    from scrubvae_amd.eval import cluster_medoids, silhouette_samples, silhouette_score
    x = np.tile(np.array([[1.5, -2.0, 0.25]]), (70, 1))
    y = np.array([0] * 41 + [1] * 29)
    got = silhouette_samples(x, y, return_parts=True)
    assert (got.s == 0).all() and (got.a == 0).all() and (got.b == 0).all()
    score = silhouette_score(x, y)
    assert score == 0.0 and np.isfinite(score)
    assert np.array_equal(cluster_medoids(x, y)[1], [0, 41])  # every row ties: the lowest row of each cluster


def test_a_cluster_of_one_row():
    from scrubvae_amd.eval import cluster_medoids, cluster_silhouette, silhouette_samples
    x, y = SC.blobs(90, 3, 3, 5)
    y = y.copy()
    y[77] = 11
    got = silhouette_samples(x, y, return_parts=True)
    assert got.s[77] == 0.0 and got.a[77] == 0.0 and got.b[77] > 0 and got.nearest[77] != 11
    ids, med = cluster_medoids(x, y)
    assert med[list(ids).index(11)] == 77
    ids, means, sizes = cluster_silhouette(x, y)
    assert means[list(ids).index(11)] == 0.0 and sizes[list(ids).index(11)] == 1


def test_columns_past_n_contribute_nothing():
    from scrubvae_amd.eval import silhouette_samples
    x, y = SC.blobs(64, 3, 2, 9)
    a64 = silhouette_samples(x, y, return_parts=True).a
    x65 = np.vstack([x, np.full((1, 3), 1000.0)])
    y65 = np.append(y, 2)
    a65 = silhouette_samples(x65, y65, return_parts=True).a
    assert bits(a65[:64]) == bits(a64) and a65[64] == 0.0


def test_work_buffer_and_launch_counts(monkeypatch):
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import silhouette as SM
    lib = _lib.lib()
    x, y, p, _ = SC.case(700, 4, 300)
    k = len(p.uniq)
    before = dict(SM._SIL_CALLS)
    SM.silhouette_samples(x, y)
    assert SM._SIL_CALLS == {**before, "silhouette": before["silhouette"] + 1}   # one launch for both chunks of 256 clusters
    assert SM._SIL_LAST == {"work": lib.svae_silhouette_work(700, 700, k), "ranges": 1}
    SM.silhouette_score(x, y)
    SM.cluster_medoids(x, y)
    SM.cluster_silhouette(x, y)
    assert SM._SIL_CALLS == {"silhouette": before["silhouette"] + 4, "mean": before["mean"] + 1, "medoids": before["medoids"] + 1}
    monkeypatch.setattr(SM, "_SIL_ROWS_PER_LAUNCH", 256)
    before = dict(SM._SIL_CALLS)
    SM.silhouette_samples(x, y)
    assert SM._SIL_CALLS["silhouette"] == before["silhouette"] + 3              # rows 0..255, 256..511, 512..699
    assert SM._SIL_LAST == {"work": max(lib.svae_silhouette_work(256, 700, k), lib.svae_silhouette_work(188, 700, k)), "ranges": 3}
