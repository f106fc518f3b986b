"""The k-nearest-neighbour search without a GPU: the restatement of tests/knn_checks.py pinned bit for bit to sklearn's KD-tree on
tie-free inputs, the kNN probes' votes and means pinned to sklearn's estimators fold by fold, R^2 to r2_score within the derived
gate, the host glue of the graph, argument errors raised before any device work, and the C-ABI exports."""
import numpy as np
import pytest
import torch

from tests import knn_checks as KC
from tests import silhouette_checks as SC


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("n,d,k", KC.SIZES)
def test_restatement_equals_sklearn_kd_tree_bit_for_bit(n, d, k):
    nb = pytest.importorskip("sklearn.neighbors")
    x, _, dist, idx = KC.case(n, d, k)
    assert KC.ties(x, k) == (0, 0), "the input is meant to have no ties among the first k + 1 keys of any row"
    sk_dist, sk_idx = nb.NearestNeighbors(n_neighbors=k, algorithm="kd_tree").fit(x).kneighbors()
    assert dist.dtype == sk_dist.dtype == np.float64 and dist.shape == sk_dist.shape == (n, k)
    assert np.array_equal(idx, sk_idx)
    assert bits(dist) == bits(sk_dist)
    assert (np.diff(dist, axis=1) > 0).all() and not (idx == np.arange(n)[:, None]).any()


def test_grid_rows_are_the_case_described():
    x = KC.grid_rows()
    dist, idx = KC.neighbors(x, 6)
    tie_s, _ = KC.ties(x, 6)
    assert len(np.unique(x, axis=0)) == 25 and tie_s == 300
    assert (dist[:, 0] == 0).all() and not (idx == np.arange(300)[:, None]).any()   # a duplicate at 0, never the row itself
    same = np.diff(dist, axis=1) == 0
    assert same.any() and (np.diff(idx, axis=1)[same] > 0).all()                    # ties in index order


def sklearn_folds(make, x, target, fold):
    out = np.empty((len(x),) + target.shape[1:], dtype=target.dtype)
    for f in range(int(fold.max()) + 1):
        te = fold == f
        out[te] = make().fit(x[~te], target[~te]).predict(x[te])
    return out


def test_cv_probes_equal_sklearn_fold_by_fold():
    nb = pytest.importorskip("sklearn.neighbors")
    sm = pytest.importorskip("sklearn.metrics")
    n, d, k, folds = KC.CV
    x, cls, y, fold, idx = KC.cv_case()
    assert KC.ties(x, k, fold) == (0, 0)
    assert (fold[idx] != fold[:, None]).all()
    pred, _ = KC.class_pred(idx, cls)
    sk_pred = sklearn_folds(lambda: nb.KNeighborsClassifier(n_neighbors=k, algorithm="kd_tree"), x, cls, fold)
    assert np.array_equal(pred, sk_pred)
    reg = KC.reg_pred(idx, y)
    sk_reg = sklearn_folds(lambda: nb.KNeighborsRegressor(n_neighbors=k, algorithm="kd_tree"), x, y, fold)
    err = np.abs(reg - sk_reg).max()
    print(f"kNN regression n={n} k={k}: largest |restated - sklearn| prediction {err:.3e}, gate {k * 2.0 ** -53 * np.abs(y).max():.3e}")
    assert err <= k * 2.0 ** -53 * np.abs(y).max()
    for f in range(folds):
        te = fold == f
        got, want, gate = KC.r2(y[te], reg[te]), sm.r2_score(y[te], reg[te]), KC.r2_gate(y[te], reg[te])
        print(f"  fold {f}: R^2 {got:.6f}, |restated - r2_score| {abs(got - want):.3e}, gate {gate:.3e}")
        assert abs(got - want) <= gate


def test_a_tied_vote_goes_to_the_lowest_class():
    nb = pytest.importorskip("sklearn.neighbors")
    from scrubvae_amd.eval.metrics import kfold_assign
    g = np.random.default_rng(4)
    x = g.normal(size=(40, 2)).astype(np.float32).astype(np.float64)
    cls = g.integers(0, 2, 40)
    fold = kfold_assign(40, 4)
    assert KC.ties(x, 4, fold) == (0, 0)
    _, idx = KC.neighbors(x, 4, fold)
    pred, votes = KC.class_pred(idx, cls)
    tied = votes[:, 0] == votes[:, 1]
    assert tied.sum() >= 3 and (pred[tied] == 0).all()
    assert np.array_equal(pred, sklearn_folds(lambda: nb.KNeighborsClassifier(n_neighbors=4, algorithm="kd_tree"), x, cls, fold))


def test_metrics_r2_is_r2_score():
    sm = pytest.importorskip("sklearn.metrics")
    from scrubvae_amd.eval.metrics import _knn_r2
    _, _, y, fold, idx = KC.cv_case()
    reg = KC.reg_pred(idx, y)
    te = fold == 0
    assert abs(_knn_r2(y[te], reg[te]) - sm.r2_score(y[te], reg[te])) <= KC.r2_gate(y[te], reg[te])
    const = np.stack([np.full(9, 2.5), np.arange(9.0)], 1)      # a constant target: sklearn's force_finite
    for p in (const.copy(), const + 1.0):
        assert _knn_r2(const, p) == sm.r2_score(const, p)


@pytest.mark.parametrize("mode", ["connectivity", "distance"])
def test_graph_glue_equals_sklearn(mode):
    nb = pytest.importorskip("sklearn.neighbors")
    pytest.importorskip("scipy.sparse")
    from scrubvae_amd.eval.neighbors import _graph
    x, _, dist, idx = KC.case(301, 3, 5)
    got = _graph(dist, idx, 301, mode)
    want = nb.kneighbors_graph(nb.NearestNeighbors(n_neighbors=5, algorithm="kd_tree").fit(x), 5, mode=mode, include_self=False)
    assert got.shape == want.shape == (301, 301) and got.format == "csr" and got.dtype == np.float64
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices) and bits(got.data) == bits(want.data)


XS, YS = SC.blobs(12, 2, 3, 0)
BAD = np.arange(24).reshape(12, 2) == 5


@pytest.mark.parametrize("z,k,kwargs", [
    (XS, 0, {}),
    (XS, -1, {}),
    (XS, 12, {}),                                             # k > n - 1
    (XS, 3.0, {}),
    (XS, True, {}),
    (XS[0], 1, {}),                                           # 1-D
    (XS[None], 1, {}),                                        # 3-D
    (XS[:1], 1, {}),                                          # one row
    (np.zeros((12, 0)), 1, {}),                               # no feature
    (np.where(BAD, np.nan, XS), 3, {}),
    (np.where(BAD, np.inf, XS), 3, {}),
    (torch.from_numpy(np.where(BAD, np.nan, XS)), 3, {}),
    (XS, 3, dict(group=np.zeros(11, dtype=np.int64))),        # group of the wrong length
    (XS, 3, dict(group=np.zeros(12))),                        # group not integers
    (XS, 3, dict(group=np.array([0] * 10 + [1, 2]))),         # the rows of group 0 keep 2 candidates
    (XS, 1, dict(group=np.zeros(12, dtype=np.int64))),        # one group: no candidate at all
])
def test_argument_errors_before_device_work(z, k, kwargs):
    """this machine has no device: a ValueError, not the "no device is available" RuntimeError, shows the order"""
    import scrubvae_amd.eval as E
    with pytest.raises(ValueError):
        E.kneighbors(z, k, **kwargs)
    if not kwargs:
        with pytest.raises(ValueError):
            E.kneighbors_graph(z, k)
        with pytest.raises(ValueError):
            E.knn_label_purity(z, YS, k)


def test_more_argument_errors_before_device_work():
    import scrubvae_amd.eval as E
    from scrubvae_amd.eval import neighbors as NB
    big = np.zeros((NB.KNN_MAX_K + 5, 1))
    with pytest.raises(ValueError, match=str(NB.KNN_MAX_K)):
        E.kneighbors(big, NB.KNN_MAX_K + 1)
    with pytest.raises(ValueError):
        E.kneighbors_graph(XS, 3, mode="weights")
    for labels in (YS[:-1], YS.astype(np.float64), YS[:, None]):
        with pytest.raises(ValueError):
            E.knn_label_purity(XS, labels, 3)
    x, cls, y, _, _ = KC.cv_case()
    for fn, target in ((E.knn_class_rand_cv, cls), (E.knn_reg_rand_cv, y)):
        with pytest.raises(ValueError):
            fn(x, target, window=1, folds=5, n_neighbors=0)
        with pytest.raises(ValueError):
            fn(x, target, window=1, folds=5, n_neighbors=NB.KNN_MAX_K + 1)
        with pytest.raises(ValueError):
            fn(x[:12], target[:12], window=1, folds=2, n_neighbors=7)   # 6 training rows per fold
        with pytest.raises(ValueError):
            fn(x, target[:-1], window=1, folds=5, n_neighbors=3)
        with pytest.raises(ValueError):
            fn(np.where(np.arange(203)[:, None] == 9, np.nan, x), target, window=1, folds=5, n_neighbors=3)


def test_check_maps_rows_and_groups():
    from scrubvae_amd.eval import neighbors as NB
    x, y = SC.blobs(50, 3, 4, 3)
    names = np.array([-1, 7, 10 ** 9, 3])[y]
    rows, k, grp = NB._knn_check(x.astype(np.float32), np.int64(4), torch.from_numpy(names))
    assert rows.dtype == np.float64 and np.array_equal(rows, x) and k == 4 and isinstance(k, int)
    assert grp.dtype == np.int32 and np.array_equal(np.unique(names)[grp], names)
    rows, k, grp = NB._knn_check(torch.from_numpy(x)[:, ::2], 49)
    assert grp is None and rows.dtype == torch.float64 and np.array_equal(rows.numpy(), x[:, ::2])


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import neighbors as NB
    lib = _lib.lib()
    work = lib.svae_knn_work
    kmax = _lib.KNN_MAX_K
    assert kmax >= 64
    assert work(1, 1) == 0 and work(0, 1) == 0 and work(-5, 1) == 0   # n < 2
    assert work(10, 0) == 0 and work(10, -1) == 0                     # k < 1
    assert work(10, 10) == 0                                          # k > n - 1
    assert work(1000, kmax + 1) == 0
    # column chunks x rows padded to 64 x k x (a uint64 key and an int32 index)
    assert work(2, 1) == 1 * 64 * 1 * 12
    assert work(301, 5) == 5 * 320 * 5 * 12                           # 5 column tiles, one chunk each
    assert work(1037, 10) == 6 * 1088 * 10 * 12                       # 17 column tiles, at most 8 chunks: 6 of 3 tiles
    assert work(1000, kmax) > 0
    assert work(40000, 15) == 1 * 40000 * 15 * 12                     # 625 row tiles: one chunk
    assert work(2 ** 31 - 1, 3) == 1 * 2 ** 31 * 3 * 12
    # the argument errors of svae_knn come before any device work (the pointers are never read): above the cap, k > n - 1, d < 1
    fake = 4096
    for n, d, k in ((1000, 4, kmax + 1), (10, 4, 10), (10, 0, 3), (1, 4, 1)):
        assert lib.svae_knn(fake, max(d, 1), d, n, k, None, fake, fake, fake, None) == _lib.ERR_ARG
    assert lib.svae_knn(fake, 4, 4, 10, 3, None, None, fake, fake, None) == _lib.ERR_ARG
    assert "null" in _lib.last_error()
    import scrubvae_amd.eval as E
    for name in ("kneighbors", "kneighbors_graph", "knn_label_purity", "knn_class_rand_cv", "knn_reg_rand_cv"):
        assert callable(getattr(E, name))
    assert NB._KNN_CALLS.keys() >= {"knn"} and NB._KNN_LAST.keys() >= {"work", "chunks"}


SPLIT_N = (2, 63, 64, 65, 301, 1037, 4096, 4097, 32775, 40000, 100000, 2 ** 31 - 1)


def _ceil(a, b):
    return -(-a // b)


def _split(units, row_blocks, cap, blocks=512):
    """the rule that splits inner units over a grid dimension, restated: (units per part, parts that are not empty)"""
    want = min(units, cap, _ceil(blocks, row_blocks))
    per = _ceil(units, want)
    return per, _ceil(units, per)


def test_split_rule_gives_the_parents_work_sizes():
    """every *_work size is a function of the one split rule (csrc/svae_internal.h chunk_split); the sizes asserted here are those
    of the library before the rule was written once, which passes this test unchanged"""
    from scrubvae_amd import _lib
    lib = _lib.lib()
    checked = 0
    # the walks over 64 x 64 tiles: at most 8 column chunks; lists of k (uint64, int32) per chunk and padded row
    for name, kmax in (("svae_knn_work", _lib.KNN_MAX_K), ("svae_mi_work", _lib.MI_MAX_K), ("svae_rank_work", _lib.KNN_MAX_K)):
        for n in SPLIT_N:
            for k in (1, kmax):
                nt = _ceil(n, 64)
                gy = _split(nt, nt, 8)[1]
                size = n * k * 16 + gy * n * k * 4 if name == "svae_rank_work" else gy * nt * 64 * k * 12
                assert getattr(lib, name)(n, k) == (size if k <= n - 1 else 0), (name, n, k)
                checked += 1
    for m in SPLIT_N:
        for n in SPLIT_N:
            for k in (1, _lib.KNN_MAX_K):
                rt = _ceil(m, 64)
                gy = _split(_ceil(n, 64), rt, 8)[1]
                assert lib.svae_knn_cross_work(m, n, k) == (gy * rt * 64 * k * 12 if k <= n else 0), (m, n, k)
                checked += 1
    # silhouette: rows x n pairs, 16, 64 or 256 cluster columns per block in grid z; n < 2^26
    for n in SPLIT_N:
        for rows in SPLIT_N:
            for K in (2, _lib.SIL_MAX_CLUSTERS):
                nc = 16 if K <= 16 else 64 if K <= 64 else 256
                gx, gz = _ceil(rows, 64), _ceil(K, nc)
                gy = _split(_ceil(n, 64), gx * gz, 8)[1]
                ok = 3 <= n < 2 ** 26 and rows <= n
                assert lib.svae_silhouette_work(rows, n, K) == (gy * gx * 64 * gz * nc if ok else 0), (rows, n, K)
                checked += 1
    # t-SNE repulsion: 256 rows per block, column tiles of 64, at most 8 chunks or the caller's count; n <= 2^26
    for n in SPLIT_N:
        for chunks in (0, 1, 3, 8):
            gx, nt = _ceil(n, 256), _ceil(n, 64)
            gy = _split(nt, gx, 8)[1] if chunks == 0 else _split(nt, 1, chunks, blocks=2 ** 40)[1]
            assert lib.svae_tsne_repulsion_work(n, chunks) == (gy * 3 * gx * 256 if n <= 2 ** 26 else 0), (n, chunks)
            checked += 1
            for m in SPLIT_N:   # the cross form splits from n alone: the most chunks there are unless the caller names a count
                gyc = _split(nt, 1, chunks or 8, blocks=2 ** 40)[1]
                ok = m <= 2 ** 26 and n <= 2 ** 26
                assert lib.svae_tsne_cross_repulsion_work(m, n, chunks) == (gyc * 3 * _ceil(m, 256) * 256 if ok else 0), (m, n, chunks)
                checked += 1
    # density: tiles of 128 x 128 cells, the points in chunks of 32 over at most 128 slices; n <= 2^30
    for n in SPLIT_N + (1,):
        for gx in (2, _lib.DENSITY_MAX_GRID):
            for gy in (2, _lib.DENSITY_MAX_GRID):
                slices = _split(_ceil(n, 32), _ceil(gx, 128) * _ceil(gy, 128), 128)[1]
                assert lib.svae_density_work(n, gx, gy) == ((slices * gy * gx + 2 * n) * 8 if n <= 2 ** 30 else 0), (n, gx, gy)
                checked += 1
    assert checked == 3 * 24 + 288 + 288 + 48 * 13 + 13 * 4
    # the rule itself, where a slip would show: the cap, the grid bound and the empty last part
    assert _split(17, 17, 8) == (3, 6) and _split(5, 5, 8) == (1, 5) and _split(625, 625, 8) == (625, 1)
    assert _split(65, 65, 8) == (9, 8) and _split(9, 1, 8) == (2, 5)
