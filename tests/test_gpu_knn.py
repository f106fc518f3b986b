"""kneighbors / kneighbors_graph / knn_label_purity / knn_class_rand_cv / knn_reg_rand_cv (csrc/knn.hip) on the device against the
numpy restatement of tests/knn_checks.py.

The key (s, j) is strict, so the result is unique: idx is held to exact equality and dist to equal bytes, with no tolerance
anywhere.  The sizes are the smallest that reach each path of the kernel: partial row and column tiles, a partial feature chunk,
rows not resident in LDS, several column tiles per block with cuts of the candidate buffers between them, exactly full tiles and
one row past them, k = n - 1, k = 1 at n = 2, the largest k, one and several column chunks per row tile."""
import numpy as np
import pytest
import torch

from tests import knn_checks as KC
from tests import silhouette_checks as SC

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def check(x, k, want=None, group=None):
    from scrubvae_amd.eval import kneighbors
    dist, idx = kneighbors(x, k, group=group)
    w_dist, w_idx = KC.neighbors(x, k, group) if want is None else want
    assert dist.dtype == np.float64 and idx.dtype == np.int64 and dist.shape == idx.shape == (len(x), k)
    assert np.array_equal(idx, w_idx), int(np.argmax((idx != w_idx).any(1)))
    assert bits(dist) == bits(w_dist)
    return dist, idx


@pytest.mark.parametrize("n,d,k", KC.SIZES)
def test_equal_to_the_restatement(n, d, k):
    x, _, dist, idx = KC.case(n, d, k)
    check(x, k, (dist, idx))


@pytest.mark.parametrize("n", [64, 65, 128, 129])
def test_full_tiles_and_one_row_past_them(n):
    x, _ = SC.blobs(n, 4, 3, seed=n)
    check(x, 3)


def test_two_rows():
    dist, idx = check(np.array([[0.0, 0.0], [3.0, 4.0]]), 1)
    assert np.array_equal(idx, [[1], [0]]) and np.array_equal(dist, [[5.0], [5.0]])


def test_the_largest_k():
    from scrubvae_amd.eval import neighbors as NB
    k = NB.KNN_MAX_K
    x, _ = SC.blobs(3 * k + 17, 5, 4, seed=k)
    check(x, k)
    with pytest.raises(ValueError):
        NB.kneighbors(x, k + 1)


def test_one_and_several_column_chunks():
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import neighbors as NB
    seen = set()
    for n, d, k in [(60, 3, 4), (301, 3, 5), (1037, 1, 10)]:
        x, _ = SC.blobs(n, d, 4, seed=n)
        check(x, k, KC.case(n, d, k)[2:] if (n, d, k) in KC.SIZES else None)
        assert NB._KNN_LAST["work"] == _lib.lib().svae_knn_work(n, k)
        seen.add(NB._KNN_LAST["chunks"])
    assert seen == {1, 5, 6}


@pytest.mark.parametrize("k", [6, 90])
def test_one_chunk_of_many_tiles_against_the_core_distances(k):
    """513 row tiles: every block walks all 513 column tiles and cuts its buffers on the way (at k = 90 after every tile that
    added a candidate), nothing is merged.  The restatement's n^2 matrix is out of reach at this size: the k-th distance is held to
    svae_hdb_core(k + 1), and the lists to their own distances, to the key order and to k different rows other than the row."""
    from scrubvae_amd.eval import neighbors as NB
    assert k <= NB.KNN_MAX_K
    n, d = 64 * 512 + 7, 2
    x, _ = SC.blobs(n, d, 4, seed=n)
    dist, idx = NB.kneighbors(x, k)
    assert NB._KNN_LAST["chunks"] == 1
    assert bits(dist[:, k - 1]) == bits(core_distances(x, k + 1))
    again = np.zeros((n, k))
    for j in range(d):
        e = x[:, j, None] - x[idx, j]
        again = again + e * e
    assert bits(np.sqrt(again)) == bits(dist)
    step = np.diff(again, axis=1)
    assert (step >= 0).all() and (np.diff(idx, axis=1)[step == 0] > 0).all()
    assert not (idx == np.arange(n)[:, None]).any() and (np.diff(np.sort(idx, axis=1), axis=1) > 0).all()


def test_ties_and_duplicates():
    x = KC.grid_rows()
    dist, idx = check(x, 6)
    assert (dist[:, 0] == 0).all() and not (idx == np.arange(300)[:, None]).any()
    same = np.diff(dist, axis=1) == 0
    assert same.any() and (np.diff(idx, axis=1)[same] > 0).all()
    check(x, 90)


def core_distances(x, k):
    """svae_hdb_core: the k-th smallest distance of every row, itself included, by radix select"""
    from scrubvae_amd import _lib, ops
    n, d = x.shape
    Z = torch.from_numpy(np.array(x, dtype=np.float64)).cuda()   # a copy: the cached cases are read-only
    core = torch.empty(n, dtype=torch.float64, device=Z.device)
    _lib.check(_lib.lib().svae_hdb_core(Z.data_ptr(), d, d, n, k, core.data_ptr(), ops._stream()), "hdb_core")
    return core.cpu().numpy()


@pytest.mark.parametrize("n,d,k", [(301, 3, 5), (131, 128, 7)])
def test_kth_distance_equals_the_core_distance(n, d, k):
    from scrubvae_amd.eval import kneighbors
    x = KC.case(n, d, k)[0]
    dist, _ = kneighbors(x, k)
    assert bits(dist[:, k - 1]) == bits(core_distances(x, k + 1))


def test_groups_and_the_probes():
    import scrubvae_amd.eval as E
    from scrubvae_amd.eval import metrics as M
    from scrubvae_amd.eval import neighbors as NB
    n, d, k, folds = KC.CV
    x, cls, y, fold, idx = KC.cv_case()
    want = KC.neighbors(x, k, fold)
    assert np.array_equal(want[1], idx)
    check(x, k, want, group=fold)
    check(x, k, want, group=torch.from_numpy(fold * 10 - 3).cuda())      # any integers, anywhere
    names = np.array([5, -2, 40, 7])[cls]
    before = NB._KNN_CALLS["knn"]
    got = M._knn_class(x, names, 1, folds, k, want_rows=True)
    assert NB._KNN_CALLS["knn"] == before + 1                        # one search for all folds
    pred, _ = KC.class_pred(idx, np.unique(names, return_inverse=True)[1])
    assert np.array_equal(got["pred"], np.unique(names)[pred]) and np.array_equal(got["fold"], fold)
    want_acc = KC.per_fold(fold, lambda te: float((np.unique(names)[pred][te] == names[te]).sum()) / float(te.sum()))
    assert got["acc"] == want_acc and E.knn_class_rand_cv(x, names, window=1, folds=folds, n_neighbors=k) == want_acc
    before = NB._KNN_CALLS["knn"]
    got = M._knn_reg(torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()), 1, folds, k, want_rows=True)
    assert NB._KNN_CALLS["knn"] == before + 1
    reg = KC.reg_pred(idx, y)
    assert bits(got["pred"]) == bits(reg)
    r2 = E.knn_reg_rand_cv(x, y, window=1, folds=folds, n_neighbors=k)
    assert r2 == got["r2"] and len(r2) == folds
    for f in range(folds):
        te = fold == f
        assert abs(r2[f] - KC.r2(y[te], reg[te])) <= KC.r2_gate(y[te], reg[te])
    # one target as a vector, and the downsample: rows 0, 3, 6, ... of a longer recording
    long_x, long_y = np.repeat(x, 3, axis=0), np.repeat(y[:, 0], 3)
    assert E.knn_reg_rand_cv(long_x, long_y, window=3, folds=folds, n_neighbors=k) == \
        E.knn_reg_rand_cv(x, y[:, :1], window=1, folds=folds, n_neighbors=k)
    share, mean = E.knn_label_purity(x, names, k)
    w_share, w_mean = KC.purity(KC.neighbors(x, k)[1], names)
    assert bits(share) == bits(w_share) and mean == w_mean and isinstance(mean, float)


def test_graph():
    pytest.importorskip("scipy.sparse")
    from scrubvae_amd.eval import kneighbors_graph
    x, _, dist, idx = KC.case(301, 3, 5)
    for mode, data in (("connectivity", np.ones(301 * 5)), ("distance", dist.reshape(-1))):
        g = kneighbors_graph(x, 5, mode=mode)
        assert g.shape == (301, 301) and np.array_equal(g.indices, idx.reshape(-1)) and bits(g.data) == bits(data)
        assert np.array_equal(g.indptr, np.arange(0, 301 * 5 + 1, 5))


def test_two_calls_give_the_same_bits():
    from scrubvae_amd.eval import kneighbors
    for size in [(301, 3, 5), (600, 8, 64)]:
        x = KC.case(*size)[0]
        a, b = kneighbors(x, size[2]), kneighbors(x, size[2])
        assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1])
        assert np.array_equal(kneighbors(x, size[2], return_distance=False), a[1])


def test_permuted_rows_give_the_permuted_result():
    from scrubvae_amd.eval import kneighbors
    x, _, dist, idx = KC.case(301, 3, 5)      # tie-free (test_knn_cpu.py): the neighbour sets do not depend on the row order
    perm = np.random.default_rng(1).permutation(301)
    inv = np.argsort(perm)
    p_dist, p_idx = kneighbors(x[perm], 5)    # row a of the permuted input is row perm[a]
    assert bits(p_dist) == bits(dist[perm]) and np.array_equal(p_idx, inv[idx[perm]])


def test_input_kinds_give_the_same_bits():
    from scrubvae_amd.eval import kneighbors
    x, _, dist, idx = KC.case(130, 37, 16)    # float32-representable values
    wide = np.zeros((130, 74))
    wide[:, ::2] = x
    xt = torch.from_numpy(x.copy())
    for z in (x.astype(np.float32), xt.cuda(), torch.from_numpy(wide).cuda()[:, ::2], wide[:, ::2], xt, xt.cuda().to(torch.float32)):
        got = kneighbors(z, 16)
        assert bits(got[0]) == bits(dist) and np.array_equal(got[1], idx)
