"""neighbor_ranks / trustworthiness / continuity / embedding_quality (csrc/rank.hip) on the device against the numpy restatement
of tests/rank_checks.py.

Every kernel output is an integer, so the ranks and the curve sums are held to exact equality; the scores are the same closing
helpers on the same integers, so they are held to == as well, and test_rank_cpu.py pins those values to sklearn's.  The shapes
are the smallest that reach each path: two rows, partial row, column and feature tiles, several column chunks, rows not resident
in LDS, K at its maximum and at n - 1, thresholds spread over all the ranks, exact ties and duplicate rows."""
import functools

import numpy as np
import pytest
import torch

from tests import rank_checks as RC

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def check_ranks(x, idx, want=None):
    from scrubvae_amd.eval import neighbor_ranks
    got = neighbor_ranks(x, idx)
    want = RC.ranks(x, idx) if want is None else want
    assert got.dtype == np.int32 and got.shape == np.shape(idx)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    return got


@functools.lru_cache(maxsize=None)
def own_list(shape):
    """(x, restated kNN table) of a Gaussian case, computed once"""
    n, d, K = shape
    x = RC.rows(n, d)[0]
    idx = RC.knn(x, K)
    x.setflags(write=False)
    idx.setflags(write=False)
    return x, idx


def test_two_rows():
    x, idx = RC.two_rows()
    assert np.array_equal(check_ranks(x, idx), [[1], [1]])


@pytest.mark.parametrize("n,d,K", RC.ROWS)
def test_cross_ranks_equal_the_restatement(n, d, K):
    """the two tables that the scores are made of: the embedding's neighbours ranked in X, and X's ranked in the embedding"""
    w = RC.quality(n, d, K)
    check_ranks(w["X"], w["idx_y"], w["rank_t"])
    check_ranks(w["Y"], w["idx_x"], w["rank_c"])


@pytest.mark.parametrize("shape", [RC.WIDE, RC.FULL])
def test_own_list_at_the_largest_k(shape):
    n, d, K = shape
    x, idx = own_list(shape)
    got = check_ranks(x, idx, np.tile(np.arange(1, K + 1, dtype=np.int32), (n, 1)))
    # any other order of the same entries, and (K = n - 1) every other row in index order
    cols = np.random.default_rng(K).permutation(K)
    assert np.array_equal(check_ranks(x, idx[:, cols]), got[:, cols])
    if K == n - 1:
        every = np.stack([np.delete(np.arange(n), i) for i in range(n)])
        assert np.array_equal(np.sort(check_ranks(x, every), axis=1), got)


def test_random_columns_spread_over_all_ranks():
    n, d, K = RC.ROWS[1]
    x = RC.rows(n, d)[0]
    idx = RC.random_idx(n, K, seed=5)
    got = check_ranks(x, idx)
    assert got.min() == 1 and got.max() == n - 1 and (np.diff(np.sort(got, axis=1), axis=1) > 0).all()


@pytest.mark.parametrize("n", [130, 1037])
def test_embedded_side_alone(n):
    """d = 2"""
    y = RC.rows(n, 5)[1]
    check_ranks(y, RC.random_idx(n, 9, seed=n))


def test_ties_and_duplicates():
    g = RC.grid_rows()
    n = len(g)
    own = RC.knn(g, RC.GRID_K)
    check_ranks(g, own, np.tile(np.arange(1, RC.GRID_K + 1, dtype=np.int32), (n, 1)))
    check_ranks(g, RC.random_idx(n, RC.GRID_K, seed=1))


@pytest.mark.parametrize("n,d,K", RC.ROWS)
def test_ranks_of_kneighbors_are_one_to_k(n, d, K):
    from scrubvae_amd.eval import kneighbors, neighbor_ranks
    x = RC.rows(n, d)[0]
    idx = kneighbors(x, K, return_distance=False)
    assert np.array_equal(neighbor_ranks(x, idx), np.tile(np.arange(1, K + 1), (n, 1)))


def test_column_order_runs_and_inputs():
    from scrubvae_amd.eval import neighbor_ranks
    n, d, K = RC.ROWS[2]
    w = RC.quality(n, d, K)
    x, idx = w["X"], w["idx_y"]
    got = check_ranks(x, idx, w["rank_t"])
    cols = np.random.default_rng(3).permutation(K)
    assert np.array_equal(neighbor_ranks(x, idx[:, cols]), got[:, cols])        # a permutation of the columns and nothing else
    assert bits(neighbor_ranks(x, idx)) == bits(got)                            # two runs
    xd, idd = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(idx.copy()).cuda()
    for a, b in ((xd, idd), (xd, idx.astype(np.int32)), (x, idd)):              # device tensors and other integer dtypes
        assert np.array_equal(neighbor_ranks(a, b), got)
    x32 = x.astype(np.float32)                                                  # fp32 rows are converted, not rejected
    want32 = RC.ranks(x32, idx)
    for a in (x32, torch.from_numpy(x32).cuda(), x32.astype(np.float64)):
        assert np.array_equal(neighbor_ranks(a, idx), want32)


@pytest.mark.parametrize("n,d,K", RC.ROWS[1:])
def test_curve_sums(n, d, K):
    from scrubvae_amd.eval import embed_quality as EQ
    w = RC.quality(n, d, K)
    for rank, pen, hit, rows in ((w["rank_t"], w["pen_t"], w["hit"], w["rows_t"]), (w["rank_c"], w["pen_c"], w["hit"], w["rows_c"])):
        table = torch.from_numpy(rank.copy()).cuda()
        got = EQ._curves_device(table)
        assert got[0].dtype == got[1].dtype == np.int64 and got[2] is None
        assert np.array_equal(got[0], pen) and np.array_equal(got[1], hit)
        for at in (1, 5, K):
            p, h, r = EQ._curves_device(table, at)
            assert np.array_equal(p, pen) and np.array_equal(h, hit) and r.dtype == np.int64 and np.array_equal(r, rows[at - 1])


@pytest.mark.parametrize("n,d,K", RC.ROWS[1:])
def test_scores_equal_the_restatement(n, d, K):
    from scrubvae_amd.eval import EmbeddingQuality, continuity, embedding_quality, trustworthiness
    w = RC.quality(n, d, K)
    X, Y = w["X"], w["Y"]
    for k in (1, 5, K):
        t, c = trustworthiness(X, Y, n_neighbors=k), continuity(X, Y, n_neighbors=k)
        assert isinstance(t, float) and isinstance(c, float) and t == w["T"][k - 1] and c == w["C"][k - 1]
    assert trustworthiness(X, Y) == w["T"][4] and continuity(torch.from_numpy(X.copy()).cuda(), Y) == w["C"][4]
    q = embedding_quality(X, Y, max_neighbors=K, rows_at=5)
    assert isinstance(q, EmbeddingQuality) and q.n == n and np.array_equal(q.k, np.arange(1, K + 1)) and q.rows_at == 5
    assert RC.same(q.trustworthiness, w["T"]) and RC.same(q.continuity, w["C"]) and RC.same(q.q_nx, w["q"]) and RC.same(q.r_nx, w["r"])
    assert q.auc_r_nx == w["auc"] and np.array_equal(q.hits, w["hit"])
    assert np.array_equal(q.penalty["trustworthiness"], w["pen_t"]) and np.array_equal(q.penalty["continuity"], w["pen_c"])
    assert np.array_equal(q.intrusion_rows, w["rows_t"][4]) and np.array_equal(q.extrusion_rows, w["rows_c"][4])
    plain = embedding_quality(torch.from_numpy(X.copy()).cuda().float(), torch.from_numpy(Y.copy()).cuda().float(), max_neighbors=3)
    assert plain.intrusion_rows is None and plain.extrusion_rows is None and len(plain.k) == 3


def test_identical_and_small():
    from scrubvae_amd.eval import embedding_quality
    X = RC.rows(130, 5)[0]
    q = embedding_quality(X, X.copy(), max_neighbors=20, rows_at=20)
    assert (q.trustworthiness == 1.0).all() and (q.continuity == 1.0).all() and (q.q_nx == 1.0).all() and q.auc_r_nx == 1.0
    assert (q.intrusion_rows == 0).all() and (q.extrusion_rows == 0).all()
    # K = n - 1: T and C are NaN from n / 2 on, R_NX at n - 1, Q_NX ends at 1
    X, Y = RC.rows(8, 3)
    from scrubvae_amd.eval import embed_quality as EQ
    w = RC.quality_of(X, Y, 7, EQ)
    q = embedding_quality(X, Y, max_neighbors=7)
    assert RC.same(q.trustworthiness, w["T"]) and RC.same(q.continuity, w["C"]) and RC.same(q.r_nx, w["r"]) and q.auc_r_nx == w["auc"]
    assert np.isnan(q.trustworthiness[3:]).all() and np.isnan(q.r_nx[6]) and q.q_nx[6] == 1.0


def test_column_chunks():
    from scrubvae_amd import _lib
    work = _lib.lib().svae_rank_work
    assert [(work(n, k) - n * k * 16) // (n * k * 4) for n, k in ((30, 29), (301, 12), (1037, 30))] == [1, 5, 6]
    from scrubvae_amd.eval import embed_quality as EQ
    x, idx = RC.two_rows()
    EQ.neighbor_ranks(x, idx)
    assert EQ._RANK_LAST == dict(work=2 * 20, chunks=1)


def test_bad_entries_read_nothing_out_of_bounds():
    """the C ABI trusts idx, but an entry out of range or equal to its row is skipped: it gets rank n, the others their own"""
    from scrubvae_amd import _lib, ops
    n, d, K = RC.ROWS[0]
    w = RC.quality(n, d, K)
    x, idx = w["X"], w["idx_y"].astype(np.int32)
    bad = idx.copy()
    bad[3, 2], bad[64, 0], bad[129, 19], bad[7, 7] = n, -1, 2 ** 31 - 1, 7
    lib = _lib.lib()
    Z, T = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(bad).cuda()
    work = torch.empty((lib.svae_rank_work(n, K) + 7) // 8, dtype=torch.int64, device="cuda")
    rank = torch.full((n, K), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.svae_knn_ranks(Z.data_ptr(), d, d, n, T.data_ptr(), K, work.data_ptr(), rank.data_ptr(), ops._stream()), "knn_ranks")
    got = rank.cpu().numpy()
    changed = bad != idx
    assert changed.sum() == 4 and (got[changed] == n).all() and np.array_equal(got[~changed], w["rank_t"][~changed])


def test_argument_errors_launch_nothing():
    from scrubvae_amd import _lib, ops
    lib, st, E = _lib.lib(), ops._stream(), _lib.ERR_ARG
    n, d, K = 40, 3, 3
    Z = torch.zeros(n, d, dtype=torch.float64, device="cuda")
    T = torch.ones(n, K, dtype=torch.int32, device="cuda")
    work = torch.zeros((lib.svae_rank_work(n, K) + 7) // 8, dtype=torch.int64, device="cuda")
    rank = torch.full((n, K), -1, dtype=torch.int32, device="cuda")
    sums = torch.full((2, K), -1, dtype=torch.int64, device="cuda")

    def ranks(k=K, n=n, w=work, idx=T):
        return lib.svae_knn_ranks(Z.data_ptr(), d, d, n, ops._p(idx), k, ops._p(w), rank.data_ptr(), st)

    for bad, text in ((dict(k=0), "neighbour count"), (dict(k=91), "neighbour count"), (dict(k=3, n=3), "neighbour count"),
                      (dict(w=None), "null"), (dict(idx=None), "null")):
        assert ranks(**bad) == E and text in _lib.last_error(), (bad, _lib.last_error())
    assert lib.svae_rank_curves(rank.data_ptr(), n, K, 4, sums[0].data_ptr(), sums[1].data_ptr(), None, st) == E
    assert lib.svae_rank_curves(rank.data_ptr(), n, K, 2, sums[0].data_ptr(), sums[1].data_ptr(), None, st) == E
    torch.cuda.synchronize()
    assert (rank == -1).all() and (work == 0).all() and (sums == -1).all()     # nothing was launched
