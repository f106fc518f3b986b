"""Neighbour ranks and the embedding scores without a GPU: the restatement of tests/rank_checks.py pinned to
sklearn.manifold.trustworthiness with exact equality, the hand-checkable outcomes that test_gpu_rank.py repeats on the device,
argument errors before any device work and the C-ABI exports."""
import os

import numpy as np
import pytest
import torch

from tests import rank_checks as RC


@pytest.mark.parametrize("n,d,K", RC.ROWS)
def test_restatement_is_sklearn(n, d, K):
    """equal, not close: the penalty is an exact integer and the closing expression is sklearn's own"""
    manifold = pytest.importorskip("sklearn.manifold")
    w = RC.quality(n, d, K)
    X, Y = w["X"], w["Y"]
    # the precondition under which sklearn's dot-product distances and the contract's difference-form distances sort alike
    gap = min(RC.gaps(X), RC.gaps(Y))
    print(f"n={n} d={d}: smallest relative gap between consecutive sorted distances of a row {gap:.2e}")
    assert gap > 1e-12
    for k in (1, 5, K):
        t, c = manifold.trustworthiness(X, Y, n_neighbors=k), manifold.trustworthiness(Y, X, n_neighbors=k)
        print(f"n={n} k={k}: T restated {w['T'][k - 1]!r} sklearn {t!r}; C restated {w['C'][k - 1]!r} sklearn {c!r}")
        assert w["T"][k - 1] == t and w["C"][k - 1] == c


@pytest.mark.parametrize("n,d,K", RC.ROWS)
def test_ranks_of_the_own_list_are_one_to_k(n, d, K):
    w = RC.quality(n, d, K)
    for x, idx in ((w["X"], w["idx_x"]), (w["Y"], w["idx_y"])):
        assert np.array_equal(RC.ranks(x, idx), np.tile(np.arange(1, K + 1, dtype=np.int32), (n, 1)))
    # distinct within a row, between 1 and n - 1, whatever the table
    r = RC.ranks(w["X"], RC.random_idx(n, K, seed=n))
    assert r.min() >= 1 and r.max() <= n - 1 and (np.diff(np.sort(r, axis=1), axis=1) > 0).all()


def test_identical_spaces_score_one():
    from scrubvae_amd.eval import embed_quality as EQ
    X, _ = RC.rows(130, 5)
    w = RC.quality_of(X, X.copy(), 20, EQ)
    assert (w["pen_t"] == 0).all() and (w["pen_c"] == 0).all() and (w["rows_t"] == 0).all() and (w["rows_c"] == 0).all()
    assert (w["T"] == 1.0).all() and (w["C"] == 1.0).all() and (w["q"] == 1.0).all() and (w["r"] == 1.0).all() and w["auc"] == 1.0
    assert np.array_equal(w["hit"], 130 * np.arange(1, 21))


def test_independent_spaces_score_near_zero():
    """For a Y drawn on its own, |N_k^X(i) & N_k^Y(i)| is hypergeometric with mean k^2 / (n - 1) and a variance below that, so
    Q_NX(k) has mean k / (n - 1) and a standard deviation of about 1 / n = 0.003 at n = 301, and R_NX = Q_NX - k / (n - 1) up to
    the factor (n - 1) / (n - 1 - k) < 1.05: 0.05 is more than ten such deviations."""
    from scrubvae_amd.eval import embed_quality as EQ
    X, _ = RC.rows(301, 3)
    Y = np.random.default_rng(77).standard_normal((301, 2))
    w = RC.quality_of(X, Y, 12, EQ)
    print(f"R_NX of an independent Y: {w['r']}, auc {w['auc']}")
    assert np.abs(w["r"]).max() < 0.05 and abs(w["auc"]) < 0.05
    assert (w["T"] < 0.6).all() and (w["C"] < 0.6).all()     # the expected penalty of a random neighbour puts both near 0.5


def test_two_rows_and_the_grid():
    x, idx = RC.two_rows()
    assert np.array_equal(RC.ranks(x, idx), [[1], [1]])
    g = RC.grid_rows()
    r = RC.ranks(g, RC.knn(g, RC.GRID_K))
    assert np.array_equal(r, np.tile(np.arange(1, RC.GRID_K + 1), (len(g), 1)))   # ties and duplicates decided by index


def test_closing_helpers():
    from scrubvae_amd.eval import embed_quality as EQ
    n, K = 301, 12
    w = RC.quality(301, 3, 12)
    k = np.arange(1, K + 1)
    # elementwise over k: the array form holds the scalar form's bits
    assert RC.same(EQ.trustworthiness_from_penalty(w["pen_t"], n, k), w["T"])
    assert EQ.trustworthiness_from_penalty(0, 10, 3) == 1.0
    assert EQ.q_nx_from_hits(np.array([10, 40]), 10, np.array([1, 2]))[1] == 2.0
    assert RC.same(EQ.r_nx_from_q(np.array([1.0, 0.75, 1.0]), 4, np.array([1, 2, 3])), np.array([1.0, 0.25, np.nan]))
    assert EQ.auc_r_nx(np.array([0.5, 0.5, np.nan]), np.array([1, 2, 3])) == 0.5
    r = EQ.EmbeddingQuality(n, w["pen_t"], w["pen_c"], w["hit"])
    assert RC.same(r.trustworthiness, w["T"]) and RC.same(r.continuity, w["C"]) and RC.same(r.q_nx, w["q"]) and RC.same(r.r_nx, w["r"])
    assert r.auc_r_nx == w["auc"] and r.rows_at is None and r.intrusion_rows is None and "auc_r_nx=" in repr(r)
    # T and C are NaN from k = n / 2 on, R_NX at k = n - 1
    small = EQ.EmbeddingQuality(6, np.zeros(5, int), np.zeros(5, int), 6 * np.arange(1, 6))
    assert np.array_equal(np.isnan(small.trustworthiness), [False, False, True, True, True])
    assert np.array_equal(np.isnan(small.continuity), [False, False, True, True, True])
    assert np.array_equal(np.isnan(small.r_nx), [False, False, False, False, True]) and small.auc_r_nx == 1.0


X8 = np.arange(24.0).reshape(8, 3) ** 1.5
Y8 = X8[:, :2] + 1.0
IDX8 = (np.arange(8)[:, None] + np.array([1, 2, 3])) % 8


def untouched(monkeypatch):
    from scrubvae_amd import _lib

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", touched)


BAD_ROWS = [
    (X8, Y8[:7]),                                            # mismatched row counts
    (np.where(X8 > 50, np.inf, X8), Y8),                     # non-finite values
    (X8, np.where(Y8 > 50, np.nan, Y8)),
    (X8[:, 0], Y8),                                          # 1-D input
    (X8, Y8[:, 0]),
    (X8[:, :0], Y8),                                         # no feature
]
WIDE = np.zeros((200, 2))
BAD_COUNT = [(X8, 0), (X8, 4), (X8, 7), (WIDE, 91), (X8, 2.0), (X8, True), (X8, None)]    # 4 = n / 2; 91 > KNN_MAX_K, below n / 2
BAD_MAX = [(X8, 0), (X8, 8), (WIDE, 91), (X8, 2.0), (X8, True), (X8, None)]               # 8 > n - 1
BAD_AT = [0, 4, 2.0, True]                                                                # rows_at with max_neighbors = 3


def both_forms(fn, x, y, **kwargs):
    with pytest.raises(ValueError):
        fn(x, y, **kwargs)
    with pytest.raises(ValueError):
        fn(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(y)), **kwargs)


def test_argument_errors_before_device_work(monkeypatch):
    """a ValueError before the library is touched: loading it fails the test"""
    from scrubvae_amd.eval import continuity, embedding_quality, trustworthiness
    untouched(monkeypatch)
    for x, y in BAD_ROWS:
        for fn in (trustworthiness, continuity, embedding_quality):
            both_forms(fn, x, y)
    for x, k in BAD_COUNT:
        for fn in (trustworthiness, continuity):
            both_forms(fn, x, x[:, :2] + 1.0, n_neighbors=k)
    for x, k in BAD_MAX:
        both_forms(embedding_quality, x, x[:, :2] + 1.0, max_neighbors=k)
    for at in BAD_AT:
        both_forms(embedding_quality, X8, Y8, max_neighbors=3, rows_at=at)


def _with(row, col, value):
    a = IDX8.copy()
    a[row, col] = value
    return a


@pytest.mark.parametrize("x,idx", [
    (X8, _with(2, 1, IDX8[2, 0])),                           # a duplicate entry in a row
    (X8, _with(5, 2, 5)),                                    # a self entry
    (X8, _with(0, 0, 8)),                                    # out of range
    (X8, _with(7, 2, -1)),
    (X8, IDX8[:7]),                                          # the wrong shape
    (X8, IDX8[:, 0]),
    (X8, IDX8[:, :0]),
    (X8, np.tile(IDX8, (1, 3))),                             # more than n - 1 columns
    (X8, IDX8.astype(np.float64)),                           # not integers
    (X8, IDX8 > 3),
    (np.where(X8 > 50, np.nan, X8), IDX8),
    (X8[:, 0], IDX8),
    (X8[:1], np.zeros((1, 1), dtype=np.int64)),              # one row has no neighbour
])
def test_idx_errors_before_device_work(x, idx, monkeypatch):
    from scrubvae_amd.eval import neighbor_ranks
    untouched(monkeypatch)
    with pytest.raises(ValueError):
        neighbor_ranks(x, idx)
    with pytest.raises(ValueError):
        neighbor_ranks(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(idx)))


def test_checked_idx():
    from scrubvae_amd.eval import embed_quality as EQ
    for table in (IDX8, IDX8.astype(np.int16), torch.from_numpy(IDX8), IDX8[:, ::-1]):
        got = EQ._eq_idx(table, 8)
        assert got.dtype == np.int32 and got.flags.c_contiguous and np.array_equal(got, np.asarray(table))


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    lib = _lib.lib()
    work, K = lib.svae_rank_work, _lib.KNN_MAX_K
    assert work(1, 1) == 0 and work(0, 1) == 0 and work(-3, 1) == 0 and work(10, 0) == 0 and work(10, -1) == 0
    assert work(10, 10) == 0 and work(100, K + 1) == 0 and work(91, K) > 0
    # n x k x 16 bytes of sorted thresholds + column chunks (at most 8, fewer once the grid holds 512 blocks) x n x k x 4 bytes
    assert work(2, 1) == 2 * (16 + 4) and work(30, 29) == 30 * 29 * (16 + 4) and work(301, 12) == 301 * 12 * (16 + 5 * 4)
    assert work(1037, 30) == 1037 * 30 * (16 + 6 * 4) and work(64 * 512 + 7, K) == (64 * 512 + 7) * K * (16 + 4)
    assert work(2 ** 31 - 1, K) == (2 ** 31 - 1) * K * 20     # no overflow
    fake, E = 4096, _lib.ERR_ARG

    def ranks(X=fake, ld=3, d=3, n=40, idx=fake, k=3, w=fake, rank=fake):
        return lib.svae_knn_ranks(X, ld, d, n, idx, k, w, rank, None)

    for bad, text in ((dict(k=0), "neighbour count"), (dict(k=K + 1, n=200), "neighbour count"), (dict(k=40), "neighbour count"),
                      (dict(n=30, k=30), "neighbour count"), (dict(idx=None), "null"), (dict(w=None), "null"), (dict(rank=None), "null"),
                      (dict(n=1), "bad rows"), (dict(X=None), "bad rows"), (dict(ld=2), "bad rows"), (dict(d=0), "bad rows")):
        assert ranks(**bad) == E and text in _lib.last_error(), (bad, _lib.last_error())
    assert ranks(w=fake + 4) == _lib.ERR_ALIGN and "aligned" in _lib.last_error()

    def curves(rank=fake, n=40, k=3, row_k=0, pen=fake, hit=fake, rows=None):
        return lib.svae_rank_curves(rank, n, k, row_k, pen, hit, rows, None)

    for bad, text in ((dict(n=0), "bad sizes"), (dict(k=0), "bad sizes"), (dict(k=K + 1), "bad sizes"), (dict(row_k=-1), "row_k"),
                      (dict(row_k=4, rows=fake), "row_k"), (dict(rank=None), "null"), (dict(pen=None), "null"), (dict(hit=None), "null"),
                      (dict(row_k=2), "pen_row"), (dict(rows=fake), "pen_row")):
        assert curves(**bad) == E and text in _lib.last_error(), (bad, _lib.last_error())
    for bad in (dict(pen=fake + 4), dict(hit=fake + 4), dict(row_k=2, rows=fake + 4)):
        assert curves(**bad) == _lib.ERR_ALIGN and "aligned" in _lib.last_error(), bad
    import scrubvae_amd.eval as EV
    for name in ("neighbor_ranks", "trustworthiness", "continuity", "embedding_quality", "EmbeddingQuality"):
        assert callable(getattr(EV, name))
    from scrubvae_amd.eval import embed_quality as EQ
    assert EQ.KNN_MAX_K == _lib.KNN_MAX_K == RC.MAX_K == 90 and EQ._RANK_CALLS.keys() >= {"ranks", "curves"}


def test_header_and_sources_name_the_new_pieces():
    from scrubvae_amd import build
    assert "rank.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "rank.hip"))
    assert any(h.endswith("knn_buffer.h") for h in build.HEADERS) and any(h.endswith("pair_tiles.h") for h in build.HEADERS)


def test_scores_need_the_built_library(monkeypatch, tmp_path):
    """no fallback: without the library the scores fail at its first load, they are not computed on the host"""
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import embed_quality as EQ
    from scrubvae_amd.eval import trustworthiness
    assert trustworthiness is EQ.trustworthiness
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libscrubvae_hip.so"))
    with pytest.raises(RuntimeError, match="not found"):
        EQ._ranks_device(torch.from_numpy(X8), torch.from_numpy(IDX8.astype(np.int32)))
    with pytest.raises(RuntimeError, match="not found"):
        EQ._curves_device(torch.zeros(8, 3, dtype=torch.int32))
