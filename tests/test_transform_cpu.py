"""The numpy restatement of placing new rows on a fitted t-SNE map (tests/transform_checks.py) against sklearn and against a
long-double difference quotient, the blob case that settles the optimiser defaults, and everything about
scrubvae_amd/eval/embed_transform.py and the new neighbour functions that needs no device."""
import functools

import numpy as np
import pytest
import torch

from tests import silhouette_checks as SC
from tests import transform_checks as XC

LD = XC.LD


@pytest.mark.parametrize("m,n,d,k", XC.KNN[1:])
def test_cross_knn_restatement_equals_sklearn(m, n, d, k):
    nb = pytest.importorskip("sklearn.neighbors")
    q, x = XC.knn_case(m, n, d, k)
    assert XC.cross_ties(q, x, min(k, n - 1)) == 0, "a tie among the keys: change the seed"
    dist, idx = XC.cross_neighbors(q, x, k)
    want_d, want_i = nb.NearestNeighbors(n_neighbors=k, algorithm="kd_tree").fit(x).kneighbors(q)
    assert np.array_equal(idx, want_i)
    assert (np.abs(dist - want_d) <= np.spacing(np.maximum(dist, want_d))).all()      # 1 ulp
    assert (np.diff(dist, axis=1) >= 0).all()


def test_cross_knn_keeps_equal_rows_and_orders_ties():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0], [3.0, 4.0], [1.0, 0.0]])
    q = np.array([[0.0, 0.0], [3.0, 4.0], [0.5, 0.0]])
    dist, idx = XC.cross_neighbors(q, x, 4)
    assert idx.tolist() == [[0, 2, 1, 4], [3, 1, 4, 0], [0, 1, 2, 4]]
    assert dist[0].tolist() == [0.0, 0.0, 1.0, 1.0] and dist[1, 0] == 0.0 and dist[2].tolist() == [0.5] * 4


def test_label_transfer_equals_sklearn():
    nb = pytest.importorskip("sklearn.neighbors")
    xr, yr, xq, _ = XC.blob_case()
    lab = np.where(np.arange(len(yr)) % 11 == 0, -1, yr * 3 + 2)      # labels that are no 0..K-1 range, with "noise" rows
    for k in (1, 4, 15):
        _, idx = XC.cross_neighbors(xq, xr, k)
        want = nb.KNeighborsClassifier(n_neighbors=k, algorithm="kd_tree").fit(xr, lab).predict(xq)
        assert np.array_equal(XC.transfer_labels(idx, lab), want)
    # a constructed tie: two votes each for 7 and 5, then 9 -> the smallest of the tied labels
    x = np.array([[0.0], [1.0], [2.0], [3.0], [10.0]])
    lab = np.array([7, 5, 7, 5, 9])
    _, idx = XC.cross_neighbors(np.array([[1.4]]), x, 4)
    assert sorted(idx[0].tolist()) == [0, 1, 2, 3] and XC.transfer_labels(idx, lab).tolist() == [5]
    assert nb.KNeighborsClassifier(n_neighbors=4).fit(x, lab).predict([[1.4]]).tolist() == [5]
    from scrubvae_amd.eval import neighbors as NB
    assert NB._vote(lab[idx]).tolist() == [5] and NB._vote(np.array([[9, -1, -1, 9, 3]])).tolist() == [-1]


@pytest.mark.skipif(not XC.HAVE_LD, reason="needs an extended-precision long double")
def test_gradient_is_the_derivative_of_klrow():
    """g at exaggeration 1 against the central difference of the long-double objective with step h.  Along a coordinate,
    u = log(1 + |y - y_e|^2) has |u'| <= 1, |u''| <= 2, |u'''| <= 3, so the attraction part (sum p = 1) has a third derivative of
    at most 3; q = exp(-u) gives |q'| <= q, |q''| <= 3 q, |q'''| <= 10 q, so log(sum q) has one of at most 10 + 3 * 3 + 2 = 21.
    The quotient is within h^2 (3 + 21) / 6 = 4 h^2 of the derivative; the two long-double values carry (n + k + 20) roundings of
    2^-64 each, divided by 2 h; the restated g carries its own gate."""
    xr, _, xq, _ = XC.blob_case()
    g0 = np.random.default_rng(5)
    Yref = 12.0 * g0.standard_normal((len(xr), 2))
    idx, P, _ = XC.affinities(xr, xq, 30.0)
    Yq = XC.weighted_init(idx, P, Yref) + 0.7 * g0.standard_normal((len(xq), 2))
    R, rowq, _ = XC.cross_repulsion(Yq, Yref)
    _, g = XC.place_values(idx, P, 1.0, Yq, Yref, R, rowq)
    gate = XC.place_gate(idx, P, 1.0, Yq, Yref)
    assert (XC.TC.err(g, gate.g) <= gate.tol_g).all()
    h = 1e-5
    n, k = len(Yref), idx.shape[1]
    worst = 0.0
    for i in range(len(Yq)):
        for c in range(2):
            e = np.zeros(2)
            e[c] = h
            fp, fm = XC.objective_ld(idx[i], P[i], Yq[i] + e, Yref), XC.objective_ld(idx[i], P[i], Yq[i] - e, Yref)
            step = (LD(Yq[i, c] + h) - LD(Yq[i, c] - h))          # the step as it was taken
            quot = (fp - fm) / step
            tol = 4 * h * h + (n + k + 20) * 2.0 ** -64 * float(abs(fp) + abs(fm)) / (2 * h) + gate.tol_g[i, c]
            err = float(abs(LD(g[i, c]) - quot))
            worst = max(worst, err / tol)
            assert err <= tol, (i, c, err, tol)
    assert np.abs(g).max() > 1e-3          # a factor 2 or 4 on the gradient would be a thousand gates away
    print(f"gradient vs difference quotient: worst error / tolerance {worst:.3f}, max |g| {np.abs(g).max():.3f}")


def test_restated_sums_inside_their_gates():
    g0 = np.random.default_rng(1)
    Yref, Yq = 30.0 * g0.standard_normal((301, 2)), 30.0 * g0.standard_normal((40, 2))
    Yq[3] = Yref[17]                                  # a query on a map point: q = 1, no force
    R, rowq, _ = XC.cross_repulsion(Yq, Yref)
    gate = XC.cross_repulsion_gate(Yq, Yref)
    assert (XC.TC.err(R, gate.R) <= gate.tol_R).all() and (XC.TC.err(rowq, gate.rowq) <= gate.tol_rowq).all()
    alone, q1, _ = XC.cross_repulsion(Yq[3:4], Yref[17:18])
    assert np.array_equal(alone, np.zeros((1, 2))) and q1[0] == 1.0


@functools.lru_cache(maxsize=None)
def blob_embedding():
    man = pytest.importorskip("sklearn.manifold")
    xr, _, _, _ = XC.blob_case()
    emb = man.TSNE(method="exact", init="pca", random_state=0).fit_transform(xr).astype(np.float64)
    emb.setflags(write=False)
    return emb


def test_blob_case_settles_the_defaults():
    """every held-out row lands among its own blob and no further from its optimum than where it started, with the defaults"""
    from scrubvae_amd.eval import TSNEMap
    import inspect
    sig = inspect.signature(TSNEMap.transform).parameters
    assert {k: sig[k].default for k in XC.DEFAULTS} == XC.DEFAULTS and sig["init"].default == "weighted" and sig["batch_rows"].default == 1 << 18
    xr, yr, xq, yq = XC.blob_case()
    emb = blob_embedding()
    out = XC.transform(xr, emb, xq, XC.BLOB["perplexity"], **XC.DEFAULTS)
    near = XC.nearest_in_plane(out.Y, emb)
    worse = out.kl > out.kl_init
    print(f"blob case: rows in another blob {int((yr[near] != yq).sum())}, rows with a larger objective {int(worse.sum())}, "
          f"mean objective {out.kl_init.mean():.4f} -> {out.kl.mean():.4f}, clipped steps {out.clipped}, max |g| at the end {out.grad_norm.max():.2e}")
    assert (yr[near] == yq).all()
    assert not worse.any()
    assert out.kl.mean() < out.kl_init.mean()


XS, _ = SC.blobs(40, 3, 3, 0)
EMB = np.random.default_rng(0).standard_normal((40, 2))
NEW, _ = SC.blobs(9, 3, 3, 1)
BAD = np.arange(27).reshape(9, 3) == 7


@pytest.mark.parametrize("z_new,kw", [
    (np.where(BAD, np.nan, NEW), {}),
    (np.where(BAD, np.inf, NEW), {}),
    (torch.from_numpy(np.where(BAD, np.nan, NEW)), {}),
    (NEW[0], {}),                                          # 1-D
    (NEW[:0], {}),                                         # no rows
    (NEW[:, :2], {}),                                      # feature-count mismatch
    (NEW, dict(max_iter=-1)),
    (NEW, dict(max_iter=10.0)),
    (NEW, dict(max_iter=True)),
    (NEW, dict(learning_rate=0.0)),
    (NEW, dict(learning_rate=-0.1)),
    (NEW, dict(learning_rate=float("inf"))),
    (NEW, dict(momentum=1.0)),
    (NEW, dict(momentum=-0.1)),
    (NEW, dict(exaggeration=0.9)),
    (NEW, dict(exaggeration=float("nan"))),
    (NEW, dict(max_grad_norm=-1.0)),
    (NEW, dict(init="pca")),
    (NEW, dict(init=np.zeros((8, 2)))),
    (NEW, dict(init=np.zeros((9, 3)))),
    (NEW, dict(init=np.where(np.arange(18).reshape(9, 2) == 3, np.nan, 0.0))),
    (NEW, dict(batch_rows=0)),
    (NEW, dict(batch_rows=2.5)),
])
def test_transform_argument_errors_before_device_work(z_new, kw):
    """this machine has no device: a ValueError, not the "no device is available" RuntimeError, shows the order"""
    import scrubvae_amd.eval as E
    with pytest.raises(ValueError):
        E.TSNEMap(XS, EMB, perplexity=5.0).transform(z_new, **kw)
    with pytest.raises(ValueError):
        E.tsne_transform(XS, EMB, z_new, perplexity=5.0, **kw)


@pytest.mark.parametrize("z_ref,emb,perplexity", [
    (np.where(np.arange(120).reshape(40, 3) == 7, np.nan, XS), EMB, 5.0),
    (XS[0], EMB, 5.0),
    (XS, EMB[:39], 5.0),
    (XS, np.zeros((40, 3)), 5.0),
    (XS, np.where(np.arange(80).reshape(40, 2) == 5, np.inf, EMB), 5.0),
    (XS, EMB, 0.0),
    (XS, EMB, 0.3),                  # floor(3 perplexity) = 0
    (XS, EMB, 30.5),                 # 91 neighbours
    (XS, EMB, 40.0),                 # perplexity >= n
    (XS[:20], EMB[:20], 20.0),       # perplexity >= n below the cap
    (XS, EMB, float("nan")),
    (XS, EMB, "30"),
])
def test_map_argument_errors(z_ref, emb, perplexity):
    import scrubvae_amd.eval as E
    with pytest.raises(ValueError):
        E.TSNEMap(z_ref, emb, perplexity=perplexity)
    with pytest.raises(ValueError):
        E.tsne_transform(z_ref, emb, NEW, perplexity=perplexity)


def test_map_holds_its_arguments_without_a_device():
    import scrubvae_amd.eval as E
    m = E.TSNEMap(XS.astype(np.float32), torch.from_numpy(EMB), perplexity=5.0)
    assert m.n_neighbors_ == 15 and E.TSNEMap(XS[:12], EMB[:12], perplexity=5.0).n_neighbors_ == 12     # min(n, floor(3 perplexity))
    with pytest.raises(ValueError):
        E.TSNEMap.from_fit(E.TSNE(), XS)                                   # not fitted
    est = E.TSNE(perplexity=5.0)
    est.embedding_ = EMB
    assert E.TSNEMap.from_fit(est, XS).n_neighbors_ == 15
    q, max_iter, lr, momentum, exag, clip, init, batch_rows = m._check(NEW.astype(np.float32), 3, 1, 0, 2, 0, np.arange(18).reshape(9, 2), 2 ** 40)
    assert q.dtype == np.float64 and (max_iter, lr, momentum, exag, clip, batch_rows) == (3, 1.0, 0.0, 2.0, 0.0, 2 ** 26)
    assert init.dtype == np.float64 and np.array_equal(init, np.arange(18.0).reshape(9, 2))


@pytest.mark.parametrize("ref,lab,q,k,kw", [
    (XS, None, NEW[:, :2], 3, {}),
    (XS, None, np.where(BAD, np.nan, NEW), 3, {}),
    (XS, None, NEW, 0, {}),
    (XS, None, NEW, 41, {}),                   # more than the reference rows
    (np.zeros((200, 2)), None, np.zeros((3, 2)), 91, {}),
    (XS, None, NEW, 2.0, {}),
    (XS, np.arange(39), NEW, 3, {}),
    (XS, np.arange(40.0), NEW, 3, {}),
    (XS, np.arange(40), NEW, 3, dict(noise_label=-1.0)),
])
def test_neighbour_argument_errors_before_device_work(ref, lab, q, k, kw):
    import scrubvae_amd.eval as E
    with pytest.raises(ValueError):
        if lab is None:
            E.kneighbors_cross(ref, q, k)
        else:
            E.knn_transfer_labels(ref, lab, q, k, **kw)


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    lib = _lib.lib()
    K = _lib.KNN_MAX_K
    work = lib.svae_knn_cross_work
    assert work(0, 10, 1) == 0 and work(10, 0, 1) == 0 and work(10, 10, 0) == 0 and work(10, 10, 11) == 0 and work(10, 1000, K + 1) == 0
    # column chunks x queries padded to 64 x k x 12; chunks: at most 8, at most one per 64-column tile, 1 once the grid holds 512 blocks
    assert work(1, 1, 1) == 64 * 12 and work(10, 10, 10) == 64 * 10 * 12
    assert work(63, 65, 15) == 2 * 64 * 15 * 12 and work(65, 1037, K) == 6 * 128 * K * 12     # 17 tiles: 6 chunks of 3
    assert work(40000, 200, 5) == 1 * 40000 * 5 * 12                                           # 625 row tiles: one chunk
    assert work(6400, 6400, 7) == 6 * 6400 * 7 * 12                                            # 100 row tiles: ceil(512 / 100)
    rep = lib.svae_tsne_cross_repulsion_work
    assert rep(0, 10, 0) == 0 and rep(10, 0, 0) == 0 and rep(2 ** 26 + 1, 10, 0) == 0 and rep(10, 2 ** 26 + 1, 0) == 0
    assert rep(10, 10, -1) == 0 and rep(10, 10, _lib.TSNE_MAX_CHUNKS + 1) == 0
    # chunks x 3 sums x queries padded to 256; chunks = 0: min(8, tiles) ranges of ceil(tiles / that) 64-column tiles, whatever m
    assert rep(1, 1, 0) == 3 * 256 and rep(300, 301, 0) == 5 * 3 * 512 and rep(300, 301, 3) == 3 * 3 * 512 and rep(1, 1037, 8) == 6 * 3 * 256
    for n in (1, 64, 301, 1037, 20000, 200000):
        chunks = {m: rep(m, n, 0) // (3 * (-(-m // 256) * 256)) for m in (1, 257, 10 ** 6)}
        tiles = -(-n // 64)
        assert chunks[1] == chunks[257] == chunks[10 ** 6] == -(-tiles // -(-tiles // min(8, tiles))), (n, chunks)
        assert rep(5, n, 0) == rep(5, n, 8)
    assert rep(10 ** 6, 20000, 0) == 8 * 3 * 1000192 and rep(10 ** 6, 1037, 0) == 6 * 3 * 1000192
    fake = 4096
    E = _lib.ERR_ARG
    assert lib.svae_knn_cross(None, 2, 5, fake, 2, 10, 2, 3, fake, fake, fake, None) == E
    assert lib.svae_knn_cross(fake, 2, 5, None, 2, 10, 2, 3, fake, fake, fake, None) == E
    assert lib.svae_knn_cross(fake, 2, 0, fake, 2, 10, 2, 3, fake, fake, fake, None) == E
    assert lib.svae_knn_cross(fake, 2, 5, fake, 2, 10, 2, 11, fake, fake, fake, None) == E          # k > n
    assert lib.svae_knn_cross(fake, 1, 5, fake, 2, 10, 2, 3, fake, fake, fake, None) == E           # ldq < d
    assert lib.svae_knn_cross(fake, 2, 5, fake, 2, 10, 2, 3, None, fake, fake, None) == E and "null" in _lib.last_error()
    far = fake + 16 * 100
    cross = lib.svae_tsne_cross_repulsion
    assert cross(fake, 0, far, 10, 0, fake, fake, fake, None) == E and cross(fake, 10, far, 0, 0, fake, fake, fake, None) == E
    assert cross(fake, 10, far, 10, 9, fake, fake, fake, None) == E
    assert cross(fake, 10, far, 10, 0, None, fake, fake, None) == E and "null" in _lib.last_error()
    assert cross(fake, 100, fake, 100, 0, fake, fake, fake, None) == E and "overlap" in _lib.last_error()
    assert cross(fake, 100, fake + 16 * 99, 5, 0, fake, fake, fake, None) == E and "overlap" in _lib.last_error()
    assert cross(fake + 16 * 4, 3, fake, 5, 0, fake, fake, fake, None) == E and "overlap" in _lib.last_error()
    step = lib.svae_tsne_place_step
    assert step(fake, fake, 3, 1.0, fake, fake, fake, fake, None, None, 0.8, 0.1, 0.25, 10, None, None, None) == E      # nothing to do
    assert step(fake, fake, 3, 1.0, fake, fake, fake, fake, fake, None, 0.8, 0.1, 0.25, 10, fake, fake, None) == E      # update without gains
    assert step(fake, fake, 0, 1.0, fake, fake, fake, fake, fake, fake, 0.8, 0.1, 0.25, 10, fake, fake, None) == E
    assert step(fake, fake, K + 1, 1.0, fake, fake, fake, fake, fake, fake, 0.8, 0.1, 0.25, 10, fake, fake, None) == E
    assert step(fake, fake, 3, 1.0, fake, fake, fake, fake, fake, fake, 0.8, 0.1, 0.25, 0, fake, fake, None) == E
    assert step(fake, fake, 3, 1.0, fake, fake, fake, fake, fake, fake, 0.8, 0.1, -1.0, 10, fake, fake, None) == E
    assert step(None, fake, 3, 1.0, fake, fake, fake, fake, fake, fake, 0.8, 0.1, 0.25, 10, fake, fake, None) == E and "null" in _lib.last_error()
    import scrubvae_amd.eval as EV
    from scrubvae_amd.eval import embed_transform as ET
    from scrubvae_amd.eval import neighbors as NB
    for name in ("TSNEMap", "tsne_transform", "kneighbors_cross", "knn_transfer_labels"):
        assert callable(getattr(EV, name))
    assert ET._PLACE_CALLS.keys() >= {"knn", "search", "repulsion", "step", "host_reads"} and ET._PLACE_LAST.keys() >= {"work", "chunks"}
    assert "cross" in NB._KNN_CALLS
