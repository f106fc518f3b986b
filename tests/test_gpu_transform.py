"""TSNEMap / tsne_transform / kneighbors_cross / knn_transfer_labels (csrc/knn.hip, csrc/tsne.hip) on the device, stage by stage
against the numpy restatement and the long-double truth of tests/transform_checks.py, whose gates are derived there.

The cross kNN has a strict key, so it is held to equal indices and equal bytes of the distances.  The cross repulsion, a sum whose
chunking the device chooses, is held to its gate, to equal bytes between two calls and to equal bytes of a row whatever else is in
the launch.  The place step is elementwise given R and rowq (stored order, correctly rounded division and square root), so
positions, update, gains and gradsq are held to equal bytes of the restatement, which is itself inside the gates; klrow, which
holds logarithms, to its gate.  The whole descent is not compared with the restatement (the gains rule and the clip are
discontinuous): it is held to the blob case's two conditions, to its own objective and to equal bytes across ways of calling it."""
import functools

import numpy as np
import pytest
import torch

from tests import knn_checks as KC
from tests import transform_checks as XC
from tests import tsne_checks as TC

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a)).to(dtype).cuda()


def device_knn_cross(q, x, k):
    from scrubvae_amd import _lib, ops
    lib = _lib.lib()
    (m, d), n = q.shape, len(x)
    nbytes = lib.svae_knn_cross_work(m, n, k)
    assert nbytes > 0
    Q, X = dev(q), dev(x)
    work = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    idx = torch.full((m, k), -1, dtype=torch.int32, device="cuda")
    dist = torch.full((m, k), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.svae_knn_cross(Q.data_ptr(), d, m, X.data_ptr(), d, n, d, k, work.data_ptr(), idx.data_ptr(), dist.data_ptr(), ops._stream()),
               "knn_cross")
    return dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64), nbytes // (-(-m // 64) * 64 * k * 12)


@pytest.mark.parametrize("m,n,d,k", XC.KNN)
def test_cross_knn_equals_the_restatement(m, n, d, k):
    q, x = XC.knn_case(m, n, d, k)
    want_d, want_i = XC.cross_neighbors(q, x, k)
    dist, idx, chunks = device_knn_cross(q, x, k)
    assert np.array_equal(idx, want_i) and bits(dist) == bits(want_d)
    assert chunks == min(8, -(-n // 64)) or (n, chunks) == (1037, 6)          # a small grid splits the columns
    again = device_knn_cross(q, x, k)
    assert np.array_equal(again[1], idx) and bits(again[0]) == bits(dist)


def test_cross_knn_on_a_wide_grid():
    m, n, d, k = XC.KNN_WIDE
    q, x = XC.knn_case(m, n, d, k)
    dist, idx, chunks = device_knn_cross(q, x, k)
    assert chunks == 1                                                        # 625 row tiles fill the grid
    rows = np.concatenate([np.random.default_rng(0).choice(m - 64, size=200, replace=False), np.arange(m - 64, m)])
    want_d, want_i = XC.cross_neighbors(q, x, k, rows)
    assert np.array_equal(idx[rows], want_i) and bits(dist[rows]) == bits(want_d)
    assert (idx >= 0).all() and (idx < n).all() and np.isfinite(dist).all() and (np.diff(dist, axis=1) >= 0).all()


def test_cross_knn_keeps_equal_rows_and_orders_ties():
    x = KC.grid_rows()                                        # 300 rows on 25 distinct points
    q = np.concatenate([x[:70], np.random.default_rng(1).integers(0, 5, size=(30, 2)).astype(np.float64), x[290:] + 0.5])
    k = 40
    want_d, want_i = XC.cross_neighbors(q, x, k)
    assert XC.cross_ties(q, x, k) == len(q) and (want_d[:70, 0] == 0.0).all()
    dist, idx, _ = device_knn_cross(q, x, k)
    assert np.array_equal(idx, want_i) and bits(dist) == bits(want_d)
    first = np.array([np.flatnonzero((x == r).all(1))[0] for r in q[:70]])
    assert np.array_equal(idx[:70, 0], first) and (dist[:70, 0] == 0.0).all()         # the lowest equal reference row, at distance 0


def test_cross_knn_of_a_set_against_itself_is_knn_plus_the_row():
    from scrubvae_amd.eval import kneighbors, kneighbors_cross
    n, d, k = 301, 3, 5
    x, _, want_d, want_i = KC.case(n, d, k)
    assert KC.ties(x, k + 1) == (0, 0)
    dist, idx = kneighbors(x, k)
    cd, ci = kneighbors_cross(x, x, k + 1)
    assert np.array_equal(ci[:, 0], np.arange(n)) and (cd[:, 0] == 0.0).all()
    assert np.array_equal(ci[:, 1:], idx) and np.array_equal(idx, want_i) and bits(cd[:, 1:]) == bits(dist)


def device_cross_repulsion(Yq, Yref, chunks):
    from scrubvae_amd import _lib, ops
    lib = _lib.lib()
    m, n = len(Yq), len(Yref)
    Yd, Rd = dev(Yq), dev(Yref)
    words = lib.svae_tsne_cross_repulsion_work(m, n, chunks)
    assert words > 0
    work = torch.full((words,), float("nan"), dtype=torch.float64, device="cuda")
    R = torch.full((m, 2), float("nan"), dtype=torch.float64, device="cuda")
    rowq = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.svae_tsne_cross_repulsion(Yd.data_ptr(), m, Rd.data_ptr(), n, chunks, work.data_ptr(), R.data_ptr(), rowq.data_ptr(),
                                             ops._stream()), "tsne_cross_repulsion")
    assert torch.equal(Yd.cpu(), torch.from_numpy(np.array(Yq))) and torch.equal(Rd.cpu(), torch.from_numpy(np.array(Yref)))
    return R.cpu().numpy(), rowq.cpu().numpy(), words // (3 * (-(-m // 256) * 256))


@functools.lru_cache(maxsize=None)
def repulsion_case(m, n, scale):
    g = np.random.default_rng(1000 * m + n)
    Yq, Yref = scale * g.standard_normal((m, 2)), scale * g.standard_normal((n, 2))
    Yq.setflags(write=False), Yref.setflags(write=False)
    return Yq, Yref, XC.cross_repulsion_gate(Yq, Yref)


@pytest.mark.parametrize("scale", [1e-4, 30.0])
@pytest.mark.parametrize("m,n", XC.REPULSION)
def test_cross_repulsion_inside_the_gate(m, n, scale):
    Yq, Yref, g = repulsion_case(m, n, scale)
    tiles = -(-n // 64)
    worst, auto = 0.0, None
    for chunks in (1, 2, 3, 4, 5, 6, 7, 8, 0):
        R, rowq, made = device_cross_repulsion(Yq, Yref, chunks)
        assert made == -(-tiles // -(-tiles // min(tiles, chunks if chunks else 8)))       # whole 64-column tiles per chunk
        eR, eq = TC.err(R, g.R), TC.err(rowq, g.rowq)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(g.tol_R > 0, eR / g.tol_R, 0))), float((eq / g.tol_rowq).max()))
        assert (eR <= g.tol_R).all() and (eq <= g.tol_rowq).all()
        again = device_cross_repulsion(Yq, Yref, chunks)
        assert bits(again[0]) == bits(R) and bits(again[1]) == bits(rowq)
        if chunks == 0:
            auto = (R, rowq, made)
    print(f"cross repulsion m={m} n={n} |Y|~{scale}: worst error / gate {worst:.4f}, chunks = 0 made {auto[2]}")
    # a row's bits do not depend on what else is in the launch
    for i in sorted({0, m // 2, m - 1}):
        R1, q1, made1 = device_cross_repulsion(Yq[i:i + 1], Yref, 0)
        assert made1 == auto[2] and bits(R1[0]) == bits(auto[0][i]) and bits(q1[0]) == bits(auto[1][i])


def test_cross_repulsion_of_a_query_on_a_map_point():
    R, rowq, _ = device_cross_repulsion(np.array([[0.25, -3.0]]), np.array([[0.25, -3.0]]), 0)
    assert np.array_equal(R, np.zeros((1, 2))) and np.array_equal(rowq, [1.0])          # q = 1, no force
    Yq, Yref, _ = repulsion_case(257, 65, 30.0)
    Yq = np.array(Yq)
    Yq[256] = Yref[64]                                                                   # the last query on the last map point
    g = XC.cross_repulsion_gate(Yq, Yref)
    for chunks in (1, 2):
        R, rowq, _ = device_cross_repulsion(Yq, Yref, chunks)
        assert (TC.err(R, g.R) <= g.tol_R).all() and (TC.err(rowq, g.rowq) <= g.tol_rowq).all() and rowq[256] > 1.0


def place_case(m, n, k, scale, seed):
    g = np.random.default_rng(seed)
    Yref, Yq = scale * g.standard_normal((n, 2)), scale * g.standard_normal((m, 2))
    idx = np.stack([g.choice(n, size=k, replace=False) for _ in range(m)]).astype(np.int64)
    P = g.random((m, k)) * (g.random((m, k)) > 0.2)                   # a fifth of the entries are p = 0
    P[5] = 0.0
    P[5, 2] = 1.0
    P = P / P.sum(1, keepdims=True)
    R, rowq, _ = XC.cross_repulsion(Yq, Yref)
    R = R * (1 + 0.1 * g.standard_normal((m, 2)))                      # any numbers: the kernel takes them as given
    update = scale * 0.01 * g.standard_normal((m, 2))
    gains = g.choice([0.01, 0.0105, 0.8, 1.0, 1.2, 3.4], size=(m, 2))
    return idx, P, Yq, Yref, R, rowq, update, gains


def device_place(idx, P, exag, Yq, Yref, R, rowq, update, gains, momentum, lr, clip, look=True, move=True):
    from scrubvae_amd import _lib, ops
    m, k = idx.shape
    t = dict(idx=torch.from_numpy(idx.astype(np.int32)).cuda(), P=dev(P), Y=dev(Yq), Yref=dev(Yref), R=dev(R), rowq=dev(rowq), update=dev(update),
             gains=dev(gains), kl=torch.full((m,), float("nan"), dtype=torch.float64, device="cuda"),
             gsq=torch.full((m,), float("nan"), dtype=torch.float64, device="cuda"))
    _lib.check(_lib.lib().svae_tsne_place_step(t["idx"].data_ptr(), t["P"].data_ptr(), k, exag, t["Y"].data_ptr(), t["Yref"].data_ptr(),
                                               t["R"].data_ptr(), t["rowq"].data_ptr(), t["update"].data_ptr() if move else None,
                                               t["gains"].data_ptr() if move else None, momentum, lr, clip, m,
                                               t["kl"].data_ptr() if look else None, t["gsq"].data_ptr() if look else None, ops._stream()),
               "tsne_place_step")
    return {k_: v.cpu().numpy() for k_, v in t.items()}


@pytest.mark.parametrize("m,n,k,exag,scale,clip", [(300, 257, 90, 1.0, 20.0, 0.25), (300, 257, 90, 4.0, 20.0, 1e9), (65, 40, 7, 4.0, 1.0, 0.05),
                                                   (257, 64, 30, 1.0, 1e-2, 0.0)])
def test_place_step_equals_the_restatement(m, n, k, exag, scale, clip):
    idx, P, Yq, Yref, R, rowq, update, gains = place_case(m, n, k, scale, m + k)
    assert (P == 0).sum() > m and np.array_equal(P[5] > 0, np.arange(k) == 2)
    momentum, lr = 0.8, 0.1 * scale
    want_Y, want_update, want_gains, want_kl, want_gsq, bit = XC.place_step(idx, P, exag, Yq, Yref, R, rowq, update, gains, momentum, lr, clip)
    if clip == 0.25:
        assert bit.any() and not bit.all()                             # the clip bites some rows and leaves others
    elif clip == 0.05:
        assert bit.all()
    else:
        assert not bit.any()
    # the restatement is inside the gates of the long-double truth
    gate = XC.place_gate(idx, P, exag, Yq, Yref, R, rowq)
    kl_fp64, g_fp64 = XC.place_values(idx, P, exag, Yq, Yref, R, rowq)
    assert (TC.err(g_fp64, gate.g) <= gate.tol_g).all() and (TC.err(kl_fp64, gate.klrow) <= gate.tol_klrow).all()
    got = device_place(idx, P, exag, Yq, Yref, R, rowq, update, gains, momentum, lr, clip)
    assert bits(got["gains"]) == bits(want_gains) and bits(got["update"]) == bits(want_update)
    assert bits(got["Y"]) == bits(want_Y) and np.abs(want_Y - Yq).max() > 0
    assert bits(got["gsq"]) == bits(want_gsq)
    assert bits(got["Yref"]) == bits(Yref) and bits(got["R"]) == bits(R) and bits(got["rowq"]) == bits(rowq)     # inputs untouched
    e = TC.err(got["kl"], gate.klrow)
    print(f"place step m={m} k={k} exag={exag} clip={clip}: klrow worst error / gate {float((e / gate.tol_klrow).max()):.4f}, "
          f"clipped rows {int(bit.sum())}")
    assert (e <= gate.tol_klrow).all()
    # without a look: the same step, klrow and gradsq untouched
    blind = device_place(idx, P, exag, Yq, Yref, R, rowq, update, gains, momentum, lr, clip, look=False)
    assert bits(blind["Y"]) == bits(want_Y) and bits(blind["gains"]) == bits(want_gains) and np.isnan(blind["kl"]).all() and np.isnan(blind["gsq"]).all()
    # evaluation only: nothing moves, klrow as before, gradsq of the clipped gradient without gains
    gc = XC.clip(g_fp64, clip)
    ev = device_place(idx, P, exag, Yq, Yref, R, rowq, update, gains, momentum, lr, clip, move=False)
    assert bits(ev["Y"]) == bits(Yq) and bits(ev["update"]) == bits(update) and bits(ev["gains"]) == bits(gains)
    assert bits(ev["kl"]) == bits(got["kl"]) and bits(ev["gsq"]) == bits(gc[:, 0] * gc[:, 0] + gc[:, 1] * gc[:, 1])
    # the plain gradient, through gradsq without the clip, inside its gate: |g|^2 moves by at most 2 |g| tol
    plain = device_place(idx, P, exag, Yq, Yref, R, rowq, update, gains, momentum, lr, 0.0, move=False)
    g2 = (gate.g * gate.g).sum(1)
    tol2 = (2 * np.abs(gate.g.astype(np.float64)) * gate.tol_g).sum(1) + 4 * TC.U * g2.astype(np.float64) + (gate.tol_g ** 2).sum(1)
    assert (TC.err(plain["gsq"], g2) <= tol2).all()


@functools.lru_cache(maxsize=None)
def blob_map():
    """the blob case's reference rows embedded by the device TSNE"""
    from scrubvae_amd.eval import TSNE
    xr, _, _, _ = XC.blob_case()
    est = TSNE(max_iter=500, random_state=0).fit(xr)
    est.embedding_.setflags(write=False)
    return est


def test_whole_transform_on_the_blob_case():
    from scrubvae_amd.eval import DensityMap, TSNEMap, embed, embed_transform as ET, tsne_transform
    xr, yr, xq, yq = XC.blob_case()
    est = blob_map()
    emb, m, its = est.embedding_, len(xq), XC.DEFAULTS["max_iter"]
    tmap = TSNEMap.from_fit(est, xr)
    before = dict(ET._PLACE_CALLS)
    Y = tmap.transform(xq)
    made = {k: ET._PLACE_CALLS[k] - before[k] for k in before}
    assert Y.shape == (m, 2) and Y.dtype == np.float64 and np.isfinite(Y).all()
    assert tmap.kl_rows_.shape == (m,) and tmap.grad_norm_rows_.shape == (m,) and tmap.neighbors_.shape == (m, 90)
    # one batch: max_iter + 1 repulsion and step launches, one search, one kNN, and the one host read after the last launch
    assert made == dict(knn=1, search=1, repulsion=its + 1, step=its + 1, host_reads=1)
    assert ET._PLACE_LAST["batches"] == 1 and ET._PLACE_LAST["reads_at"] == [(2 * (its + 1) + 2,) * 2]
    # the stages it starts from: the restatement's neighbours, and the device's P of their distances (test_gpu_tsne.py holds the
    # search to the restatement; its P carries the device's exp, so what follows takes it as the input it is)
    idx, _, s = XC.affinities(xr, xq, 30.0)
    assert s.near >= 1e-9 and s.tiny >= 1e-12 and np.array_equal(tmap.neighbors_, idx)
    dist, _ = XC.cross_neighbors(xq, xr, 90)
    P = embed._search_device(dev(dist * dist), 30.0)[0].cpu().numpy()
    assert (TC.err(P, TC.search_truth(dist * dist, s.used)) <= TC.p_gate(TC.search_truth(dist * dist, s.used))).all()
    # (a) next to a map point of its own blob; (b) no worse than where it started
    near = XC.nearest_in_plane(Y, emb)
    Y0 = XC.weighted_init(idx, P, emb)
    start = TSNEMap.from_fit(est, xr)
    assert bits(start.transform(xq, max_iter=0)) == bits(Y0)                   # the initial positions, evaluated by the device
    print(f"blob case on the device: rows in another blob {int((yr[near] != yq).sum())}, mean objective {start.kl_rows_.mean():.4f} -> "
          f"{tmap.kl_rows_.mean():.4f}, rows with a larger one {int((tmap.kl_rows_ > start.kl_rows_).sum())}, max |g| {tmap.grad_norm_rows_.max():.2e}")
    assert (yr[near] == yq).all()
    assert (tmap.kl_rows_ <= start.kl_rows_).all()
    # kl_rows_ and grad_norm_rows_ are the objective and its gradient at the returned positions
    gate = XC.place_gate(idx, P, 1.0, Y, emb)
    e = TC.err(tmap.kl_rows_, gate.klrow)
    print(f"  kl_rows_ worst error / gate {float((e / gate.tol_klrow).max()):.4f}")
    assert (e <= gate.tol_klrow).all()
    gn = np.sqrt((gate.g * gate.g).sum(1)).astype(np.float64)
    assert (np.abs(tmap.grad_norm_rows_ - gn) <= np.sqrt((gate.tol_g ** 2).sum(1)) + 4 * TC.U * gn).all()
    # the same bytes however it is called
    kl = tmap.kl_rows_
    for how, got in [("again", TSNEMap.from_fit(est, xr).transform(xq)),
                     ("device float32 rows", tmap.transform(torch.from_numpy(xq.astype(np.float32)).cuda())),
                     ("one call", tsne_transform(xr, emb, xq, perplexity=est.perplexity))]:
        assert bits(got) == bits(Y), how
    assert bits(tmap.kl_rows_) == bits(kl)
    before = dict(ET._PLACE_CALLS)
    small = tmap.transform(xq, batch_rows=7)
    made = {k: ET._PLACE_CALLS[k] - before[k] for k in before}
    batches = -(-m // 7)
    assert bits(small) == bits(Y) and bits(tmap.kl_rows_) == bits(kl)
    assert made == dict(knn=batches, search=batches, repulsion=batches * (its + 1), step=batches * (its + 1), host_reads=batches)
    assert ET._PLACE_LAST["reads_at"] == [(2 * (its + 1) + 2,) * 2] * batches
    perm = np.random.default_rng(0).permutation(m)
    mixed = tmap.transform(xq[perm])
    assert bits(mixed[np.argsort(perm)]) == bits(Y) and bits(tmap.kl_rows_[np.argsort(perm)]) == bits(kl)
    # a given init is used as given
    given = tmap.transform(xq, init=Y0)
    assert bits(given) == bits(Y)
    # the placed rows go straight into the density map of the reference embedding
    regions = DensityMap().fit(emb).predict(Y)
    assert regions.shape == (m,) and regions.dtype.kind in "iu"


def test_neighbour_front_ends():
    from scrubvae_amd.eval import kneighbors_cross, knn_transfer_labels
    xr, yr, xq, _ = XC.blob_case()
    lab = np.where(np.arange(len(yr)) % 11 == 0, -1, yr * 3 + 2)
    for k in (1, 4, 15):
        want_d, want_i = XC.cross_neighbors(xq, xr, k)
        want_l = XC.transfer_labels(want_i, lab)
        for ref, new in [(xr, xq), (torch.from_numpy(xr.astype(np.float32)).cuda(), torch.from_numpy(xq).cuda()), (xr, torch.from_numpy(xq).cuda())]:
            dist, idx = kneighbors_cross(ref, new, k)
            assert idx.dtype == np.int64 and np.array_equal(idx, want_i) and bits(dist) == bits(want_d)
            assert np.array_equal(kneighbors_cross(ref, new, k, return_distance=False), want_i)
            got = knn_transfer_labels(ref, lab, new, k, noise_label=-1)
            assert np.array_equal(got, want_l) and got.dtype == lab.dtype
        assert np.array_equal(knn_transfer_labels(xr, torch.from_numpy(lab), xq, k), want_l)
    assert (XC.transfer_labels(XC.cross_neighbors(xq, xr, 15)[1], lab) == -1).sum() == (knn_transfer_labels(xr, lab, xq, 15) == -1).sum()
