"""GPU checks of csrc/kmeans.hip and scrubvae_amd.eval.KMeans against the fp64 restatement of tests/kmeans_checks.py: the
assignment bit for bit, the per-cluster sums and new centres within the bounds of re-ordered fp64 sums, one Lloyd step at a time,
and whole fits on data whose assignment margins exceed what those bounds can move."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from tests import kmeans_checks as KC

pytestmark = pytest.mark.gpu

U = KC.U


def planted(n, d, K, seed):
    """float32 latents: K clusters with column offsets |mean| >> std, a constant column, a duplicated column and one tight
    component (std 1e-3) about 30 units from the global mean (the generator of test_gpu_gmm.py)"""
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


def _rows(x32, K):
    """(_Centred rows on the device, _Lloyd state, the device's own centred A read back [n, d])"""
    from scrubvae_amd.eval import cluster as C
    dev = torch.device("cuda")
    R = C._Centred(torch.from_numpy(np.ascontiguousarray(x32)).cuda(), K, dev)
    return R, C._Lloyd(R), R.A[:, :R.d].cpu().numpy()


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


SHAPES = [(1, 1, 1), (63, 3, 2), (64, 16, 63), (65, 17, 64), (257, 33, 65), (1000, 128, 130), (1000, 1, 2), (65, 128, 1), (257, 16, 130),
          (64, 33, 63), (63, 17, 65), (1, 3, 64)]


def _case(n, d, K):
    g = np.random.default_rng(1000 * n + 10 * d + K)
    x = (g.normal(size=(n, d)) + 5.0 * g.normal(size=d)).astype(np.float32)
    R, it, A = _rows(x, K)
    # centres: rows of A where there are enough (those rows are at distance 0), others near rows; centres 0 and 1 are duplicates
    C = A[g.integers(0, n, K)] + (g.random(K) < 0.5)[:, None] * g.normal(size=(K, d))
    C[0] = A[0]
    if K > 1:
        C[1] = C[0]
    return g, R, it, A, np.ascontiguousarray(C)


def _assign_all(it, C, prev, want_D=True):
    n, K = it.R.n, C.shape[0]
    i32 = dict(dtype=torch.int32, device="cuda")
    out = dict(label=torch.full((n,), -7, **i32), dist=torch.empty(n, **it.R.f64), gap=torch.empty(n, **it.R.f64),
               D=torch.empty(n, K, **it.R.f64) if want_D else None, changed=torch.full((1,), 99, **i32))
    it.assign(_dev(C), prev=_dev(prev, torch.int32), part=it.ipart, **out)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}, it.inertia()


@pytest.mark.parametrize("n,d,K", SHAPES)
def test_assignment_equals_restatement_bit_for_bit(n, d, K):
    g, R, it, A, C = _case(n, d, K)
    prev = g.integers(0, K, n)
    got, inertia = _assign_all(it, C, prev)
    labels, dist, gap, s = KC.assign(A, C)
    assert np.array_equal(got["label"], labels)
    assert np.array_equal(got["dist"], dist) and np.array_equal(got["gap"], gap) and np.array_equal(got["D"], s)
    assert int(got["changed"][0]) == int((prev != labels).sum())
    exact = math.fsum(dist)
    assert abs(inertia - exact) <= (n - 1) * U * exact
    # duplicated centres resolve to the lower index; a row equal to a centre is at distance 0
    assert not (got["label"] == 1).any() or K == 1
    assert got["label"][0] == 0 and got["dist"][0] == 0.0
    if K == 1:
        assert np.isposinf(got["gap"]).all()
    again, inertia2 = _assign_all(it, C, prev, want_D=False)
    for k in ("label", "dist", "gap", "changed"):
        assert np.array_equal(again[k], got[k])
    assert inertia2 == inertia


def _chunk_edge(d, K, chunks):
    """the smallest n that the update sums in `chunks` chunks"""
    from scrubvae_amd import _lib
    f = _lib.lib().svae_kmeans_chunks
    n = 1
    while f(n, d, K) < chunks:
        n += 1
    return n


def _update_shapes():
    return SHAPES + [(_chunk_edge(5, 7, 2), 5, 7), (_chunk_edge(5, 7, 3), 5, 7), (_chunk_edge(20, 40, 3) + 2, 20, 40),
                     (700, 9, 300)]  # more than 256 clusters: two cluster groups per chunk


@functools.lru_cache(maxsize=None)
def _update_shapes_cached():
    return tuple(_update_shapes())


def _run_update(it, labels, C_old):
    it.update(_dev(labels, torch.int32))
    C_old_d, C_new_d = _dev(C_old), torch.empty(C_old.shape, **it.R.f64)
    changed, shift, n_empty = it.finish(C_old_d, C_new_d)
    return it.sums.cpu().numpy(), C_new_d.cpu().numpy(), changed, shift, n_empty


@pytest.mark.parametrize("i", range(16))
def test_update_and_finish(i):
    n, d, K = _update_shapes_cached()[i]
    if i == 12:
        assert n == 257  # 256-row units: just above one chunk
    if i == 13:
        assert n == 513  # just above two
    g, R, it, A, C_old = _case(n, d, K)
    labels = g.integers(0, K, n)
    hole = K - 2 if K >= 3 else None  # an empty cluster
    if hole is not None:
        labels[labels == hole] = K - 1
    sums, C_new, changed, shift, n_empty = _run_update(it, labels, C_old)
    ref, bound = KC.fsum_cluster_sums(A, labels, K)
    counts = np.bincount(labels, minlength=K)
    assert np.array_equal(sums[:, d], counts) and changed == -1
    assert (np.abs(sums[:, :d] - ref[:, :d]) <= bound[:, :d]).all()
    live = counts > 0
    assert n_empty == int((~live).sum())
    assert np.array_equal(C_new[~live], C_old[~live])
    c_ref = ref[live, :d] / counts[live, None]
    assert (np.abs(C_new[live] - c_ref) <= bound[live, :d] / counts[live, None] + 2 * U * np.abs(c_ref)).all()
    # the shift of the device's own centres: K d squares (the same roundings on the host), their sum within the bound of any order
    sq = ((C_new - C_old) ** 2).ravel()
    exact = math.fsum(sq)
    assert abs(shift - exact) <= (len(sq) - 1) * U * exact
    # twice the same bits
    sums2, C_new2, _, shift2, _ = _run_update(it, labels, C_old)
    assert np.array_equal(sums2, sums) and np.array_equal(C_new2, C_new) and shift2 == shift
    # renumbering the clusters permutes the sums bit for bit
    perm = g.permutation(K)
    sums3, C_new3, _, _, n_empty3 = _run_update(it, perm[labels], C_old[np.argsort(perm)])
    assert np.array_equal(sums3[perm], sums) and n_empty3 == n_empty
    assert np.array_equal(C_new3[perm][live], C_new[live])


def _tol(it, tol=1e-4):
    return tol * it.sum_of_squares() / (it.R.n * it.R.d)


def test_one_lloyd_step_at_a_time():
    from scrubvae_amd.eval import cluster as CL
    x = planted(2003, 16, 6, seed=16)
    K = 9
    R, it, A = _rows(x, K)
    tol_ = _tol(it)
    assert abs(tol_ - KC.tolerance(A, 1e-4)) <= 2003 * 16 * U * tol_
    seeds = R.kmeans_pp(CL.check_random_state(0))
    assert np.array_equal(seeds, KC.kmeans_pp(A, K, KC.check_random_state(0)))
    C, C_new = it.C
    C.copy_(_dev(A[seeds]))
    label, prev = it.label
    prev.fill_(-1)
    prev_ref = np.full(len(A), -1)
    gate = KC.centre_gate(A)
    stopped = False
    for _ in range(300):
        C_in = C.cpu().numpy()
        changed, shift, n_empty = it.step(C, C_new, label, prev)
        st = KC.lloyd_step(A, C_in)
        assert np.array_equal(label.cpu().numpy(), st["labels"]) and n_empty == st["n_empty"]
        assert np.array_equal(it.dist.cpu().numpy(), st["dist"])
        assert np.abs(C_new.cpu().numpy() - st["centers"]).max() <= gate
        assert changed == int((st["labels"] != prev_ref).sum())
        strict, strict_ref = changed == 0, np.array_equal(st["labels"], prev_ref)
        small, small_ref = shift <= tol_, st["shift"] <= tol_
        print(f"changed {changed} shift {shift!r} ref {st['shift']!r} tol {tol_!r}")
        assert strict == strict_ref and small == small_ref
        if strict or small:
            stopped = True
            break
        C, C_new = C_new, C
        label, prev = prev, label
        prev_ref = st["labels"]
    assert stopped


def _gap_margin(trace, gate, d):
    """what a move of every centre coordinate by `gate` can change in a row's top-two gap, at the most, over the iterations of a
    fit: 2 (2 sqrt(s d) gate + d gate^2) for the larger s of the two -- and the smallest gap seen"""
    effect = max(2.0 * (2.0 * math.sqrt(float((t["dist"] + t["gap"]).max()) * d) * gate + d * gate * gate) for t in trace)
    return effect, min(float(t["gap"].min()) for t in trace)


@functools.lru_cache(maxsize=None)
def _fit_data():
    x = planted(2003, 16, 6, seed=3)
    R, it, A = _rows(x, 9)
    return x, A, R.mean.copy()


@pytest.mark.parametrize("init,n_init,seed", [("k-means++", 1, 0), ("random", 3, 1), ("array", 1, 2)])
def test_whole_fit_equals_restatement(init, n_init, seed):
    from scrubvae_amd.eval import KMeans
    x, A, mean = _fit_data()
    K = 9
    if init == "array":
        init_dev = x[np.random.default_rng(seed).choice(len(x), K, replace=False)].astype(np.float64)
        init_ref = init_dev - mean[None, :]
    else:
        init_dev = init_ref = init
    trace = []
    ref = KC.fit(A, K, init=init_ref, n_init=n_init, random_state=seed, centred=True, trace=trace)
    effect, min_gap = _gap_margin(trace, KC.centre_gate(A), A.shape[1])
    print(f"min gap {min_gap!r} gate effect {effect!r} iterations {ref['n_iter']}")
    assert min_gap > effect
    m = KMeans(K, init=init_dev, n_init=n_init, random_state=seed).fit(x)
    assert m.labels_.dtype == np.int32 and m.cluster_centers_.dtype == np.float64 and m.n_features_in_ == 16
    assert np.array_equal(m.labels_, ref["labels"]) and m.n_iter_ == ref["n_iter"]
    assert np.abs(m.cluster_centers_ - (ref["centers"] + mean[None, :])).max() <= KC.centre_gate(x.astype(np.float64))
    assert abs(m.inertia_ - ref["inertia"]) <= KC.inertia_gate(len(x)) * ref["inertia"]


def test_relocation_path_equals_restatement():
    from scrubvae_amd.eval import KMeans
    x, A, mean = _fit_data()
    K = 7
    init = x[np.random.default_rng(5).choice(len(x), K, replace=False)].astype(np.float64)
    init[K - 1] += 1000.0
    init[K - 2] += 2000.0
    trace = []
    ref = KC.fit(A, K, init=init - mean[None, :], centred=True, trace=trace)
    assert trace[0]["n_empty"] == 2
    effect, min_gap = _gap_margin(trace, KC.centre_gate(A), A.shape[1])
    assert min_gap > effect
    m = KMeans(K, init=init).fit(x)
    assert np.array_equal(m.labels_, ref["labels"]) and m.n_iter_ == ref["n_iter"] and len(np.unique(m.labels_)) == K
    assert np.abs(m.cluster_centers_ - (ref["centers"] + mean[None, :])).max() <= KC.centre_gate(x.astype(np.float64))


def test_predict_transform_score_and_device_input():
    from scrubvae_amd.eval import KMeans
    x, A, mean = _fit_data()
    m = KMeans(9, random_state=0).fit(x)
    assert np.array_equal(m.predict(x), m.labels_)
    s = KC.sqdist(A, m.cluster_centers_ - mean[None, :])
    want = np.sqrt(s)
    t = m.transform(x)
    assert t.shape == (len(x), 9) and (np.abs(t - want) <= np.spacing(want)).all()
    assert abs(m.score(x) + m.inertia_) <= KC.inertia_gate(len(x)) * m.inertia_
    assert np.array_equal(m.fit_predict(x), m.labels_)
    md = KMeans(9, random_state=0).fit(torch.from_numpy(x).cuda())
    assert np.array_equal(md.labels_, m.labels_) and np.array_equal(md.cluster_centers_, m.cluster_centers_)
    assert md.inertia_ == m.inertia_ and md.n_iter_ == m.n_iter_
    assert np.array_equal(KMeans(9, random_state=0).fit_transform(x), t)


def test_fit_at_the_cluster_limit():
    from scrubvae_amd.eval import KMeans
    from scrubvae_amd.eval.cluster import ConvergenceWarning
    x = np.random.default_rng(4).normal(size=(2048, 4)).astype(np.float32)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = KMeans(1024, random_state=0).fit(x)
    distinct = len(np.unique(m.labels_))
    assert distinct == 1024 or any(issubclass(i.category, ConvergenceWarning) for i in w)
    assert m.cluster_centers_.shape == (1024, 4) and m.labels_.min() >= 0 and m.labels_.max() < 1024 and np.isfinite(m.inertia_)
