"""t-SNE without a GPU: the restatement of tests/tsne_checks.py pinned stage by stage -- the perplexity search to sklearn's
_binary_search_perplexity, the exact gradient and KL value to their long-double evaluation (and sklearn's _kl_divergence to the
same gate), the optimiser's schedule to sklearn's TSNE(method="exact") -- then the package's argument errors raised before any
device work, its PCA sign rule, its schedule and the C-ABI exports."""
import math

import numpy as np
import pytest
import torch

from tests import silhouette_checks as SC
from tests import tsne_checks as TC

needs_ld = pytest.mark.skipif(not TC.HAVE_LD, reason="no 80-bit long double on this platform")


@pytest.mark.parametrize("n,d,k,seed", TC.SEARCH_CPU)
def test_restated_search_against_sklearn(n, d, k, seed):
    utils = pytest.importorskip("sklearn.manifold._utils")
    d2, s = TC.search_case(n, d, k, seed)
    perplexity = TC.search_perplexity(k)
    sk = utils._binary_search_perplexity(d2.astype(np.float32), perplexity, 0)
    assert sk.shape == s.P.shape == (n, k) and s.P.dtype == np.float64
    top = s.P.max(1)
    multiple = (np.abs(s.P - sk.astype(np.float64)).max(1) / (2.0 ** -23 * top)).max()
    print(f"search n={n} d={d} k={k}: max |P - sklearn| = {multiple:.3f} x 2^-23 of the row's largest P (gate 4); steps up to "
          f"{s.steps.max()}; nearest | |diff| - 1e-5 | {s.near:.3e}, smallest |diff| {s.tiny:.3e}")
    assert multiple <= 4.0
    assert s.near >= 1e-9 and s.tiny >= 1e-12, "a step of some row sits on a comparison: change the seed, not the gate"
    if TC.HAVE_LD:
        H = TC.entropy(s.P)
        worst = float(np.abs(H - np.log(TC.LD(perplexity))).max())
        print(f"  entropy: max |H - log(perplexity)| = {worst:.3e}")
        assert worst <= 1e-5 + 1e-9
        truth = TC.search_truth(d2, s.used)
        assert (TC.err(s.P, truth) <= TC.p_gate(truth)).all()
    assert (s.steps < TC.STEPS).all() and np.array_equal(s.beta, s.used)   # every row converged: beta is the beta of P


def test_search_on_identical_rows():
    s = TC.search(np.zeros((5, 6)), 2.0)
    assert np.array_equal(s.P, np.full((5, 6), 1.0 / 6.0)) and np.array_equal(s.beta, np.full(5, 2.0 ** 100))
    assert np.array_equal(s.used, np.full(5, 2.0 ** 99)) and (s.steps == 100).all()


def dense_case(n, d, blobs, scale, seed):
    x, _ = SC.blobs(n, d, blobs, seed=seed)
    P, _, _ = TC.affinities(x, min(30.0, (n - 1) / 3.0))
    Y = scale * np.random.default_rng(seed).standard_normal((n, 2))
    return P, Y


@needs_ld
@pytest.mark.parametrize("n,scale,exag", [(150, 1e-4, 12.0), (150, 20.0, 1.0), (300, 3.0, 1.0)])
def test_restated_gradient_and_kl_against_long_double(n, scale, exag):
    pytest.importorskip("scipy.sparse")
    P, Y = dense_case(n, 5, 4, scale, n)
    kl, grad = TC.objective(P, Y, exag)
    g = TC.objective_gate(P, Y, exag)
    e_kl, e_grad = float(TC.err(kl, g.kl)), TC.err(grad, g.grad)
    print(f"n={n} |Y|~{scale} exag={exag}: KL {float(g.kl):.6f}, |restated - truth| {e_kl:.3e} (gate {g.tol_kl:.3e}); gradient: worst "
          f"error / gate {float((e_grad / g.tol_grad).max()):.3f}")
    assert e_kl <= g.tol_kl and (e_grad <= g.tol_grad).all()
    # the gate is a gate: a gradient with one neighbour's attraction left out of one row is far outside it
    rowptr, col, val = TC.csr_rows(P)
    val = val.copy()
    val[rowptr[7]] = 0.0
    A, _, _, _, _ = TC.attraction(rowptr, col, val, exag, Y)
    R, _, Z, _ = TC.repulsion(Y)
    assert (TC.err(TC.gradient(A, R, Z, exag), g.grad) > g.tol_grad).any()


@needs_ld
@pytest.mark.parametrize("n,scale", [(150, 1e-4), (150, 20.0), (300, 3.0)])
def test_sklearn_kl_divergence_inside_the_same_gate(n, scale):
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    P, Y = dense_case(n, 5, 4, scale, n)
    dense = P.toarray()
    assert np.array_equal(dense, dense.T) and (dense[dense > 0] > np.finfo(np.float64).eps).all()   # sklearn clips P and Q at eps
    terms = n * (n - 1) // 2
    g = TC.objective_gate(P, Y, 1.0, adds=terms)
    kl, grad = tsne._kl_divergence(Y.ravel(), squareform(dense, checks=False), 1.0, n, 2)
    e_kl = float(TC.err(kl, g.kl))
    print(f"n={n} |Y|~{scale}: sklearn's KL {kl:.6f}, |sklearn - truth| {e_kl:.3e}, gate for {terms} terms in an unknown order {g.tol_kl:.3e}")
    assert e_kl <= g.tol_kl
    mine_kl, mine_grad = TC.objective(P, Y, 1.0)
    assert np.abs(grad.reshape(n, 2) - mine_grad).max() <= 1e-9 * np.abs(mine_grad).max()   # the same gradient, not held to the gate


def record_sklearn(monkeypatch):
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    calls = []
    real = tsne._gradient_descent

    def spy(objective, p0, it, max_iter, **kw):
        out = real(objective, p0, it, max_iter, **kw)
        calls.append(dict(it=it, max_iter=max_iter, momentum=kw["momentum"], learning_rate=kw["learning_rate"],
                          n_iter_without_progress=kw["n_iter_without_progress"], P_sum=float(kw["args"][0].sum()) * 2, end=out[2]))
        return out

    monkeypatch.setattr(tsne, "_gradient_descent", spy)
    return tsne, calls


@pytest.mark.parametrize("max_iter,min_grad_norm,ee", [(300, 1e-7, 12.0), (1000, 1e10, 12.0), (250, 1e-7, 4.0)])
def test_restated_schedule_against_sklearn(monkeypatch, max_iter, min_grad_norm, ee):
    from scrubvae_amd.eval import embed
    tsne, calls = record_sklearn(monkeypatch)
    n = 60
    x, _ = SC.blobs(n, 4, 3, seed=5)
    Y0 = 1e-4 * np.random.RandomState(0).standard_normal((n, 2))
    sk = tsne.TSNE(method="exact", init=Y0.copy(), perplexity=10.0, max_iter=max_iter, min_grad_norm=min_grad_norm, early_exaggeration=ee)
    sk.fit(x)
    P, _, _ = TC.affinities(x, 10.0)
    _, n_iter, spans, checks = TC.optimise(P, Y0, max_iter=max_iter, min_grad_norm=min_grad_norm, early_exaggeration=ee)
    want = TC.schedule(n, max_iter=max_iter, early_exaggeration=ee)
    mine = embed._tsne_schedule(max_iter, 300, ee)
    print(f"max_iter={max_iter} min_grad_norm={min_grad_norm}: sklearn's calls {calls}; restated spans {spans}, n_iter_ {n_iter} / {sk.n_iter_}")
    assert len(calls) == len(spans) == 2 and n_iter == sk.n_iter_
    assert sk.learning_rate_ == want[0]["learning_rate"] == embed._auto_learning_rate(n, ee) == max(n / ee / 4.0, 50.0)
    for c, w, m, span in zip(calls, want, mine, spans):
        assert (c["it"], c["end"]) == span                       # where exaggeration ends and where the run ends
        assert c["max_iter"] == w["max_iter"] == m["max_iter"] and c["momentum"] == w["momentum"] == m["momentum"]
        assert c["n_iter_without_progress"] == w["n_iter_without_progress"] == m["window"]
        assert c["learning_rate"] == w["learning_rate"]
        assert abs(c["P_sum"] - w["exag"]) <= 1e-6 * w["exag"] and w["exag"] == m["exag"]   # the factor on P in this phase
    assert mine[0]["it"] == 0 and mine[1]["it"] is None and embed._EXPLORATION_ITER == 250 and embed._N_ITER_CHECK == 50
    if min_grad_norm > 1:
        assert spans == [(0, 49), (50, 99)] and n_iter == 99     # each phase stops at its first check
    else:
        assert n_iter == (max_iter - 1 if max_iter > 250 else 250) and [i for i, _ in checks] == list(range(49, max_iter, 50))


def test_pca_sign_rule():
    dec = pytest.importorskip("sklearn.decomposition")
    from scrubvae_amd.eval import embed
    for n, d, seed in ((200, 6, 0), (150, 2, 3), (90, 16, 7)):
        x, _ = SC.blobs(n, d, 4, seed=seed)
        got = embed._pca_init(torch.from_numpy(x.copy())).numpy()
        want = TC.pca_init(x)
        sk = dec.PCA(n_components=2, svd_solver="full").fit_transform(x)
        sk = sk / np.std(sk[:, 0]) * 1e-4
        assert got.shape == (n, 2) and got.dtype == np.float64
        assert np.abs(got - want).max() <= 1e-9 * 1e-4 and np.abs(got - sk).max() <= 1e-9 * 1e-4   # the same signs as sklearn's svd_flip
        assert abs(np.std(got[:, 0]) - 1e-4) <= 1e-15
    # the rule itself: a component whose largest-magnitude loading is negative in the decomposition comes out flipped
    x = np.random.default_rng(1).standard_normal((300, 3)) * np.array([5.0, 1.0, 0.1])
    Y = embed._pca_init(torch.from_numpy(x)).numpy()
    xc = x - x.mean(0)
    assert np.corrcoef(Y[:, 0], xc[:, 0])[0, 1] > 0.99 and np.corrcoef(Y[:, 1], xc[:, 1])[0, 1] > 0.99
    Yn = embed._pca_init(torch.from_numpy(-x)).numpy()
    assert np.abs(Yn + Y).max() <= 1e-12   # the loadings are the same, the scores change sign


XS, _ = SC.blobs(40, 3, 3, 0)
BAD = np.arange(120).reshape(40, 3) == 7


@pytest.mark.parametrize("z,kw", [
    (np.where(BAD, np.nan, XS), {}),
    (np.where(BAD, np.inf, XS), {}),
    (torch.from_numpy(np.where(BAD, np.nan, XS)), {}),
    (XS[0], {}),                                              # 1-D
    (XS[:1], dict(perplexity=0.5)),                           # one row
    (XS, dict(n_components=3)),
    (XS, dict(n_components=1)),
    (XS, dict(perplexity=0.0)),
    (XS, dict(perplexity=-2.0)),
    (XS, dict(perplexity=0.3)),                               # floor(3 perplexity) = 0
    (XS, dict(perplexity=30.5)),                              # 91 neighbours
    (XS, dict(perplexity=40.0)),                              # perplexity >= n
    (XS[:20], dict(perplexity=20.0)),                         # perplexity >= n below the cap
    (XS, dict(perplexity=float("nan"))),
    (XS, dict(max_iter=249)),
    (XS, dict(max_iter=300.0)),
    (XS, dict(early_exaggeration=0.5)),
    (XS, dict(init="spectral")),
    (XS, dict(init=np.zeros((39, 2)))),
    (XS, dict(init=np.zeros((40, 3)))),
    (XS, dict(init=np.where(np.arange(80).reshape(40, 2) == 3, np.nan, 0.0))),
    (XS, dict(learning_rate="fast")),
    (XS, dict(learning_rate=0.0)),
    (XS[:, :1], dict(init="pca")),                            # one feature has no second component
])
def test_argument_errors_before_device_work(z, kw):
    """this machine has no device: a ValueError, not the "no device is available" RuntimeError, shows the order"""
    import scrubvae_amd.eval as E
    kw = dict(dict(perplexity=5.0), **kw)
    with pytest.raises(ValueError):
        E.TSNE(**kw).fit(z)
    with pytest.raises(ValueError):
        E.tsne(z, **kw)
    if set(kw) == {"perplexity"}:
        with pytest.raises(ValueError):
            E.tsne_affinities(z, kw["perplexity"])


def test_the_cap_is_named_and_the_default_is_allowed():
    import scrubvae_amd.eval as E
    from scrubvae_amd.eval import embed
    big = np.zeros((200, 2))
    with pytest.raises(ValueError, match="KNN_MAX_K = 90"):
        E.tsne_affinities(big, 31.0)
    assert embed._tsne_neighbors(200, 30.0) == 90 == embed.KNN_MAX_K
    assert embed._tsne_neighbors(200, 30.3) == 90 and embed._tsne_neighbors(20, 10.0) == 19 and embed._tsne_neighbors(200, 5) == 15
    t = E.TSNE()
    assert (t.n_components, t.perplexity, t.early_exaggeration, t.learning_rate, t.max_iter, t.n_iter_without_progress, t.min_grad_norm,
            t.init, t.random_state) == (2, 30.0, 12.0, "auto", 1000, 300, 1e-7, "pca", None)
    x, k, init, lr = E.TSNE(perplexity=5.0, init="random", random_state=3)._check(XS.astype(np.float32))
    assert x.dtype == np.float64 and k == 15 and lr == 50.0
    assert np.array_equal(init, 1e-4 * np.random.RandomState(3).standard_normal((40, 2)))
    given = np.arange(80.0).reshape(40, 2)
    assert np.array_equal(E.TSNE(perplexity=5.0, init=torch.from_numpy(given))._check(XS)[2], given)
    assert E.TSNE(perplexity=5.0, learning_rate=120)._check(XS)[3] == 120.0


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    lib = _lib.lib()
    work = lib.svae_tsne_repulsion_work
    assert work(1, 0) == 0 and work(0, 1) == 0 and work(-3, 0) == 0 and work(2 ** 26 + 1, 0) == 0   # n out of range
    assert work(100, -1) == 0 and work(100, _lib.TSNE_MAX_CHUNKS + 1) == 0
    # chunks x 3 sums x rows padded to 256; a forced count is cut to the number of 64-column tiles
    assert work(2, 0) == 1 * 3 * 256 and work(2, 8) == 1 * 3 * 256
    assert work(301, 0) == 5 * 3 * 512 and work(301, 3) == 3 * 3 * 512 and work(301, 1) == 3 * 512
    assert work(1037, 0) == 6 * 3 * 1280 and work(1037, 8) == 6 * 3 * 1280      # 17 tiles: 8 chunks asked, 6 of 3 tiles made
    assert work(20000, 0) == 7 * 3 * 20224                                      # 79 row blocks: 7 chunks reach 512 blocks
    assert work(200000, 0) == 1 * 3 * 200192                                    # 782 row blocks: one chunk
    assert work(2 ** 26, 0) == 3 * 2 ** 26
    fake = 4096
    assert lib.svae_tsne_search(fake, 0, 10, 3.0, fake, fake, None) == _lib.ERR_ARG
    assert lib.svae_tsne_search(fake, _lib.KNN_MAX_K + 1, 1000, 3.0, fake, fake, None) == _lib.ERR_ARG
    assert lib.svae_tsne_search(fake, 3, 10, 0.0, fake, fake, None) == _lib.ERR_ARG
    assert lib.svae_tsne_search(None, 3, 10, 3.0, fake, fake, None) == _lib.ERR_ARG
    assert lib.svae_tsne_repulsion(fake, 1, 0, fake, fake, fake, fake, None) == _lib.ERR_ARG
    assert lib.svae_tsne_repulsion(fake, 10, 9, fake, fake, fake, fake, None) == _lib.ERR_ARG
    assert lib.svae_tsne_repulsion(fake, 10, 0, None, fake, fake, fake, None) == _lib.ERR_ARG and "null" in _lib.last_error()
    assert lib.svae_tsne_step(fake, fake, fake, 1.0, fake, fake, fake, fake, None, 0.5, 1.0, 10, fake, fake, None) == _lib.ERR_ARG
    assert lib.svae_tsne_step(fake, fake, fake, 1.0, fake, fake, fake, None, None, 0.5, 1.0, 10, None, None, None) == _lib.ERR_ARG
    assert lib.svae_tsne_step(fake, fake, fake, 1.0, fake, fake, fake, fake, fake, 0.5, 1.0, 1, fake, fake, None) == _lib.ERR_ARG
    assert lib.svae_tsne_sums(fake, None, 0, fake, None) == _lib.ERR_ARG
    import scrubvae_amd.eval as E
    from scrubvae_amd.eval import embed
    for name in ("TSNE", "tsne", "tsne_affinities"):
        assert callable(getattr(E, name))
    assert embed._TSNE_CALLS.keys() >= {"search", "repulsion", "step", "host_reads"} and embed._TSNE_LAST.keys() >= {"work", "chunks"}


def test_constants_equal_the_headers():
    from scrubvae_amd import _lib
    assert _lib.TSNE_SEARCH_STEPS == TC.STEPS
    assert _lib.KNN_MAX_K == 3 * 30
    assert math.floor(3 * 30.0) == _lib.KNN_MAX_K
