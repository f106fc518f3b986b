"""TSNE / tsne / tsne_affinities (csrc/tsne.hip) on the device, stage by stage against the numpy restatement and the long-double
truth of tests/tsne_checks.py, whose gates are derived there.

The search's beta is dyadic, so it is held to equal bytes (the inputs have no step near a comparison: asserted); gains, update and
the new Y are elementwise given the row's sums in stored order, so they are held to equal bytes too.  Every floating-point sum
whose order the device chooses (the repulsion, Z, the KL value) is held to its gate, and to equal bytes between two calls.  The
whole fit, a chaotic optimisation, is held to properties and to the spread of sklearn's own Barnes-Hut fits over five seeds."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import silhouette_checks as SC
from tests import tsne_checks as TC

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a)).to(dtype).cuda()


def device_search(d2, perplexity):
    from scrubvae_amd.eval import embed
    P, beta = embed._search_device(dev(d2), perplexity)
    return P.cpu().numpy(), beta.cpu().numpy()


@pytest.mark.parametrize("n,d,k,seed", TC.SEARCH_GPU)
def test_search_equals_the_restatement(n, d, k, seed):
    d2, s = TC.search_case(n, d, k, seed)
    perplexity = TC.search_perplexity(k)
    assert s.near >= 1e-9 and s.tiny >= 1e-12, "a step of some row sits on a comparison: change the seed, not the gate"
    P, beta = device_search(d2, perplexity)
    assert P.shape == (n, k) and bits(beta) == bits(s.beta)
    truth = TC.search_truth(d2, s.used)
    e = TC.err(P, truth)
    H = TC.entropy(P)
    worst = float(np.abs(H - np.log(TC.LD(perplexity))).max())
    print(f"search n={n} k={k}: worst |P - truth| / gate {float((e / TC.p_gate(truth)).max()):.3f}, max |H - log(perplexity)| {worst:.3e}")
    assert (e <= TC.p_gate(truth)).all()
    assert worst <= 1e-5 + 1e-9
    again = device_search(d2, perplexity)
    assert bits(again[0]) == bits(P) and bits(again[1]) == bits(beta)


def test_search_on_identical_rows():
    n, k = 70, 6
    P, beta = device_search(np.zeros((n, k)), 2.0)
    assert np.isfinite(P).all() and np.array_equal(P, np.full((n, k), 1.0 / k))
    assert np.array_equal(beta, np.full(n, 2.0 ** TC.STEPS))   # doubled at every one of the 100 steps
    want = TC.search(np.zeros((n, k)), 2.0)
    assert bits(P) == bits(want.P) and bits(beta) == bits(want.beta)


def device_repulsion(Y, chunks):
    from scrubvae_amd import _lib, ops
    lib = _lib.lib()
    n = len(Y)
    Yd = dev(Y)
    words = lib.svae_tsne_repulsion_work(n, chunks)
    assert words > 0
    work = torch.full((words,), float("nan"), dtype=torch.float64, device="cuda")
    R = torch.full((n, 2), float("nan"), dtype=torch.float64, device="cuda")
    rowq = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    Z = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.svae_tsne_repulsion(Yd.data_ptr(), n, chunks, work.data_ptr(), R.data_ptr(), rowq.data_ptr(), Z.data_ptr(), ops._stream()),
               "tsne_repulsion")
    assert torch.equal(Yd.cpu(), torch.from_numpy(np.array(Y)))
    return R.cpu().numpy(), rowq.cpu().numpy(), float(Z.cpu()[0]), words // (3 * (-(-n // 256) * 256))


@functools.lru_cache(maxsize=None)
def repulsion_case(n, scale):
    Y = scale * np.random.default_rng(n).standard_normal((n, 2))
    Y.setflags(write=False)
    return Y, TC.repulsion_gate(Y)


def check_repulsion(Y, g, chunks):
    R, rowq, Z, made = device_repulsion(Y, chunks)
    eR, eq, eZ = TC.err(R, g.R), TC.err(rowq, g.rowq), float(TC.err(Z, g.Z))
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = max(float(np.nanmax(np.where(g.tol_R > 0, eR / g.tol_R, 0))), float((eq / g.tol_rowq).max()), eZ / g.tol_Z)
    assert (eR <= g.tol_R).all() and (eq <= g.tol_rowq).all() and eZ <= g.tol_Z
    again = device_repulsion(Y, chunks)
    assert bits(again[0]) == bits(R) and bits(again[1]) == bits(rowq) and again[2] == Z
    return worst, made


@pytest.mark.parametrize("scale", [1e-4, 30.0])
@pytest.mark.parametrize("n", TC.REPULSION_N)
def test_repulsion_inside_the_gate(n, scale):
    Y, g = repulsion_case(n, scale)
    tiles = -(-n // 64)
    seen = {}
    for chunks in (1, 3, 8, 0):
        worst, made = check_repulsion(Y, g, chunks)
        seen[chunks] = made
        assert made == -(-tiles // -(-tiles // min(tiles, chunks if chunks else 8)))   # whole 64-column tiles per chunk
        print(f"repulsion n={n} |Y|~{scale} chunks={chunks} (made {made}): worst error / gate {worst:.4f}")
    if n == 1037:
        assert seen == {1: 1, 3: 3, 8: 6, 0: 6}
    if n == 2:
        assert seen == {1: 1, 3: 1, 8: 1, 0: 1}


def test_repulsion_of_coincident_points():
    R, rowq, Z, _ = device_repulsion(np.array([[0.25, -3.0], [0.25, -3.0]]), 0)
    assert np.array_equal(R, np.zeros((2, 2))) and np.array_equal(rowq, [1.0, 1.0]) and Z == 2.0   # q = 1, no force
    Y = np.array(repulsion_case(65, 30.0)[0])
    Y[64] = Y[0]                 # in two different 64-column tiles
    g = TC.repulsion_gate(Y)
    for chunks in (1, 2):
        check_repulsion(Y, g, chunks)
    R, rowq, _, _ = device_repulsion(Y, 1)
    # the two rows see the same others and each other at q = 1 with no force, but row 0 meets row 64 last and row 64 meets row 0
    # first: the same sums in two orders
    assert (np.abs(R[0] - R[64]) <= 2 * g.tol_R[0]).all() and abs(rowq[0] - rowq[64]) <= 2 * g.tol_rowq[0] and rowq[0] > 1.0


def random_csr(n, seed):
    """rows of 0 to 40 entries in ascending columns, none on the diagonal, row 5 empty, values like joint probabilities"""
    g = np.random.default_rng(seed)
    rowptr, col = [0], []
    for i in range(n):
        m = 0 if i == 5 else int(g.integers(1, min(41, n - 1)))
        c = np.sort(g.choice(np.delete(np.arange(n), i), size=m, replace=False))
        col.extend(c)
        rowptr.append(len(col))
    val = g.random(len(col)) / len(col) * 2
    return np.array(rowptr, dtype=np.int32), np.array(col, dtype=np.int32), val


def device_step(rowptr, col, val, exag, Y, R, Z, update, gains, momentum, lr, look=True, move=True):
    from scrubvae_amd import _lib, ops
    n = len(Y)
    t = dict(rowptr=torch.from_numpy(rowptr).cuda(), col=torch.from_numpy(col).cuda(), val=dev(val), Y=dev(Y), R=dev(R), Z=dev([Z]),
             update=dev(update), gains=dev(gains), kl=torch.full((n,), float("nan"), dtype=torch.float64, device="cuda"),
             gsq=torch.full((n,), float("nan"), dtype=torch.float64, device="cuda"))
    _lib.check(_lib.lib().svae_tsne_step(t["rowptr"].data_ptr(), t["col"].data_ptr(), t["val"].data_ptr(), exag, t["Y"].data_ptr(),
                                         t["R"].data_ptr(), t["Z"].data_ptr(), t["update"].data_ptr() if move else None,
                                         t["gains"].data_ptr() if move else None, momentum, lr, n, t["kl"].data_ptr() if look else None,
                                         t["gsq"].data_ptr() if look else None, ops._stream()), "tsne_step")
    return {k: v.cpu().numpy() for k, v in t.items()}


@pytest.mark.parametrize("n,exag,scale", [(300, 12.0, 1e-4), (300, 1.0, 20.0), (65, 1.0, 1.0)])
def test_step_equals_the_restatement(n, exag, scale):
    g = np.random.default_rng(n + int(exag))
    rowptr, col, val = random_csr(n, n)
    assert rowptr[6] == rowptr[5] and len(set(np.diff(rowptr))) > 5
    Y = scale * g.standard_normal((n, 2))
    R, _, Z, _ = TC.repulsion(Y)
    R = R * (1 + 0.1 * g.standard_normal((n, 2)))            # any numbers: the kernel takes them as given
    update = scale * 0.1 * g.standard_normal((n, 2))
    gains = g.choice([0.01, 0.0105, 0.8, 1.0, 1.2, 3.4], size=(n, 2))
    momentum, lr = 0.8, 200.0 * scale * scale * 1e4          # large enough to move every row by about its distance to a neighbour
    want_Y, want_update, want_gains, want_kl, want_gsq = TC.step(rowptr, col, val, exag, Y, R, Z, update, gains, momentum, lr)
    assert np.abs(want_Y - Y).max() > 1e-3 * scale           # a row that read a moved neighbour would not reproduce these bytes
    got = device_step(rowptr, col, val, exag, Y, R, Z, update, gains, momentum, lr)
    assert bits(got["gains"]) == bits(want_gains) and (want_gains >= 0.01).all() and (want_gains == 0.01).any()
    assert bits(got["update"]) == bits(want_update)
    assert bits(got["Y"]) == bits(want_Y)
    assert bits(got["gsq"]) == bits(want_gsq)
    _, truth_kl, _, klw, _ = TC.attraction(rowptr, col, val, exag, Y, TC.LD)
    tol = (TC.U * klw).astype(np.float64)
    e = TC.err(got["kl"], truth_kl)
    print(f"step n={n} exag={exag}: klpart worst error / gate {float((e[tol > 0] / tol[tol > 0]).max()):.4f}")
    assert (e <= tol).all() and got["kl"][5] == 0.0 and (TC.err(want_kl, truth_kl) <= tol).all()
    # without a look: the same step, klpart and gradsq untouched
    blind = device_step(rowptr, col, val, exag, Y, R, Z, update, gains, momentum, lr, look=False)
    assert bits(blind["Y"]) == bits(want_Y) and bits(blind["gains"]) == bits(want_gains) and np.isnan(blind["kl"]).all() and np.isnan(blind["gsq"]).all()
    # evaluation only: nothing moves, klpart as before, gradsq of the plain gradient
    A, _, _, _, _ = TC.attraction(rowptr, col, val, exag, Y)
    grad = TC.gradient(A, R, Z, exag)
    ev = device_step(rowptr, col, val, exag, Y, R, Z, update, gains, momentum, lr, move=False)
    assert bits(ev["Y"]) == bits(Y) and bits(ev["update"]) == bits(update) and bits(ev["gains"]) == bits(gains)
    assert bits(ev["kl"]) == bits(got["kl"]) and bits(ev["gsq"]) == bits(grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1])


def test_sums_are_fixed_order():
    from scrubvae_amd.eval import embed
    g = np.random.default_rng(0)
    for n in (1, 255, 256, 257, 5000):
        a, b = g.standard_normal(n) * 10.0 ** g.integers(-3, 4, n), g.random(n)
        out = embed._sums_device(dev(a), dev(b)).cpu().numpy()
        for got, v in zip(out, (a, b)):
            assert abs(got - float(v.astype(TC.LD).sum())) <= (n // 256 + 10) * TC.U * np.abs(v).sum()
        assert bits(embed._sums_device(dev(a), dev(b)).cpu().numpy()) == bits(out)
        assert embed._sums_device(dev(a)).cpu().numpy()[0] == out[0]


@pytest.mark.parametrize("n,d,perplexity", [(301, 3, 30.0), (120, 5, 4.5), (40, 2, 30.0)])
def test_affinities_equal_the_restatement(n, d, perplexity):
    pytest.importorskip("scipy.sparse")
    from scrubvae_amd.eval import tsne_affinities
    x, _ = SC.blobs(n, d, 4, seed=n)
    want, s, S = TC.affinities(x, perplexity)
    assert s.near >= 1e-9 and s.tiny >= 1e-12
    P, beta = tsne_affinities(x, perplexity)
    k = min(n - 1, int(math.floor(3 * perplexity)))
    assert P.shape == (n, n) and P.format == "csr" and P.dtype == np.float64 and beta.dtype == np.float64
    assert np.array_equal(P.indptr, want.indptr) and np.array_equal(P.indices, want.indices)     # the structure, exactly
    assert (np.diff(P.indices)[np.diff(np.repeat(np.arange(n), np.diff(P.indptr))) == 0] > 0).all()   # ascending within a row
    assert bits(beta) == bits(s.beta)
    # both sides: entries of at most two P, each within (k + 12) U, one addition, a sum of nnz terms, one division
    tol = 2 * (2 * (k + 13) + P.nnz) * TC.U * want.data
    e = np.abs(P.data - want.data)
    print(f"affinities n={n} k={k} nnz={P.nnz}: worst error / gate {float((e / tol).max()):.4f}, |sum - 1| {abs(P.data.astype(TC.LD).sum() - 1):.2e}")
    assert (e <= tol).all() and abs(float(P.data.astype(TC.LD).sum() - 1)) <= (P.nnz + 2) * TC.U
    assert abs(P - P.T).max() == 0.0
    again, beta2 = tsne_affinities(torch.from_numpy(x.astype(np.float32)).cuda(), perplexity)    # float32-representable rows
    assert bits(again.data) == bits(P.data) and np.array_equal(again.indices, P.indices) and bits(beta2) == bits(beta)


@functools.lru_cache(maxsize=None)
def sklearn_trust_range(n, d, blobs):
    man = pytest.importorskip("sklearn.manifold")
    x, _ = TC.fit_case(n, d, blobs)
    vals = []
    for seed in range(5):
        emb = man.TSNE(method="barnes_hut", init="random", max_iter=500, random_state=seed).fit_transform(x)
        vals.append(float(man.trustworthiness(x, emb, n_neighbors=5)))
    return vals


@pytest.mark.parametrize("n,d,blobs", TC.FITS)
def test_whole_fit(n, d, blobs):
    man = pytest.importorskip("sklearn.manifold")
    from scrubvae_amd.eval import TSNE, embed, tsne, tsne_affinities
    x, _ = TC.fit_case(n, d, blobs)
    before = dict(embed._TSNE_CALLS)
    est = TSNE(max_iter=500, random_state=1)
    Y = est.fit_transform(x)
    made = {k: embed._TSNE_CALLS[k] - before[k] for k in before}
    checks = list(embed._TSNE_LAST["kl_checks"])
    assert Y is est.embedding_ and Y.shape == (n, 2) and Y.dtype == np.float64 and np.isfinite(Y).all()
    # the schedule: all 500 iterations, a look every 50, one read of three numbers per look and one for the final value
    assert est.n_iter_ == 499 and [i for i, _ in checks] == list(range(49, 500, 50))
    assert made["repulsion"] == 501 and made["step"] == 501 and made["host_reads"] == 11 and made["search"] == 1
    assert est.learning_rate_ == max(n / 12.0 / 4.0, 50.0)
    first_after = dict(checks)[299]
    print(f"fit n={n}: KL at the looks {[round(v, 4) for _, v in checks]}, final {est.kl_divergence_:.6f}")
    assert est.kl_divergence_ < first_after
    # the reported KL is the KL of the reported embedding
    P, _ = tsne_affinities(x, 30.0)
    g = TC.objective_gate(P, Y, 1.0)
    kl, _ = TC.objective(P, Y, 1.0)
    e = float(TC.err(est.kl_divergence_, g.kl))
    print(f"  kl_divergence_ {est.kl_divergence_:.12f}, |device - truth| {e:.3e}, |restated - truth| {float(TC.err(kl, g.kl)):.3e}, gate {g.tol_kl:.3e}")
    assert e <= g.tol_kl and float(TC.err(kl, g.kl)) <= g.tol_kl
    # two fits give equal bytes, whatever the input's kind
    again = TSNE(max_iter=500, random_state=1).fit(torch.from_numpy(x.astype(np.float32)).cuda())
    assert bits(again.embedding_) == bits(Y) and again.kl_divergence_ == est.kl_divergence_ and again.n_iter_ == 499
    # as good as sklearn's own fits, within their own seed-to-seed spread
    ref = sklearn_trust_range(n, d, blobs)
    t = float(man.trustworthiness(x, Y, n_neighbors=5))
    gate = min(ref) - (max(ref) - min(ref))
    print(f"  trustworthiness {t:.5f}; sklearn Barnes-Hut over seeds 0..4 {[round(v, 5) for v in ref]}; gate {gate:.5f}")
    assert t >= gate
    if n == 400:
        assert bits(tsne(x, max_iter=500)) == bits(Y)


def test_early_stop_and_given_init():
    from scrubvae_amd.eval import TSNE
    x, _ = TC.fit_case(400, 8, 5)
    Y0 = 1e-4 * np.random.RandomState(0).standard_normal((400, 2))
    est = TSNE(max_iter=1000, min_grad_norm=1e10, init=Y0, perplexity=10).fit(x)
    assert est.n_iter_ == 99                       # each phase stops at its first look (sklearn does: test_tsne_cpu.py)
    ran = TSNE(max_iter=250, init="random", random_state=0, perplexity=10, min_grad_norm=1e10).fit(x)
    assert bits(ran.embedding_) == bits(est.embedding_) and ran.n_iter_ == 99
    assert TSNE(max_iter=250, init=Y0, perplexity=10).fit(x).n_iter_ == 250     # sklearn's value when nothing is left for the second phase
