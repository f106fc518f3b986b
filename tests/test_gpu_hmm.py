"""GPU checks of the Gaussian HMM (csrc/hmm.hip, scrubvae_amd/eval/hmm.py) against the restatements and gates of
tests/hmm_checks.py: the pass against long double, structural zeros, separability, bit reproducibility, Viterbi, one EM iteration,
a whole fit on a planted sticky chain and the behaviour of the interface."""
import functools
import importlib
import pickle
import warnings

import numpy as np
import pytest

from tests import gmm_checks as GC
from tests import hmm_checks as HC

pytestmark = pytest.mark.gpu
H = importlib.import_module("scrubvae_amd.eval.hmm")  # the package exports the function hmm under the module's name


def length_sets(L):
    return [[1], [2], [L], [L + 1], [3 * L + 5], [1, L, 2, 2 * L + 1, 7]]


@pytest.mark.parametrize("K", [3, 16, 17, 33, 64])
def test_pass_inside_the_gates(K):
    from scrubvae_amd import _lib
    L = int(_lib.lib().svae_hmm_segment(K))
    assert L == HC.segment_length(K) and int(_lib.lib().svae_hmm_padded(K)) == HC.padded(K)
    pi, A = HC.chain(K, seed=K)
    for i, lengths in enumerate(length_sets(L)):
        n = int(np.sum(lengths))
        x, means, _ = HC.overlapping(n, K, 4, seed=100 * K + i)
        B, lpn = HC.emissions(x, means)
        ref = HC.plain(B, lpn, pi, A, lengths, np.longdouble)
        got = H.forward_backward(B, lpn, pi, A, lengths)
        used = HC.check_pass(got, ref, K, lengths, L)
        print("K", K, "lengths", lengths, "share of the gates", used)
        assert max(used.values()) <= 1.0, (lengths, used)
        assert np.abs(got["gamma"].sum(0) - 1.0).max() <= (K + 2) * HC.U
        assert got["work"] == int(_lib.lib().svae_hmm_work(K, got["nseg"]))


def test_structural_zeros():
    K = 5
    L = HC.segment_length(K)
    A = np.zeros((K, K))
    for i in range(K - 1):
        A[i, i], A[i, i + 1] = 0.9, 0.1
    A[K - 1, K - 1] = 1.0
    pi = np.zeros(K)
    pi[0] = 1.0
    n = 3 * L + 5
    st = np.minimum(np.arange(n) // (n // K + 1), K - 1)
    means = np.arange(K)[:, None] * 60.0 * np.ones((1, 2))
    x = (means[st] + np.random.default_rng(0).normal(size=(n, 2))).astype(np.float32)
    B, lpn = HC.emissions(x, means)
    assert (B == 0).any()
    ref = HC.plain(B, lpn, pi, A, [n], np.longdouble)
    got = H.forward_backward(B, lpn, pi, A, [n])
    for k in ("gamma", "Xi", "start_post", "c"):
        assert np.isfinite(got[k]).all(), k
    for k in ("gamma", "Xi", "start_post"):
        assert (got[k][np.asarray(ref[k] == 0)] == 0).all(), k
    assert np.isfinite(got["loglik"])
    used = HC.check_pass(got, ref, K, [n], L)
    print("structural zeros: share of the gates", used)
    assert max(used.values()) <= 1.0, used


def test_sequences_are_separable_bit_for_bit():
    K = 17
    L = HC.segment_length(K)
    lengths = [L + 44, 2 * L + 1, 40]
    pi, A = HC.chain(K, seed=2)
    x, means, _ = HC.overlapping(sum(lengths), K, 4, seed=9)
    B, lpn = HC.emissions(x, means)
    lo = np.cumsum([0] + lengths[:-1])
    both = H.forward_backward(B, lpn, pi, A, lengths)
    again = H.forward_backward(B, lpn, pi, A, lengths)
    for k in ("gamma", "c", "Xi", "start_post"):
        assert np.array_equal(both[k], again[k]), k
    assert both["loglik"] == again["loglik"]
    order = [2, 1, 0]
    cols = np.concatenate([np.arange(lo[s], lo[s] + lengths[s]) for s in order])
    rev = H.forward_backward(B[:, cols], lpn[cols], pi, A, [lengths[s] for s in order])
    rlo = np.cumsum([0] + [lengths[s] for s in order][:-1])
    for pos, s in enumerate(order):
        sl = slice(lo[s], lo[s] + lengths[s])
        alone = H.forward_backward(B[:, sl], lpn[sl], pi, A, [lengths[s]])
        rsl = slice(rlo[pos], rlo[pos] + lengths[s])
        for k in ("gamma", "c"):
            assert np.array_equal(both[k][..., sl], alone[k]), (k, s)
            assert np.array_equal(both[k][..., sl], rev[k][..., rsl]), (k, s)


def _hand_model(K, d, seed, cov="full"):
    from scrubvae_amd.eval import GaussianHMM
    g = np.random.default_rng(seed)
    m = GaussianHMM(K, covariance_type=cov)
    m.startprob_, m.transmat_ = HC.chain(K, seed)
    m.means_ = g.normal(size=(K, d))
    m.precisions_cholesky_ = np.ones((K, d)) if cov == "diag" else np.stack([np.eye(d)] * K)
    m.covars_ = m.precisions_cholesky_.copy()
    m.n_features_in_ = d
    return m


def test_input_kinds_give_the_same_bits():
    import torch
    m = _hand_model(6, 4, seed=3)
    lengths = [300, 13]
    x, _, _ = HC.overlapping(313, 6, 4, seed=4)
    outs = [m.score_samples(v, lengths) for v in (x, x.astype(np.float64), torch.from_numpy(x), torch.from_numpy(x).cuda())]
    for ll, post in outs[1:]:
        assert ll == outs[0][0] and np.array_equal(post, outs[0][1])
    assert outs[0][1].shape == (313, 6)
    assert np.array_equal(m.predict_proba(x, lengths), outs[0][1]) and m.score(x, lengths) == outs[0][0]
    assert np.array_equal(m.predict(x, lengths), m.predict(torch.from_numpy(x).cuda(), lengths))


def test_viterbi_equals_the_numpy_recursion():
    g = np.random.default_rng(11)
    for K, lengths in ((3, [7]), (5, [1, 2, 300, 33]), (64, [600, 70]), (17, [257])):
        n = sum(lengths)
        logB = np.log(g.random((K, n)))
        pi, A = HC.chain(K, seed=K, sticky=0.5)
        if K == 5:  # planted ties and impossible moves
            logB[1], logB[2, ::3] = logB[0], -np.inf
            A[:, 1] = A[:, 0]
            A[3, 4] = 0.0
            A /= A.sum(1, keepdims=True)
            pi[1] = pi[0]
        with np.errstate(divide="ignore"):
            ls, lt = np.log(pi), np.log(A)
        states, lp = H.viterbi(logB, ls, lt, lengths)
        rs, rlp = HC.viterbi(logB, ls, lt, lengths)
        assert np.array_equal(states, rs), K
        assert np.array_equal(lp, rlp), K
    # through the model: the same recursion on the log densities read back from the device
    m = _hand_model(6, 4, seed=3)
    x, _, _ = HC.overlapping(700, 6, 4, seed=5)
    lengths = [400, 300]
    _, logB = m._log_emissions(x, lengths)
    rs, rlp = HC.viterbi(logB.cpu().numpy(), np.log(m.startprob_), np.log(m.transmat_), lengths)
    lp, states = m.decode(x, lengths)
    assert np.array_equal(states, rs) and lp == float(rlp.sum())


@pytest.mark.parametrize("cov", ["full", "diag"])
def test_one_em_iteration(cov):
    """the device's iteration against the restated one (mixture E- and M-step of gmm_checks.py around the long-double pass): the
    pass gate plus the mixture M-step's tolerance of test_gpu_gmm.py (1e-9 of the scale)"""
    K, d, diag = 6, 4, cov == "diag"
    lengths = [HC.segment_length(K) + 30, 400, 5]
    n = sum(lengths)
    x, means, _ = HC.overlapping(n, K, d, seed=21, sep=3.0)
    pi, A = HC.chain(K, seed=8)
    P = np.ones((K, d)) if diag else np.stack([np.eye(d)] * K)
    got = H.em_step(x, lengths, pi, A, means, P, covariance_type=cov, reg_covar=1e-6)
    ref = HC.em_iteration(x, lengths, pi, A, means, P, diag, 1e-6, dtype=np.longdouble)
    x64 = x.astype(np.float64)
    lpn, resp = GC.estep(x64, np.ones(K), means, P, diag)
    fb = HC.plain(resp.T, lpn, pi, A, lengths, np.longdouble)
    g = HC.gates(K, lengths, HC.segment_length(K), fb)
    scale = np.abs(x64).max()
    print("loglik", got[0], ref[0], "gate", g["loglik"])
    assert abs(got[0] - ref[0]) <= g["loglik"] + 1e-10 * abs(ref[0])
    assert np.abs(got[1] - ref[1]).max() <= g["start_post"] + 1e-9
    assert np.abs(got[2] - ref[2]).max() <= 2 * g["Xi"] + 1e-9
    assert np.abs(got[3] - ref[3]).max() <= (g["gamma"] + 1e-9) * scale
    assert np.abs(got[4] - ref[4]).max() <= (g["gamma"] + 1e-9) * np.abs(ref[4]).max()
    assert np.abs(got[5] - ref[5]).max() <= (g["gamma"] + 1e-9) * np.abs(ref[5]).max()


# the restated fit of HC.planted_sticky(seed=0) (tests/hmm_checks.py::fit, random_state=0), run on the CPU when this test was written
PLANTED = dict(lengths=[1500, 1300, 1200], n_iter=13, first=-23807.907, last=-23288.649, agree_hmm=0.57375, agree_init=0.372)


@functools.lru_cache(maxsize=None)
def _planted():
    x, st = HC.planted_sticky(seed=0)
    return x, st, HC.fit(x, PLANTED["lengths"], 4, random_state=0)


def _agreement(labels, truth):
    from scrubvae_amd.eval import hungarian_match
    return float((hungarian_match(labels, truth) == truth).mean())


def test_fit_on_a_planted_sticky_chain():
    from scrubvae_amd.eval import GaussianHMM
    x, st, ref = _planted()
    lengths, n = PLANTED["lengths"], len(x)
    assert ref["n_iter"] == PLANTED["n_iter"] and ref["converged"]
    assert abs(ref["history"][0] - PLANTED["first"]) < 1e-3 and abs(ref["history"][-1] - PLANTED["last"]) < 1e-3
    assert _agreement(ref["states"], st) == PLANTED["agree_hmm"] and _agreement(ref["initial_labels"], st) == PLANTED["agree_init"]
    m = GaussianHMM(4, random_state=0).fit(x, lengths)
    assert m.n_iter_ == ref["n_iter"] and m.converged_
    # The accumulated gate (tests/hmm_checks.py, "A fit adds ..."): both runs evaluate iteration i within own[i] = the pass's
    # log-likelihood gate + the emissions' sum e_E at that iteration's parameters; the parameters entering iteration i come from
    # the initial mixture and i - 1 M-steps, each within the mixture M-step's tolerance delta = 1e-9 (test_gpu_gmm.py), which moves
    # the log-likelihood by delta x sensitivity[i]; the chain's entries differ by the Xi gate (twice: row sums) + delta per
    # iteration, n x that in the log-likelihood.  Nothing is assumed to contract, so the differences add up over the iterations.
    hist, rh = np.array(m.history_), np.array(ref["history"])
    own, it = ref["own_gate"], np.arange(1, len(rh) + 1)
    follow = 2 * own + it * (1e-9 * ref["sensitivity"] + n * (2 * ref["xi_gate"] + 1e-9))
    print("history - restated", hist - rh, "gate", follow, "own", own)
    assert (np.abs(hist - rh) <= follow).all()
    # EM does not decrease the likelihood: a computed decrease is at most the two evaluations' own gates
    assert (np.diff(hist) >= -(own[1:] + own[:-1])).all()
    states = m.predict(x, lengths)
    got_hmm, got_init = _agreement(states, st), _agreement(m.initial_labels_, st)
    print("agreement", got_hmm, got_init)
    assert got_hmm > got_init + 0.1  # the restated run: 0.574 against 0.372
    assert abs(got_hmm - PLANTED["agree_hmm"]) < 0.01
    assert np.allclose(m.transmat_.sum(1), 1.0, atol=1e-14) and abs(m.startprob_.sum() - 1.0) < 1e-14
    m2 = GaussianHMM(4, random_state=0).fit(x, lengths)
    assert m2.history_ == m.history_ and np.array_equal(m2.transmat_, m.transmat_) and np.array_equal(m2.means_, m.means_)


def test_convergence_warning_pickle_and_cache(tmp_path):
    from scrubvae_amd.eval import GaussianHMM, hmm
    from scrubvae_amd.eval.cluster import ConvergenceWarning
    x, st, _ = _planted()
    x, lengths = x[:1500], [1000, 500]
    with pytest.warns(ConvergenceWarning):
        m = GaussianHMM(4, n_iter=1, random_state=0).fit(x, lengths)
    assert m.n_iter_ == 1 and not m.converged_ and len(m.history_) == 1
    m2 = pickle.loads(pickle.dumps(m))
    for k in ("startprob_", "transmat_", "means_", "covars_", "precisions_cholesky_"):
        assert isinstance(getattr(m2, k), np.ndarray) and getattr(m2, k).dtype == np.float64
        assert np.array_equal(getattr(m2, k), getattr(m, k))
    assert np.array_equal(m2.predict(x, lengths), m.predict(x, lengths))
    path = str(tmp_path) + "/"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        s1, h1 = hmm(x, label="a", path=path, lengths=lengths, n_components=3, random_state=1)
    assert (tmp_path / "a_hmm.p").exists() and (tmp_path / "a_hmm.npy").exists() and isinstance(h1, GaussianHMM)
    s2, h2 = hmm(x, label="a", path=path, lengths=lengths, n_components=3, random_state=1)
    assert np.array_equal(s1, s2) and np.array_equal(h1.transmat_, h2.transmat_)
    assert np.array_equal(s1, h1.predict(x, lengths))
    (tmp_path / "a_hmm.npy").unlink()
    s3, _ = hmm(x, label="a", path=path, lengths=lengths, n_components=3)
    assert np.array_equal(s3, s1)


@pytest.mark.parametrize("cov", ["full", "diag"])
def test_not_positive_definite_raises(cov):
    x, _, _ = HC.overlapping(500, 3, 4, seed=2)
    x[:, 2] = 1.5  # a constant column: its variance is exactly 0 in every state
    pi, A = HC.chain(3, seed=1)
    P = np.ones((3, 4)) if cov == "diag" else np.stack([np.eye(4)] * 3)
    means = np.random.default_rng(0).normal(size=(3, 4))
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        H.em_step(x, None, pi, A, means, P, covariance_type=cov, reg_covar=0.0)


@pytest.mark.parametrize("cov", ["full", "diag"])
def test_fit_raises_when_not_positive_definite(cov, monkeypatch):
    from scrubvae_amd.eval import GaussianHMM
    x, _, _ = HC.overlapping(500, 3, 4, seed=2)
    x[:, 2] = 1.5
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        GaussianHMM(3, covariance_type=cov, reg_covar=0.0, random_state=0).fit(x)  # the initial mixture refuses already

    class Regularised(H.GaussianMixture):  # let the initial mixture through, so that the HMM's own M-step meets the zero variance
        def __init__(self, *a, **k):
            super().__init__(*a, **dict(k, reg_covar=1e-6))

    monkeypatch.setattr(H, "GaussianMixture", Regularised)
    before = H._HMM_CALLS["mstep"]
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        GaussianHMM(3, covariance_type=cov, reg_covar=0.0, random_state=0).fit(x)
    assert H._HMM_CALLS["mstep"] == before + 1  # raised by the fit loop after its first iteration


@pytest.mark.parametrize("cov", ["full", "diag"])
def test_library_calls_per_em_iteration(cov):
    import torch
    K, d, lengths = 5, 4, [700, 3]
    n = sum(lengths)
    x, means, _ = HC.overlapping(n, K, d, seed=3)
    dev = torch.device("cuda", torch.cuda.current_device())
    R = H._Rows(torch.from_numpy(x).cuda(), K, cov == "diag", dev)
    R.set_params(np.ones(K), means, np.ones((K, d)) if cov == "diag" else np.stack([np.eye(d)] * K))
    em = H._HmmEM(R, np.array(lengths), 1e-6, 1.0, 1.0)
    em.set_chain(*HC.chain(K, seed=1))
    want = dict(H.CALLS_PER_ITERATION)
    if cov == "diag":
        want["factor"] = want["precision"] = 0
    assert sum(want.values()) == (6 if cov == "diag" else 8)
    for _ in range(2):
        before = dict(H._HMM_CALLS)
        _, ok = em.iterate()
        assert ok and {k: H._HMM_CALLS[k] - before[k] for k in want} == want
    # inference: scoring is one E-step and one pass, decoding one E-step and one Viterbi call and no pass
    m = _hand_model(K, d, seed=3)
    before = dict(H._HMM_CALLS)
    m.score(x, lengths)
    assert {k: H._HMM_CALLS[k] - before[k] for k in want} == dict(want, mstep=0, factor=0, precision=0, update=0)
    before = dict(H._HMM_CALLS)
    m.predict(x, lengths)
    assert {k: v - before[k] for k, v in H._HMM_CALLS.items() if v != before[k]} == {"estep": 1, "viterbi": 1}


def test_launches_and_workspace_equal_the_queries():
    import torch
    from scrubvae_amd import _lib
    lib = _lib.lib()
    K, lengths = 33, [700, 3]
    n = sum(lengths)
    p = H._Pass(n, K, np.array(lengths), torch.device("cuda", torch.cuda.current_device()))
    L = int(lib.svae_hmm_segment(K))
    assert p.nseg == sum(-(-ln // L) for ln in lengths) and p.nseq == 2
    assert p.work.numel() == int(lib.svae_hmm_work(K, p.nseg))
    KP, nb = int(lib.svae_hmm_padded(K)), int(lib.svae_hmm_xi_blocks(p.nseg))
    assert nb == min(p.nseg, 1024)
    assert p.work.numel() == p.nseg * KP * KP + 2 * p.nseg * KP + p.nseg + nb * KP * KP + (p.nseg * KP + 1) // 2
    x, means, _ = HC.overlapping(n, K, 4, seed=1)
    B, lpn = HC.emissions(x, means)
    pi, A = HC.chain(K, seed=1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for it in range(1, 3):
        p.run(dev(B), dev(lpn), dev(pi), dev(A))
        assert p.launches == it * H.LAUNCHES_PER_PASS
