"""CPU checks of the Gaussian HMM: the segmented restatement inside its gates against long double, Viterbi against enumeration,
the segment table, run lengths, argument errors before the device, defaults, the C ABI declarations and the constants."""
import importlib
import inspect

import numpy as np
import pytest

from tests import abi_header as ABI
from tests import hmm_checks as HC

H = importlib.import_module("scrubvae_amd.eval.hmm")  # the package exports the function hmm under the module's name


def length_sets(L):
    return [[1], [2], [L], [L + 1], [3 * L + 5], [1, L, 2, 2 * L + 1, 7]]


@pytest.mark.parametrize("K", [3, 16, 17, 33, 64])
def test_segmented_restatement_inside_the_gates(K):
    L = HC.segment_length(K)
    pi, A = HC.chain(K, seed=K)
    for i, lengths in enumerate(length_sets(L)):
        n = int(np.sum(lengths))
        x, means, _ = HC.overlapping(n, K, 4, seed=100 * K + i)
        B, lpn = HC.emissions(x, means)
        ref = HC.plain(B, lpn, pi, A, lengths, np.longdouble)
        assert float(ref["gamma"].min()) > 1e6 * HC.FLOOR  # the reference stays clear of the floor
        got = HC.segmented(B, lpn, pi, A, lengths, L)
        used = HC.check_pass(got, ref, K, lengths, L)
        print(K, lengths, used)
        assert max(used.values()) <= 1.0, (lengths, used)
        assert np.abs(got["gamma"].sum(0) - 1.0).max() <= (K + 2) * HC.U


def test_segmented_restatement_with_structural_zeros():
    K, L = 5, 64
    A = np.zeros((K, K))
    for i in range(K):
        A[i, i], A[i, min(i + 1, K - 1)] = 0.9, A[i, min(i + 1, K - 1)] + 0.1
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
    got = HC.segmented(B, lpn, pi, A, [n], L)
    for k in ("gamma", "Xi", "start_post"):
        assert np.isfinite(got[k]).all()
        assert (got[k][np.asarray(ref[k] == 0)] == 0).all()
    assert max(HC.check_pass(got, ref, K, [n], L).values()) <= 1.0


def test_viterbi_equals_enumeration():
    g = np.random.default_rng(5)
    K, T = 3, 7
    for trial in range(20):
        logB = np.log(g.random((K, T)))
        pi, A = HC.chain(K, seed=trial, sticky=0.3)
        if trial % 2:  # planted ties: equal rows and columns
            logB[1] = logB[0]
            A[:, 1] = A[:, 0]
            A /= A.sum(1, keepdims=True)
            pi[1] = pi[0]
        states, lp = HC.viterbi(logB, np.log(pi), np.log(A))
        best, _ = HC.viterbi_brute(logB, np.log(pi), np.log(A))
        assert lp[0] == best
        s = np.log(pi)[states[0]] + logB[states[0], 0]
        for t in range(1, T):
            s = s + np.log(A)[states[t - 1], states[t]]
            s = s + logB[states[t], t]
        assert s == best


@pytest.mark.parametrize("lengths", [[1], [255], [256], [257], [1, 255, 256, 257, 600, 3]])
def test_segment_table(lengths):
    L = 256
    seg, seq = H.segment_table(lengths, L)
    rseg, rseq = HC.segment_table(lengths, L)
    assert seg.dtype == np.int32 and np.array_equal(seg, rseg) and np.array_equal(seq, rseq)
    assert seg[:, 1].sum() == sum(lengths) and (seg[:, 1] >= 1).all() and (seg[:, 1] <= L).all()
    assert np.array_equal(seg[1:, 0], np.cumsum(seg[:, 1])[:-1])  # the segments tile the frames in order
    starts = np.cumsum([0] + lengths[:-1])
    assert np.array_equal(seg[seg[:, 2] == 1, 0], starts)        # a sequence begins a segment: none crosses a boundary
    assert np.array_equal(seq[:, 1], [-(-ln // L) for ln in lengths])


def test_state_runs_and_dwell_times():
    from scrubvae_amd.eval import dwell_times, state_runs
    s = [2, 2, 2, 0, 0, 2, 1, 1, 1, 1]
    st, start, ln = state_runs(s)
    assert st.tolist() == [2, 0, 2, 1] and start.tolist() == [0, 3, 5, 6] and ln.tolist() == [3, 2, 1, 4]
    st, start, ln = state_runs(s, [2, 6, 2])  # boundaries cut the runs 2 2 | 2 0 0 2 1 1 | 1 1
    assert st.tolist() == [2, 2, 0, 2, 1, 1] and start.tolist() == [0, 2, 3, 5, 6, 8] and ln.tolist() == [2, 1, 2, 1, 2, 2]
    d = dwell_times(s, n_states=4)
    assert d["mean"][:3].tolist() == [2.0, 4.0, 2.0] and d["median"][:3].tolist() == [2.0, 4.0, 2.0] and np.isnan(d["mean"][3])
    assert d["occupancy"].tolist() == [0.2, 0.4, 0.4, 0.0] and d["count"].tolist() == [1, 1, 2, 0]
    assert len(dwell_times(s)["mean"]) == 3
    with pytest.raises(ValueError):
        state_runs(s, [4, 4])
    with pytest.raises(ValueError):
        dwell_times(s, n_states=2)


def _forbid_device(monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(H, "_device_of", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)


@pytest.mark.parametrize("kwargs,x,lengths", [
    (dict(covariance_type="tied"), None, None),
    (dict(covariance_type="spherical"), None, None),
    (dict(n_components=65), np.zeros((100, 4)), None),
    (dict(n_components=0), None, None),
    (dict(n_components=3), np.zeros((2, 4)), None),
    (dict(n_components=2, n_iter=0), None, None),
    (dict(n_components=2, tol=-1.0), None, None),
    (dict(n_components=2, transmat_prior=-1.0), None, None),
    (dict(n_components=2), np.zeros((10, 129)), None),
    (dict(n_components=2), np.array([[0.0, 1.0], [np.nan, 2.0], [1.0, 1.0]]), None),
    (dict(n_components=2), None, [20, 20]),      # does not sum to n
    (dict(n_components=2), None, [50, 0]),       # a length below 1
    (dict(n_components=2), None, [25.0, 25.0]),  # not integers
    (dict(n_components=2), None, [[50]]),
])
def test_value_errors_before_the_device(monkeypatch, kwargs, x, lengths):
    from scrubvae_amd.eval import GaussianHMM
    _forbid_device(monkeypatch)
    if x is None:
        x = np.random.default_rng(0).normal(size=(50, 3))
    with pytest.raises(ValueError):
        GaussianHMM(**kwargs).fit(x, lengths)


def test_defaults_and_exports():
    import scrubvae_amd.eval as E
    sig = inspect.signature(E.GaussianHMM.__init__)
    want = dict(n_components=1, covariance_type="full", n_iter=100, tol=1e-3, reg_covar=1e-6, transmat_prior=1.0, startprob_prior=1.0,
                init_iter=10, random_state=None, verbose=0)
    assert {k: p.default for k, p in sig.parameters.items() if k != "self"} == want
    assert all(p.kind is p.KEYWORD_ONLY for k, p in sig.parameters.items() if k not in ("self", "n_components"))
    hs = inspect.signature(E.hmm)
    assert [(k, p.default) for k, p in hs.parameters.items()] == [("latents", inspect._empty), ("lengths", None), ("n_components", 25),
                                                                 ("covariance_type", "full"), ("random_state", None),
                                                                 ("label", "cluster"), ("path", None)]  # then gmm()'s cache arguments
    for name in ("GaussianHMM", "hmm", "state_runs", "dwell_times"):
        assert callable(getattr(E, name))
    for m in ("fit", "score", "score_samples", "predict_proba", "predict", "decode"):
        assert list(inspect.signature(getattr(E.GaussianHMM, m)).parameters)[1:] == ["X", "lengths"]


def test_abi_names_and_constants_equal_the_header():
    from scrubvae_amd import _lib
    assert ABI.declared("svae_hmm_") == {"svae_hmm_padded", "svae_hmm_segment", "svae_hmm_xi_blocks", "svae_hmm_work",
                                         "svae_hmm_transfer_f64", "svae_hmm_carry_f64", "svae_hmm_fill_f64", "svae_hmm_update_f64",
                                         "svae_hmm_viterbi"}
    assert _lib.HMM_MAX_STATES == _lib.GMM_MAX_COMPONENTS == 64
    assert _lib.HMM_SEGMENT == HC.SEGMENT
    for K in (1, 16, 17, 32, 33, 64):
        assert H.padded_states(K) == HC.padded(K) and H.segment_length(K) == HC.segment_length(K)


def test_without_device_raises_runtime_error(monkeypatch):
    import torch
    from scrubvae_amd.eval import GaussianHMM
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError):
        GaussianHMM(2).fit(np.random.default_rng(0).normal(size=(50, 3)))
