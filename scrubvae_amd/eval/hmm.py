"""Segmentation of latents in time: a hidden Markov model with Gaussian emissions fitted on the device.

    GaussianHMM(n_components=1, *, covariance_type="full", n_iter=100, tol=1e-3, reg_covar=1e-6, transmat_prior=1.0,
                startprob_prior=1.0, init_iter=10, random_state=None, verbose=0)
      .fit(X, lengths=None) .score(X, lengths=None) .score_samples(X, lengths=None) -> (loglik, posteriors)
      .predict_proba(X, lengths=None) .predict(X, lengths=None) .decode(X, lengths=None) -> (logprob, states)
      startprob_, transmat_, means_, covars_, precisions_cholesky_, history_, n_iter_, converged_
    hmm(latents, lengths=None, n_components=25, covariance_type="full", random_state=None) -> (states, model)
    state_runs(states, lengths=None) -> (state, start, length)
    dwell_times(states, lengths=None, n_states=None) -> dict(mean, median, occupancy, count), one entry per state

The latents are consecutive windows of a recording; `lengths` (hmmlearn's convention: positive integers that sum to n, None = one
sequence) says where one recording ends and the next begins.  The emissions are the Gaussians of GaussianMixture (full or diagonal
covariance), the hidden state follows a Markov chain, and the fit is Baum-Welch (EM):

  E-step   svae_gmm_estep_f64 with unit weights gives, per frame, the emission densities scaled to sum to one and the log of the
           scale; csrc/hmm.hip runs the scaled forward-backward pass over them, parallel in time and exact: transfer matrices of
           segments of svae_hmm_segment(K) frames on the fp64 matrix cores, a carry over the segments of a sequence, the plain
           recursion inside every segment.
  M-step   svae_gmm_mstep_f64 with the smoothed posteriors as responsibilities (then the mixture's factor and precision calls),
           transmat = Xi + transmat_prior - 1 and startprob = start_post + startprob_prior - 1, row-normalised (Dirichlet
           pseudo-counts; negative entries are clipped to 0; a row whose total is 0 keeps its old values).

Initialisation: the project's GaussianMixture(n_components, covariance_type, max_iter=init_iter, random_state) gives the emission
parameters, startprob starts uniform and transmat from the counts of consecutive mixture labels within sequences plus 1; it is
deterministic given random_state.  The host reads one record per iteration (log-likelihood, not-positive-definite flag); the fit
stops when the mean log-likelihood per frame moves by less than tol, as the mixture's.  history_ holds the total log-likelihood of
every iteration's E-step.  predict and decode use Viterbi (one workgroup per sequence); predict_proba and score_samples the
posteriors.  Rows go in as for GaussianMixture (read as fp32 once, fp64 after that); fitted attributes are host numpy fp64.

hmmlearn, pomegranate and ssm are not dependencies and were not available to pin against: the defaults and the random draws are
this project's own, not hmmlearn's.  Limits: d <= 128, n_components <= 64, n < 2^26, every length >= 1; covariance "full" or "diag".
"""
from __future__ import annotations

import functools
import numbers
import warnings

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from .cluster import (COVARIANCE_TYPES, _EM, _NOT_PD, ConvergenceWarning, GaussianMixture, _check_model_exists, _Rows, _rows32)

MAX_FRAMES = 1 << 26
LAUNCHES_PER_PASS = 3  # library calls of one forward-backward pass: transfer, carry, fill
# library calls by this process, by entry point, and what one EM iteration adds to them (full covariance; "diag" makes neither the
# factor nor the precision call: its M-step writes the precisions itself)
_HMM_CALLS = {k: 0 for k in ("estep", "transfer", "carry", "fill", "mstep", "factor", "precision", "update", "viterbi")}
CALLS_PER_ITERATION = {"estep": 1, "transfer": 1, "carry": 1, "fill": 1, "mstep": 1, "factor": 1, "precision": 1, "update": 1, "viterbi": 0}

_device_of = functools.partial(_device._device_of, who="GaussianHMM runs on the GPU (csrc/hmm.hip); no device is available")


def padded_states(K):
    """the padded state count of the kernels (svae_hmm_padded)"""
    return 16 if K <= 16 else 32 if K <= 32 else 64


def segment_length(K):
    """the segment length of the time-parallel pass, a function of K alone (svae_hmm_segment)"""
    return _lib.HMM_SEGMENT[padded_states(K)]


def _check_lengths(lengths, n):
    """lengths as an int64 array of positive integers summing to n (None: one sequence)"""
    if lengths is None:
        return np.array([n], dtype=np.int64)
    a = np.asarray(lengths)
    if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("lengths must be a non-empty 1D array of integers")
    a = a.astype(np.int64)
    if (a < 1).any():
        raise ValueError("every length must be >= 1")
    if int(a.sum()) != n:
        raise ValueError(f"lengths sum to {int(a.sum())}, but there are {n} rows")
    return a


def segment_table(lengths, L):
    """The host's segment table: every sequence cut into segments of L frames, the last one shorter.
    -> seg [nseg, 4] int32 = {first frame, frames, first segment of its sequence, sequence},
       seq [nseq, 4] int32 = {first segment, segments, first frame, frames}"""
    lengths = np.asarray(lengths, np.int64)
    nsegs = (lengths + L - 1) // L
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    first_seg = np.concatenate([[0], np.cumsum(nsegs)[:-1]])
    seq = np.stack([first_seg, nsegs, starts, lengths], 1).astype(np.int32)
    sid = np.repeat(np.arange(len(lengths)), nsegs)
    within = np.arange(int(nsegs.sum())) - first_seg[sid]
    t0 = starts[sid] + within * L
    ln = np.minimum(L, starts[sid] + lengths[sid] - t0)
    seg = np.stack([t0, ln, within == 0, sid], 1).astype(np.int32)
    return seg, seq


class _Pass:
    """Device buffers of the forward-backward pass over n frames of K states cut by `lengths`, and the pass itself."""

    def __init__(self, n, K, lengths, device, L=None):
        self.n, self.K, self.device = n, K, device
        lib = _lib.lib()
        self.L = int(lib.svae_hmm_segment(K)) if L is None else int(L)
        seg, seq = segment_table(lengths, self.L)
        self.nseg, self.nseq = len(seg), len(seq)
        self.seg = torch.from_numpy(seg).to(device)
        self.seq = torch.from_numpy(seq).to(device)
        f64 = dict(dtype=torch.float64, device=device)
        self.work = torch.empty(int(lib.svae_hmm_work(K, self.nseg)), **f64)
        self.gamma = torch.empty(K, n, **f64)
        self.c = torch.empty(n, **f64)
        self.Xi = torch.empty(K, K, **f64)
        self.start_post = torch.empty(K, **f64)
        self.loglik = torch.empty(1, **f64)
        self.launches = 0

    def transfer(self, B, transmat):
        check(_lib.lib().svae_hmm_transfer_f64(B.data_ptr(), B.stride(0), self.n, self.K, transmat.data_ptr(), self.seg.data_ptr(),
                                               self.nseg, self.seq.data_ptr(), self.nseq, self.work.data_ptr(), ops._stream()),
              "hmm_transfer_f64")
        self.launches += 1
        _HMM_CALLS["transfer"] += 1

    def carry(self, startprob):
        check(_lib.lib().svae_hmm_carry_f64(self.n, self.K, startprob.data_ptr(), self.seg.data_ptr(), self.nseg, self.seq.data_ptr(),
                                            self.nseq, self.work.data_ptr(), ops._stream()), "hmm_carry_f64")
        self.launches += 1
        _HMM_CALLS["carry"] += 1

    def fill(self, B, lpn, transmat):
        check(_lib.lib().svae_hmm_fill_f64(B.data_ptr(), B.stride(0), lpn.data_ptr(), self.n, self.K, transmat.data_ptr(),
                                           self.seg.data_ptr(), self.nseg, self.seq.data_ptr(), self.nseq, self.work.data_ptr(),
                                           self.gamma.data_ptr(), self.c.data_ptr(), self.Xi.data_ptr(), self.start_post.data_ptr(),
                                           self.loglik.data_ptr(), ops._stream()), "hmm_fill_f64")
        self.launches += 1
        _HMM_CALLS["fill"] += 1

    def run(self, B, lpn, startprob, transmat):
        """B [K, n], lpn [n], startprob [K], transmat [K, K] on the device -> gamma, Xi, start_post, loglik in this object"""
        self.transfer(B, transmat)
        self.carry(startprob)
        self.fill(B, lpn, transmat)


def forward_backward(B, lpn, startprob, transmat, lengths=None, L=None):
    """The pass alone, on scaled emissions B [K, n] and their log scales lpn [n] (numpy arrays or tensors) -> dict of host arrays
    gamma [K, n], c [n], Xi [K, K], start_post [K] and loglik.  L overrides the segment length (the tests and the benchmark)."""
    dev = _device_of(B if torch.is_tensor(B) else np.zeros(1))
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        Bd = torch.as_tensor(B).to(**f64).contiguous()
        K, n = Bd.shape
        p = _Pass(n, K, _check_lengths(lengths, n), dev, L=L)
        p.run(Bd, torch.as_tensor(lpn).to(**f64).contiguous(), torch.as_tensor(startprob).to(**f64).contiguous(),
              torch.as_tensor(transmat).to(**f64).contiguous())
        return dict(gamma=p.gamma.cpu().numpy(), c=p.c.cpu().numpy(), Xi=p.Xi.cpu().numpy(), start_post=p.start_post.cpu().numpy(),
                    loglik=float(p.loglik.item()), work=p.work.numel(), nseg=p.nseg)


def viterbi(logB, log_startprob, log_transmat, lengths=None):
    """Viterbi paths on the device from logB [K, n] (numpy array or tensor) -> (states [n] int64, logprob [nseq])"""
    dev = _device_of(logB if torch.is_tensor(logB) else np.zeros(1))
    with torch.cuda.device(dev):
        f64 = dict(dtype=torch.float64, device=dev)
        lb = torch.as_tensor(logB).to(**f64).contiguous()
        K, n = lb.shape
        _, seq = segment_table(_check_lengths(lengths, n), 1 << 30)
        return _viterbi(lb, torch.as_tensor(log_startprob).to(**f64).contiguous(), torch.as_tensor(log_transmat).to(**f64).contiguous(),
                        torch.from_numpy(seq).to(dev))


def _viterbi_device(logB, log_start, log_trans, seq):
    """the kernel alone -> (states [n] int32, logprob [nseq]) on the device"""
    K, n = logB.shape
    dev = logB.device
    bp = torch.empty(n * K, dtype=torch.uint8, device=dev)
    states = torch.empty(n, dtype=torch.int32, device=dev)
    logprob = torch.empty(len(seq), dtype=torch.float64, device=dev)
    check(_lib.lib().svae_hmm_viterbi(log_start.data_ptr(), log_trans.data_ptr(), logB.data_ptr(), n, K, seq.data_ptr(), len(seq),
                                      bp.data_ptr(), states.data_ptr(), logprob.data_ptr(), ops._stream()), "hmm_viterbi")
    _HMM_CALLS["viterbi"] += 1
    return states, logprob


def _viterbi(logB, log_start, log_trans, seq):
    states, logprob = _viterbi_device(logB, log_start, log_trans, seq)
    return states.cpu().numpy().astype(np.int64), logprob.cpu().numpy()


class _HmmState:
    """Device state of a model on rows R (_Rows): the scaled emissions B [K, n] and their log scales, the chain parameters, and
    the pass, whose buffers are made when it is first asked for (Viterbi needs none of them)."""

    def __init__(self, R, lengths, B=None):
        self.R, self.lengths = R, lengths
        f64 = R.f64
        self.B = torch.empty(R.K, R.n, **f64) if B is None else B
        self.lpn = torch.empty(R.n, **f64)
        self.startprob, self.transmat = torch.empty(R.K, **f64), torch.empty(R.K, R.K, **f64)
        self._p = None

    @property
    def p(self):
        if self._p is None:
            self._p = _Pass(self.R.n, self.R.K, self.lengths, self.R.device)
        return self._p

    def set_chain(self, startprob, transmat):
        self.startprob.copy_(torch.from_numpy(np.ascontiguousarray(startprob, np.float64)))
        self.transmat.copy_(torch.from_numpy(np.ascontiguousarray(transmat, np.float64)))

    def emissions(self):
        self.R.estep(resp=self.B, lpn=self.lpn)
        _HMM_CALLS["estep"] += 1

    def estep(self):
        """emissions and the pass -> the posteriors in self.p"""
        self.emissions()
        self.p.run(self.B, self.lpn, self.startprob, self.transmat)


class _HmmEM(_HmmState):
    """Device state of one Baum-Welch fit: _HmmState with the mixture's M-step buffers (_EM), whose resp holds the emissions."""

    def __init__(self, R, lengths, reg_covar, transmat_prior, startprob_prior):
        self.em = _EM(R, reg_covar)
        super().__init__(R, lengths, B=self.em.resp)
        self.tprior, self.sprior = float(transmat_prior), float(startprob_prior)
        self.ones = torch.ones(R.K, **R.f64)

    def iterate(self):
        """one EM iteration on the device -> (log-likelihood of its E-step, all covariances positive definite)"""
        R, em, p, L, st = self.R, self.em, self.p, _lib.lib(), ops._stream()
        self.estep()
        check(L.svae_gmm_mstep_f64(R.A.data_ptr(), R.lda, R.d, R.n, R.K, int(R.diag), p.gamma.data_ptr(), em.reg, em.mpart.data_ptr(),
                                   em.s1.data_ptr(), em.nk.data_ptr(), em.w.data_ptr(), R.mu.data_ptr(), em.cov.data_ptr(),
                                   R.P.data_ptr(), R.cst.data_ptr(), em.bad.data_ptr(), st), "gmm_mstep_f64")
        _HMM_CALLS["mstep"] += 1
        if R.diag:
            R.cst.sub_(torch.log(em.w))  # the M-step's constant carries log w; the emissions have unit weights
        else:
            check(L.svae_spd_factor_solve_f64(em.cov.data_ptr(), R.d, R.d * R.d, R.d, R.K, None, 0, 0, em.Lf.data_ptr(), None,
                                              em.logdet.data_ptr(), em.rank.data_ptr(), 0.0, st), "spd_factor_solve_f64")
            check(L.svae_gmm_precision_f64(em.Lf.data_ptr(), em.rank.data_ptr(), self.ones.data_ptr(), R.d, R.K, R.ldp, R.P.data_ptr(),
                                           R.cst.data_ptr(), em.bad.data_ptr(), st), "gmm_precision_f64")
            _HMM_CALLS["factor"] += 1
            _HMM_CALLS["precision"] += 1
        check(L.svae_hmm_update_f64(p.Xi.data_ptr(), p.start_post.data_ptr(), R.K, self.tprior, self.sprior, self.transmat.data_ptr(),
                                    self.startprob.data_ptr(), st), "hmm_update_f64")
        _HMM_CALLS["update"] += 1
        res = torch.cat([p.loglik, em.bad.max().double().view(1)]).cpu().numpy()
        return float(res[0]), res[1] == 0

    def params(self):
        """host fp64 (startprob, transmat, means, covariances, precisions_cholesky)"""
        _, means, cov, P = self.em.params()
        return self.startprob.cpu().numpy(), self.transmat.cpu().numpy(), means, cov, P


def _initial_transmat(labels, lengths, K):
    """counts of consecutive labels within sequences, plus 1, row-normalised"""
    counts = np.ones((K, K))
    inside = np.ones(len(labels) - 1, bool)
    inside[np.cumsum(lengths)[:-1] - 1] = False
    np.add.at(counts, (labels[:-1][inside], labels[1:][inside]), 1.0)
    return counts / counts.sum(1, keepdims=True)


class GaussianHMM:
    """Hidden Markov model with Gaussian emissions ("full" or "diag" covariance) fitted by EM on the GPU (module docstring)."""

    runs_on_device = True  # gmm()'s caching decorator predicts with the model itself

    def __init__(self, n_components=1, *, covariance_type="full", n_iter=100, tol=1e-3, reg_covar=1e-6, transmat_prior=1.0,
                 startprob_prior=1.0, init_iter=10, random_state=None, verbose=0):
        self.n_components = n_components
        self.covariance_type = covariance_type
        self.n_iter = n_iter
        self.tol = tol
        self.reg_covar = reg_covar
        self.transmat_prior = transmat_prior
        self.startprob_prior = startprob_prior
        self.init_iter = init_iter
        self.random_state = random_state
        self.verbose = verbose

    def _check_parameters(self):
        if self.covariance_type not in COVARIANCE_TYPES:
            raise ValueError(f"covariance_type {self.covariance_type!r} is not supported: use one of {COVARIANCE_TYPES}")
        if not isinstance(self.n_components, numbers.Integral) or self.n_components < 1:
            raise ValueError(f"n_components must be an integer >= 1, got {self.n_components!r}")
        if self.n_components > _lib.HMM_MAX_STATES:
            raise ValueError(f"n_components={self.n_components} > {_lib.HMM_MAX_STATES} is not supported")
        if not isinstance(self.n_iter, numbers.Integral) or self.n_iter < 1:
            raise ValueError(f"n_iter must be an integer >= 1, got {self.n_iter!r}")
        if not isinstance(self.init_iter, numbers.Integral) or self.init_iter < 0:
            raise ValueError(f"init_iter must be an integer >= 0, got {self.init_iter!r}")
        if not (self.tol >= 0 and self.reg_covar >= 0):
            raise ValueError("tol and reg_covar must be >= 0")
        if not (self.transmat_prior >= 0 and self.startprob_prior >= 0):
            raise ValueError("transmat_prior and startprob_prior must be >= 0")

    def _rows(self, X, lengths, fitting):
        """validated fp32 rows and lengths -- every ValueError comes before the device is touched"""
        if fitting:
            self._check_parameters()
        x = _rows32(X)
        n, d = x.shape
        if d < 1 or n < 1:
            raise ValueError(f"Found array with shape {tuple(x.shape)}")
        if d > _lib.CV_MAX_DIM:
            raise ValueError(f"{d} features > {_lib.CV_MAX_DIM} is not supported")
        if n >= MAX_FRAMES:
            raise ValueError(f"{n} frames >= 2^26 is not supported")
        if fitting:
            if n < max(2, self.n_components):
                raise ValueError(f"Expected n_samples >= max(2, n_components) = {max(2, self.n_components)}, got n_samples={n}")
        elif d != self.n_features_in_:
            raise ValueError(f"X has {d} features, but GaussianHMM is expecting {self.n_features_in_} features as input.")
        return x, _check_lengths(lengths, n)

    def fit(self, X, lengths=None):
        x, lengths = self._rows(X, lengths, True)
        dev = _device_of(x)
        K, diag = int(self.n_components), self.covariance_type == "diag"
        with torch.cuda.device(dev):
            xt = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            xt = xt.to(dev)
            gm = GaussianMixture(K, covariance_type=self.covariance_type, max_iter=int(self.init_iter), reg_covar=self.reg_covar,
                                 random_state=self.random_state)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", ConvergenceWarning)
                labels = gm.fit_predict(xt)
            R = _Rows(xt, K, diag, dev)
            n, d = R.n, R.d
            R.set_params(np.ones(K), gm.means_, gm.precisions_cholesky_)
            em = _HmmEM(R, lengths, self.reg_covar, self.transmat_prior, self.startprob_prior)
            startprob, transmat = np.full(K, 1.0 / K), _initial_transmat(labels, lengths, K)
            em.set_chain(startprob, transmat)
            means, cov, P = gm.means_, gm.covariances_, gm.precisions_cholesky_
            prev, history, converged, it = -np.inf, [], False, 0
            for it in range(1, int(self.n_iter) + 1):
                loglik, ok = em.iterate()
                if not ok:
                    raise ValueError(_NOT_PD)
                history.append(loglik)
                change = (loglik - prev) / n
                prev = loglik
                if self.verbose >= 2:
                    print(f"  Iteration {it}\t log-likelihood: {loglik}\t change per frame: {change}")
                if abs(change) < self.tol:
                    converged = True
                    break
            startprob, transmat, means, cov, P = em.params()
            if self.verbose >= 1:
                print(f"GaussianHMM {'converged' if converged else 'did not converge'} after {it} iterations. log-likelihood: {prev}")
            if not converged:
                warnings.warn("The fit did not converge. Try a larger n_iter or tol, or check for degenerate data.", ConvergenceWarning)
            self.startprob_, self.transmat_, self.means_, self.covars_, self.precisions_cholesky_ = startprob, transmat, means, cov, P
            self.history_, self.n_iter_, self.converged_ = [float(h) for h in history], int(it), bool(converged)
            self.initial_labels_ = np.asarray(labels, np.int64)
            self.n_features_in_ = d
        return self

    def _fitted(self, X, lengths):
        """the device state of the fitted model on new rows, the chain parameters uploaded"""
        if not hasattr(self, "means_"):
            raise RuntimeError("This GaussianHMM instance is not fitted yet. Call 'fit' first.")
        x, lengths = self._rows(X, lengths, False)
        dev = _device_of(x)
        K, diag = self.means_.shape[0], self.covariance_type == "diag"
        xt = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        with torch.cuda.device(dev):
            R = _Rows(xt.to(dev), K, diag, dev)
            R.set_params(np.ones(K), np.asarray(self.means_, np.float64), np.asarray(self.precisions_cholesky_, np.float64))
            em = _HmmState(R, lengths)  # no M-step buffers, and no pass until one is run
            em.set_chain(self.startprob_, self.transmat_)
        return em

    def score_samples(self, X, lengths=None):
        """(total log-likelihood, posteriors [n, K])"""
        em = self._fitted(X, lengths)
        with torch.cuda.device(em.R.device):
            em.estep()
            return float(em.p.loglik.item()), em.p.gamma.cpu().numpy().T.copy()

    def score(self, X, lengths=None):
        return self.score_samples(X, lengths)[0]

    def predict_proba(self, X, lengths=None):
        return self.score_samples(X, lengths)[1]

    def _log_emissions(self, X, lengths=None):
        """(device state, logB [K, n] on the device): the log densities Viterbi reads, computed once outside its kernel, in the
        buffer of the emissions (the only K x n array of a Viterbi call)"""
        em = self._fitted(X, lengths)
        with torch.cuda.device(em.R.device):
            em.emissions()
            return em, em.B.log_().add_(em.lpn[None, :])

    def decode(self, X, lengths=None):
        """(log-probability of the Viterbi paths, summed over the sequences; states [n])"""
        em, logB = self._log_emissions(X, lengths)
        with torch.cuda.device(em.R.device):
            with np.errstate(divide="ignore"):
                ls, lt = np.log(np.asarray(self.startprob_, np.float64)), np.log(np.asarray(self.transmat_, np.float64))
            dev = em.R.device
            seq = torch.from_numpy(segment_table(em.lengths, 1 << 30)[1]).to(dev)
            states, logprob = _viterbi(logB, torch.from_numpy(ls).to(dev), torch.from_numpy(np.ascontiguousarray(lt)).to(dev), seq)
            return float(logprob.sum()), states

    def predict(self, X, lengths=None):
        return self.decode(X, lengths)[1]


def em_step(X, lengths, startprob, transmat, means, precisions_cholesky, covariance_type="full", reg_covar=1e-6, transmat_prior=1.0,
            startprob_prior=1.0):
    """One EM iteration from given parameters on the device: (log-likelihood of the E-step, startprob, transmat, means, covariances,
    precisions_cholesky after the M-step).  Raises ValueError when a covariance is not positive definite."""
    x = _rows32(X)
    lengths = _check_lengths(lengths, x.shape[0])
    dev = _device_of(x)
    means = np.asarray(means, np.float64)
    K = means.shape[0]
    with torch.cuda.device(dev):
        xt = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        R = _Rows(xt.to(dev), K, covariance_type == "diag", dev)
        R.set_params(np.ones(K), means, np.asarray(precisions_cholesky, np.float64))
        em = _HmmEM(R, lengths, reg_covar, transmat_prior, startprob_prior)
        em.set_chain(startprob, transmat)
        loglik, ok = em.iterate()
        if not ok:
            raise ValueError(_NOT_PD)
        return (loglik,) + em.params()


def _fit_hmm(latents, lengths=None, n_components=25, covariance_type="full", random_state=None):
    return GaussianHMM(n_components=n_components, covariance_type=covariance_type, reg_covar=1e-5, random_state=random_state,
                       verbose=1).fit(latents, lengths)


_fit_hmm.__name__ = "hmm"                # the cache files are {path}{label}_hmm.p and .npy
_fit_hmm.predict_keys = ("lengths",)     # arguments the cached model's predict takes along with the latents
_fit_hmm.model_name = "HMM"              # what the decorator's messages call the model
_cached_hmm = _check_model_exists(_fit_hmm)


def hmm(latents, lengths=None, n_components=25, covariance_type="full", random_state=None, label="cluster", path=None):
    """GaussianHMM(n_components, covariance_type, reg_covar=1e-5, verbose=1) fitted to the latents -> (states, model), the Viterbi
    states; cached as gmm() caches: {path}{label}_hmm.p and .npy"""
    return _cached_hmm(latents, label=label, path=path, lengths=lengths, n_components=n_components, covariance_type=covariance_type,
                       random_state=random_state)


def state_runs(states, lengths=None):
    """Maximal runs of one state within sequences -> (state, start, length) int64 arrays, in time order; a run ends at a sequence
    boundary even when the next sequence begins in the same state."""
    s = np.asarray(states)
    if s.ndim != 1:
        raise ValueError("states must be a 1D array")
    n = len(s)
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy()
    lengths = _check_lengths(lengths, n)
    brk = np.zeros(n, bool)
    brk[0] = True
    brk[1:] = s[1:] != s[:-1]
    brk[np.cumsum(lengths)[:-1]] = True
    start = np.flatnonzero(brk)
    return s[start].astype(np.int64), start.astype(np.int64), np.diff(np.append(start, n)).astype(np.int64)


def dwell_times(states, lengths=None, n_states=None):
    """Per state: mean and median run length in frames (nan for a state that never occurs), occupancy (the share of frames) and the
    number of runs -> dict(mean, median, occupancy, count) of arrays [n_states] (default: largest state + 1)."""
    st, _, ln = state_runs(states, lengths)
    K = int(n_states) if n_states is not None else (int(st.max()) + 1 if len(st) else 0)
    if len(st) and (st.min() < 0 or st.max() >= K):
        raise ValueError(f"states must lie in [0, {K})")
    mean, median = np.full(K, np.nan), np.full(K, np.nan)
    occ, count = np.zeros(K), np.zeros(K, np.int64)
    total = max(int(ln.sum()), 1)
    for k in range(K):
        r = ln[st == k]
        count[k] = len(r)
        if len(r):
            mean[k], median[k], occ[k] = r.mean(), np.median(r), r.sum() / total
    return dict(mean=mean, median=median, occupancy=occ, count=count)
