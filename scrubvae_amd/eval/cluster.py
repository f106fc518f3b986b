"""Clustering of latents on the device (reference: src/scrubvae/eval/cluster.py::gmm and ::dbscan, and the fits of
eval/metrics.py::epoch_cluster_entropy).

    GaussianMixture(n_components=1, *, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100,
                    init_params="k-means++", random_state=None, verbose=0)
    gmm(latents, label="cluster", path=None, n_components=25, covariance_type="full", random_state=None) -> (k_pred, model)

GaussianMixture restates sklearn 1.7's GaussianMixture with n_init=1 and k-means++ seeding: the same arguments, methods and
fitted attributes (host numpy fp64 arrays), the same host random draws (check_random_state, RandomState.choice and .uniform in
sklearn's order), the same initial parameters (responsibilities one-hot at the seeds: nk = 1 + 10 eps, means = x_seed / nk,
weights = nk / n) and the same EM loop (lower bound = mean log-likelihood of the E-step before each M-step, stop when it moves by
less than tol, a final E-step for the labels).  The seeding rounds, the E-steps and the M-steps run in csrc/gmm.hip; the host
sends a few draws per seeding round and reads one lower bound per EM iteration.  sklearn is never imported.

Input rows (numpy array or torch tensor, CPU or device, [n, d]) are read as fp32, as the decodability metrics read latents:
fp64 input is rounded to fp32 once.  Everything after that is fp64.

Differences from sklearn, by design:
  - all arithmetic is fp64, summed in a fixed order.  sklearn keeps float32 latents in float32 and forms X P - mu P (full) and
    E[x^2] - mu^2 (diag), which cancel; here the E-step forms (x - mu) P and the M-step sums about the new means (two passes).
    A fit on float32 latents therefore follows the same algorithm and the same random draws as the reference but not its
    rounding: it can pick different k-means++ seeds and end at a slightly different optimum.
  - k-means++ distances are sum (x - c)^2, not |x|^2 - 2 x.c + |c|^2.
  - the initial covariance is exactly reg_covar * I (sklearn's carries a rounding residue of order |x|^2 eps).
Only covariance_type in {"full", "diag"}, init_params="k-means++" and n_init=1 are supported; d <= 128 and n_components <= 64.

    KMeans(n_clusters=8, *, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, verbose=0, random_state=None, copy_x=True,
           algorithm="lloyd")
    kmeans(latents, label="cluster", path=None, n_clusters=25, random_state=None) -> (k_pred, model)

KMeans restates sklearn 1.7's KMeans(algorithm="lloyd") with unit sample weights: rows centred by their mean, tol scaled by the mean
column variance, the same host draws (k-means++ through the seeding above, or RandomState.choice for init="random", nothing else
between restarts), Lloyd's iteration with sklearn's two stopping tests, the relocation of empty clusters, the extra assignment
after a stop by tol, the restart kept by inertia unless it is the same clustering renumbered.  The iteration runs in
csrc/kmeans.hip (assignment, per-cluster sums on the fp64 matrix cores, new centres); the host reads one record of three numbers
per iteration.  Input rows are read as for the mixture: fp32 once, fp64 after that.

Differences from sklearn's KMeans, by design:
  - all arithmetic is fp64 in a fixed order, also for float32 input; distances are sum (x - c)^2 in feature order, not
    |x|^2 - 2 x.c + |c|^2, and a row at equal distance from two centres takes the lower index.
  - new centres are sums / count (sklearn multiplies by 1 / count); the shift is sum |new - old|^2 (sklearn squares the rounded
    norms); a cluster emptied by a relocation keeps its old centre; tol's variance is the centred rows' sum of squares / (n d).
  - empty clusters take the rows farthest from their centres with the lower row first on equal distances (sklearn's argpartition
    leaves ties open).
  - predict, transform and score centre the new rows at their own mean and shift the centres alike, as the mixture's predict does.
Only unit sample weights, algorithm="lloyd" and init in {"k-means++", "random", an array} are supported; d <= 128,
n_clusters <= 1024 and n_samples >= n_clusters.
"""
from __future__ import annotations

import functools
import numbers
import pickle
import warnings
from pathlib import Path

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from .metrics import ConvergenceWarning as _MetricsConvergenceWarning

_EPS10 = 10.0 * np.finfo(np.float64).eps
_LOG2PI = np.log(2.0 * np.pi)
COVARIANCE_TYPES = ("full", "diag")
INIT_PARAMS = ("k-means++",)
_NOT_PD = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused "
           "by singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input "
           "data. The numerical accuracy can also be improved by passing float64 data instead of float32.")


class ConvergenceWarning(_MetricsConvergenceWarning):
    """An EM fit stopped at max_iter with the lower bound still moving by tol or more, or a k-means fit ended with fewer than
    n_clusters distinct labels (sklearn's ConvergenceWarning)."""


def check_random_state(seed):
    """sklearn.utils.check_random_state: None -> numpy's global RandomState, an int -> RandomState(int), an instance as it is."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def _pad8(d):
    return (int(d) + 7) // 8 * 8


def _rows32(X):
    """X as fp32 [n, d]: a host numpy array, or a torch tensor left where it is"""
    if torch.is_tensor(X):
        t = X.detach()
        if t.dim() != 2:
            raise ValueError(f"Expected 2D array, got {t.dim()}D tensor instead")
        if t.dtype != torch.float32:
            t = t.to(torch.float32)
        if not bool(torch.isfinite(t).all()):
            raise ValueError("Input X contains NaN or infinity.")
        return t
    a = np.asarray(X)
    if a.ndim != 2:
        raise ValueError(f"Expected 2D array, got {a.ndim}D array instead")
    with np.errstate(over="ignore"):
        a = a.astype(np.float32)
    if not np.isfinite(a).all():
        raise ValueError("Input X contains NaN or infinity.")
    return a


_device_of = functools.partial(_device._device_of, who="GaussianMixture runs on the GPU (csrc/gmm.hip); no device is available")


def _host_log_det(P, diag):
    return np.log(P).sum(1) if diag else np.log(np.diagonal(P, axis1=1, axis2=2)).sum(1)


class _Centred:
    """fp32 rows [n, d] on the device, centred once into the fp64 matrix A [n][lda] (svae_cv_center) every kernel reads, and the
    k-means++ seeding of K of them."""

    def __init__(self, x, K, device):
        n, d = x.shape
        self.n, self.d, self.K, self.device = n, d, K, device
        self.lda = ops.pad16(d + 1)
        f64 = dict(dtype=torch.float64, device=device)
        self.f64 = f64
        x = x.to(device=device, dtype=torch.float32).contiguous()
        perm = torch.arange(n, dtype=torch.int32, device=device)
        self.mean_d = torch.empty(d, **f64)
        self.A = torch.empty(n, self.lda, **f64)
        check(_lib.lib().svae_cv_center(x.data_ptr(), d, d, None, 0, 0, perm.data_ptr(), n, self.mean_d.data_ptr(), self.A.data_ptr(),
                                        self.lda, ops._stream()), "cv_center")
        self.mean = self.mean_d.cpu().numpy()

    def kmeans_pp(self, rs):
        """sklearn's _kmeans_plusplus with unit sample weights: host draws, device distances; returns the K seed row indices"""
        n, K = self.n, self.K
        L = _lib.lib()
        st = ops._stream()
        T = 2 + int(np.log(K))
        nb = L.svae_gmm_kpp_blocks(n)
        f64 = self.f64
        closest, tot = torch.empty(n, **f64), torch.empty(nb, **f64)
        d2, part = torch.empty(T, n, **f64), torch.empty(T, nb, **f64)
        vals = torch.empty(T, **f64)
        cand = torch.empty(T, dtype=torch.int32, device=self.device)
        out = torch.empty(2, **f64)  # pot, then the chosen row as an int32 pair view
        out_i = torch.empty(2, dtype=torch.int32, device=self.device)
        center_id = int(rs.choice(n, p=np.ones(n) / n))
        cand[0] = center_id
        indices = [center_id]
        check(L.svae_gmm_kpp_round(self.A.data_ptr(), self.lda, self.d, n, None, 1, cand.data_ptr(), closest.data_ptr(), tot.data_ptr(),
                                   d2.data_ptr(), part.data_ptr(), out.data_ptr(), out_i.data_ptr(), out_i[1:].data_ptr(), st),
              "gmm_kpp_round")
        pot = float(out[0].item())
        for _ in range(1, K):
            rv = rs.uniform(size=T) * pot
            vals.copy_(torch.from_numpy(rv))
            check(L.svae_gmm_kpp_round(self.A.data_ptr(), self.lda, self.d, n, vals.data_ptr(), T, cand.data_ptr(), closest.data_ptr(),
                                       tot.data_ptr(), d2.data_ptr(), part.data_ptr(), out.data_ptr(), out_i.data_ptr(),
                                       out_i[1:].data_ptr(), st), "gmm_kpp_round")
            pot = float(out[0].item())
            indices.append(int(out_i[0].item()))
        return np.array(indices, dtype=np.int64)


class _Rows(_Centred):
    """The centred rows and the device parameters of the E-step (means in the centred frame, precision factors, constants)."""

    def __init__(self, x, K, diag, device):
        super().__init__(x, K, device)
        d, f64 = self.d, self.f64
        self.diag = bool(diag)
        self.ldp = d if diag else _pad8(d)
        self.mu = torch.empty(K, d, **f64)
        self.P = torch.zeros(K, d, self.ldp, **f64) if not diag else torch.empty(K, d, **f64)
        self.cst = torch.empty(K, **f64)

    def set_params(self, weights, means, prec):
        """upload host parameters (sklearn's weights_, means_, precisions_cholesky_)"""
        K, d = self.K, self.d
        cst = np.log(weights) + _host_log_det(prec, self.diag) - 0.5 * d * _LOG2PI
        self.mu.copy_(torch.from_numpy(np.ascontiguousarray(means - self.mean[None, :])))
        if self.diag:
            self.P.copy_(torch.from_numpy(np.ascontiguousarray(prec)))
        else:
            Pp = np.zeros((K, d, self.ldp))
            Pp[:, :, :d] = np.triu(prec)
            self.P.copy_(torch.from_numpy(Pp))
        self.cst.copy_(torch.from_numpy(np.asarray(cst, np.float64)))

    def estep(self, resp=None, lpn=None, part=None, label=None, gap=None):
        check(_lib.lib().svae_gmm_estep_f64(self.A.data_ptr(), self.lda, self.d, self.n, self.K, int(self.diag), self.mu.data_ptr(),
                                            self.P.data_ptr(), self.ldp, self.cst.data_ptr(), ops._p(resp), ops._p(lpn), ops._p(part),
                                            ops._p(label), ops._p(gap), ops._stream()), "gmm_estep_f64")

    def labels(self, want_gap=False):
        label = torch.empty(self.n, dtype=torch.int32, device=self.device)
        gap = torch.empty(self.n, **self.f64) if want_gap else None
        self.estep(label=label, gap=gap)
        lab = label.cpu().numpy().astype(np.int64)
        return (lab, gap.cpu().numpy()) if want_gap else lab

    def resp_lpn(self):
        resp = torch.empty(self.K, self.n, **self.f64)
        lpn = torch.empty(self.n, **self.f64)
        self.estep(resp=resp, lpn=lpn)
        return resp, lpn


class _EM:
    """Device state of one EM fit on _Rows R: responsibilities, M-step buffers and the current parameters."""

    def __init__(self, R, reg_covar):
        self.R, self.reg = R, float(reg_covar)
        K, d, n = R.K, R.d, R.n
        L = _lib.lib()
        f64 = R.f64
        self.resp = torch.empty(K, n, **f64)
        self.nblk = L.svae_gmm_estep_blocks(n)
        self.epart = torch.empty(self.nblk, **f64)
        self.chunks = L.svae_gmm_chunks(n, d)
        self.mpart = torch.empty(self.chunks * K * max(d + 1, d if R.diag else d * d), **f64)
        self.s1 = torch.empty(K, d + 1, **f64)
        self.nk, self.w = torch.empty(K, **f64), torch.empty(K, **f64)
        self.cov = torch.empty(K, d, **f64) if R.diag else torch.empty(K, d, d, **f64)
        self.Lf = None if R.diag else torch.empty(K, d, d, **f64)
        self.logdet = torch.empty(K, **f64)
        self.rank = torch.empty(K, dtype=torch.int32, device=R.device)
        self.bad = torch.zeros(K, dtype=torch.int32, device=R.device)
        self.lb = torch.empty(1, **f64)

    def iterate(self):
        """E-step (lower bound) and M-step on the device -> (lower bound, all covariances positive definite)"""
        R, L, st = self.R, _lib.lib(), ops._stream()
        R.estep(resp=self.resp, part=self.epart)
        check(L.svae_gmm_sum_f64(self.epart.data_ptr(), self.nblk, float(R.n), self.lb.data_ptr(), st), "gmm_sum_f64")
        check(L.svae_gmm_mstep_f64(R.A.data_ptr(), R.lda, R.d, R.n, R.K, int(R.diag), self.resp.data_ptr(), self.reg, self.mpart.data_ptr(),
                                   self.s1.data_ptr(), self.nk.data_ptr(), self.w.data_ptr(), R.mu.data_ptr(), self.cov.data_ptr(),
                                   R.P.data_ptr(), R.cst.data_ptr(), self.bad.data_ptr(), st), "gmm_mstep_f64")
        if not R.diag:
            check(L.svae_spd_factor_solve_f64(self.cov.data_ptr(), R.d, R.d * R.d, R.d, R.K, None, 0, 0, self.Lf.data_ptr(), None,
                                              self.logdet.data_ptr(), self.rank.data_ptr(), 0.0, st), "spd_factor_solve_f64")
            check(L.svae_gmm_precision_f64(self.Lf.data_ptr(), self.rank.data_ptr(), self.w.data_ptr(), R.d, R.K, R.ldp, R.P.data_ptr(),
                                           R.cst.data_ptr(), self.bad.data_ptr(), st), "gmm_precision_f64")
        res = torch.cat([self.lb, self.bad.max().double().view(1)]).cpu().numpy()
        return float(res[0]), res[1] == 0

    def params(self):
        """host fp64 (weights, means, covariances, precisions_cholesky) of the current device parameters"""
        R = self.R
        w = self.w.cpu().numpy()
        means = R.mu.cpu().numpy() + R.mean[None, :]
        cov = self.cov.cpu().numpy()
        P = R.P.cpu().numpy() if R.diag else R.P[:, :, :R.d].cpu().numpy()
        return w, means, cov, P


def _initial_params(x_seed, n, reg, diag):
    """GaussianMixture._initialize with responsibilities one-hot at the seeds"""
    K, d = x_seed.shape
    nk = 1.0 + _EPS10
    means = x_seed.astype(np.float64) / nk
    weights = np.full(K, nk / n)
    if reg <= 0.0:
        raise ValueError(_NOT_PD)
    if diag:
        cov = np.full((K, d), reg)
        P = 1.0 / np.sqrt(cov)
    else:
        cov = np.broadcast_to(np.eye(d) * reg, (K, d, d)).copy()
        P = np.broadcast_to(np.eye(d) / np.sqrt(reg), (K, d, d)).copy()
    return weights, means, cov, P


class GaussianMixture:
    """sklearn.mixture.GaussianMixture (n_init=1, init_params="k-means++", covariance_type "full" or "diag") fitted on the GPU.

    X may be a numpy array or a torch tensor, on the CPU or the device, of shape [n, d]; rows are read as fp32 (fp64 input is
    rounded to fp32 once) and all arithmetic after that is fp64 (module docstring: differences from sklearn).  Fitted attributes
    are host numpy fp64 arrays with sklearn's names and shapes, so a fitted object pickles and unpickles without a GPU."""

    def __init__(self, n_components=1, *, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 init_params="k-means++", random_state=None, verbose=0):
        self.n_components = n_components
        self.covariance_type = covariance_type
        self.tol = tol
        self.reg_covar = reg_covar
        self.max_iter = max_iter
        self.n_init = n_init
        self.init_params = init_params
        self.random_state = random_state
        self.verbose = verbose

    def _check_parameters(self):
        if self.covariance_type not in COVARIANCE_TYPES:
            raise ValueError(f"covariance_type {self.covariance_type!r} is not supported: use one of {COVARIANCE_TYPES}")
        if self.init_params not in INIT_PARAMS:
            raise ValueError(f"init_params {self.init_params!r} is not supported: use 'k-means++'")
        if self.n_init != 1:
            raise ValueError(f"n_init={self.n_init} is not supported: only n_init=1")
        if not isinstance(self.n_components, numbers.Integral) or self.n_components < 1:
            raise ValueError(f"n_components must be an integer >= 1, got {self.n_components!r}")
        if self.n_components > _lib.GMM_MAX_COMPONENTS:
            raise ValueError(f"n_components={self.n_components} > {_lib.GMM_MAX_COMPONENTS} is not supported")
        if not isinstance(self.max_iter, numbers.Integral) or self.max_iter < 0:
            raise ValueError(f"max_iter must be an integer >= 0, got {self.max_iter!r}")
        if self.tol < 0 or self.reg_covar < 0:
            raise ValueError("tol and reg_covar must be >= 0")

    def _rows(self, X, fitting):
        """validated fp32 rows (host or device) -- every ValueError comes before the device is touched"""
        if fitting:
            self._check_parameters()
        x = _rows32(X)
        n, d = x.shape
        if fitting:
            if n < max(2, self.n_components):
                raise ValueError(f"Expected n_samples >= max(2, n_components) = {max(2, self.n_components)}, got n_samples={n}")
        elif d != self.n_features_in_:
            raise ValueError(f"X has {d} features, but GaussianMixture is expecting {self.n_features_in_} features as input.")
        if d > _lib.CV_MAX_DIM:
            raise ValueError(f"{d} features > {_lib.CV_MAX_DIM} is not supported")
        if d < 1 or n < 1:
            raise ValueError(f"Found array with shape {tuple(x.shape)}")
        return x

    def _fit(self, X):
        x = self._rows(X, True)
        dev = _device_of(x)
        K, diag = int(self.n_components), self.covariance_type == "diag"
        with torch.cuda.device(dev):
            xt = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            R = _Rows(xt, K, diag, dev)
            n, d = R.n, R.d
            rs = check_random_state(self.random_state)
            seeds = R.kmeans_pp(rs)
            x_seed = xt[torch.as_tensor(seeds, device=xt.device)].cpu().numpy()
            weights, means, cov, P = _initial_params(x_seed, n, float(self.reg_covar), diag)
            R.set_params(weights, means, P)
            em = _EM(R, self.reg_covar)
            lower_bound, bounds, converged, n_iter = -np.inf, [], False, 0
            for n_iter in range(1, self.max_iter + 1):
                prev = lower_bound
                lower_bound, ok = em.iterate()
                if not ok:
                    raise ValueError(_NOT_PD)
                bounds.append(lower_bound)
                change = lower_bound - prev
                if self.verbose >= 2:
                    print(f"  Iteration {n_iter}\t change: {change}")
                if abs(change) < self.tol:
                    converged = True
                    break
            if self.max_iter > 0:
                weights, means, cov, P = em.params()
            if self.verbose >= 1:
                print(f"Initialization {'converged' if converged else 'did not converge'}. lower bound: {lower_bound}")
            if not converged and self.max_iter > 0:
                warnings.warn("Best performing initialization did not converge. Try different init parameters, or increase max_iter, "
                              "tol, or check for degenerate data.", ConvergenceWarning)
            self.weights_, self.means_, self.covariances_, self.precisions_cholesky_ = weights, means, cov, P
            self.converged_, self.n_iter_ = bool(converged), int(n_iter if self.max_iter > 0 else 0)
            self.lower_bound_, self.lower_bounds_ = float(lower_bound), [float(b) for b in bounds]
            self.n_features_in_ = d
            # the final E-step uses the host attributes, exactly as predict does: fit_predict(X) == fit(X).predict(X)
            R.set_params(self.weights_, self.means_, self.precisions_cholesky_)
            return R.labels()

    def fit(self, X, y=None):
        self._fit(X)
        return self

    def fit_predict(self, X, y=None):
        return self._fit(X)

    def _fitted_rows(self, X):
        if not hasattr(self, "means_"):
            raise RuntimeError("This GaussianMixture instance is not fitted yet. Call 'fit' first.")
        x = self._rows(X, False)
        dev = _device_of(x)
        K, diag = self.means_.shape[0], self.covariance_type == "diag"
        xt = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        with torch.cuda.device(dev):
            R = _Rows(xt, K, diag, dev)
            R.set_params(np.asarray(self.weights_, np.float64), np.asarray(self.means_, np.float64),
                         np.asarray(self.precisions_cholesky_, np.float64))
        return R

    def _predict_gap(self, X):
        """(labels, top-two gap of the weighted log probabilities) of each row"""
        R = self._fitted_rows(X)
        with torch.cuda.device(R.device):
            return R.labels(want_gap=True)

    def predict(self, X):
        R = self._fitted_rows(X)
        with torch.cuda.device(R.device):
            return R.labels()

    def predict_proba(self, X):
        R = self._fitted_rows(X)
        with torch.cuda.device(R.device):
            resp, _ = R.resp_lpn()
            return resp.cpu().numpy().T.copy()

    def score_samples(self, X):
        R = self._fitted_rows(X)
        with torch.cuda.device(R.device):
            _, lpn = R.resp_lpn()
            return lpn.cpu().numpy()

    def score(self, X, y=None):
        return float(self.score_samples(X).mean())


def em_step(X, weights, means, precisions_cholesky, covariance_type="full", reg_covar=1e-6):
    """One EM iteration from given parameters on the device: (lower bound of the E-step, weights, means, covariances,
    precisions_cholesky after the M-step).  Raises ValueError when a covariance is not positive definite."""
    x = _rows32(X)
    dev = _device_of(x)
    means = np.asarray(means, np.float64)
    K = means.shape[0]
    diag = covariance_type == "diag"
    with torch.cuda.device(dev):
        xt = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        R = _Rows(xt, K, diag, dev)
        R.set_params(np.asarray(weights, np.float64), means, np.asarray(precisions_cholesky, np.float64))
        em = _EM(R, reg_covar)
        lb, ok = em.iterate()
        if not ok:
            raise ValueError(_NOT_PD)
        return (lb,) + em.params()


class _Fitted(GaussianMixture):
    """a GaussianMixture built from another object's fitted attributes (e.g. an sklearn model unpickled by gmm())"""


def _as_device_model(model):
    """model itself when it is a GaussianMixture or KMeans of this module (or a GaussianHMM of eval/hmm.py), else a copy of sklearn's fitted attribute names of it"""
    if isinstance(model, (GaussianMixture, KMeans)) or getattr(model, "runs_on_device", False):
        return model
    if hasattr(model, "cluster_centers_"):
        m = KMeans(n_clusters=len(model.cluster_centers_))
        m.cluster_centers_ = np.asarray(model.cluster_centers_, np.float64)
        m.n_features_in_ = m.cluster_centers_.shape[1]
        return m
    m = _Fitted(n_components=len(model.weights_), covariance_type=model.covariance_type)
    m.weights_ = np.asarray(model.weights_, np.float64)
    m.means_ = np.asarray(model.means_, np.float64)
    m.precisions_cholesky_ = np.asarray(model.precisions_cholesky_, np.float64)
    m.n_features_in_ = m.means_.shape[1]
    return m


def _check_model_exists(func):
    """the reference's caching decorator (cluster.py:7-48): with a path, the model is pickled to {path}{label}_{name}.p and the
    labels saved to {path}{label}_{name}.npy; an existing pickle is loaded, and its labels too when that file exists.  A pickle
    without a labels file predicts (the reference raises UnboundLocalError there)."""

    what = getattr(func, "model_name", "GMM")  # the reference's messages say GMM

    @functools.wraps(func)
    def wrapper(latents, label="cluster", path=None, **kwargs):
        if path is None:
            model_exists = False
        else:
            model_path = "{}{}_{}.p".format(path, label, func.__name__)
            preds_path = "{}{}_{}.npy".format(path, label, func.__name__)
            model_exists = Path(model_path).exists()
        if model_exists:
            print("Found {} model - Loading ...".format(func.__name__))
            with open(model_path, "rb") as f:
                model = pickle.load(f)
        else:
            model = func(latents=latents, **kwargs)
            if path is not None:
                print("Saving {} model".format(what))
                with open(model_path, "wb") as f:
                    pickle.dump(model, f)
        if model_exists and Path(preds_path).exists():
            print("Found existing {} clusterings - Loading ...".format(func.__name__))
            k_pred = np.load(preds_path)
        else:
            print("Calculating {} clusters on the device ...".format(func.__name__))
            # func.predict_keys: the arguments predict takes along with the latents (hmm(): the sequence lengths)
            extra = {k: kwargs[k] for k in getattr(func, "predict_keys", ()) if k in kwargs}
            k_pred = _as_device_model(model).predict(latents, **extra)
            if path is not None:
                print("Saving {} cluster predictions".format(what))
                np.save(preds_path, k_pred)
        return k_pred, model

    return wrapper


@_check_model_exists
def gmm(latents, n_components=25, covariance_type="full", random_state=None):
    """GaussianMixture(n_components, covariance_type, max_iter=150, init_params="k-means++", reg_covar=1e-5, verbose=1) fitted to
    the latents (reference cluster.py:51-66) -> (k_pred, model)."""
    return GaussianMixture(n_components=n_components, covariance_type=covariance_type, max_iter=150, init_params="k-means++",
                           reg_covar=1e-5, random_state=random_state, verbose=1).fit(latents)


def dbscan(latents, eps=0.1, min_samples=500, label="cluster", path="./results/"):
    """HDBSCAN(min_cluster_size=min_samples).fit_predict(latents) on the device, the labels saved to {path}{label}_sc_pred.npy
    (reference cluster.py:69-87; eps is unused there too)."""
    from .hdbscan import HDBSCAN
    preds_path = "{}{}_sc_pred.npy".format(path, label)
    print("Calculating sklearn dbscan clusters ...")
    k_pred = HDBSCAN(min_cluster_size=min_samples).fit_predict(latents)
    print(len(np.unique(k_pred)))
    np.save(preds_path, k_pred)
    return k_pred


# ---- k-means ------------------------------------------------------------------------------------------------------------------------
KMEANS_INITS = ("k-means++", "random")
_km_device_of = functools.partial(_device._device_of, who="KMeans runs on the GPU (csrc/kmeans.hip); no device is available")


def _relocation_rows(dist, n_empty):
    """the rows the empty clusters take: by descending distance to their own centre, the lower row first on a tie"""
    return np.lexsort((np.arange(len(dist)), -dist))[:n_empty]


def _is_same_clustering(labels1, labels2, n_clusters):
    """sklearn's _is_same_clustering: labels2 is labels1 with the clusters renumbered"""
    mapping = np.full(n_clusters, -1, dtype=np.int64)
    u, first = np.unique(labels1, return_index=True)
    mapping[u] = labels2[first]
    return bool((mapping[labels1] == labels2).all())


class _Lloyd:
    """Device state of Lloyd's iteration on the centred rows R (_Centred): two centre and two label buffers that swap roles, the
    distances, the partial buffers of csrc/kmeans.hip and the record of one iteration."""

    def __init__(self, R, fitting=True):
        self.R = R
        n, d, K, dev, f64 = R.n, R.d, R.K, R.device, R.f64
        L = _lib.lib()
        self.nb = L.svae_kmeans_assign_blocks(n)
        self.ipart = torch.empty(self.nb, **f64)
        self.total = torch.empty(1, **f64)
        if not fitting:  # assignment only
            self.label = [torch.empty(n, dtype=torch.int32, device=dev)]
            return
        self.chunks = L.svae_kmeans_chunks(n, d, K)
        self.C = [torch.empty(K, d, **f64), torch.empty(K, d, **f64)]
        self.label = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]
        self.dist = torch.empty(n, **f64)
        self.part = torch.empty(self.chunks * K * (d + 1), **f64)
        self.sums = torch.empty(K, d + 1, **f64)
        self.changed = torch.zeros(1, dtype=torch.int32, device=dev)
        self.rec = torch.empty(3, **f64)

    def assign(self, C, label=None, prev=None, dist=None, gap=None, D=None, part=None, changed=None):
        R = self.R
        check(_lib.lib().svae_kmeans_assign_f64(R.A.data_ptr(), R.lda, R.d, R.n, C.data_ptr(), C.stride(0), C.shape[0], ops._p(prev),
                                                ops._p(label), ops._p(dist), ops._p(gap), ops._p(D), ops._p(part), ops._p(changed),
                                                ops._stream()), "kmeans_assign_f64")

    def update(self, label):
        R = self.R
        check(_lib.lib().svae_kmeans_update_f64(R.A.data_ptr(), R.lda, R.d, R.n, label.data_ptr(), R.K, self.part.data_ptr(),
                                                self.sums.data_ptr(), ops._stream()), "kmeans_update_f64")

    def finish(self, C_old, C_new, changed=None):
        """-> host (rows whose label changed, shift, empty clusters)"""
        R = self.R
        check(_lib.lib().svae_kmeans_finish_f64(self.sums.data_ptr(), R.d, R.K, C_old.data_ptr(), C_new.data_ptr(), C_old.stride(0),
                                                ops._p(changed), self.rec.data_ptr(), ops._stream()), "kmeans_finish_f64")
        rec = self.rec.cpu().numpy()
        return int(rec[0]), float(rec[1]), int(rec[2])

    def inertia(self):
        """the sum of the last assignment's distances (its block sums, added in a fixed order)"""
        check(_lib.lib().svae_gmm_sum_f64(self.ipart.data_ptr(), self.nb, 1.0, self.total.data_ptr(), ops._stream()), "gmm_sum_f64")
        return float(self.total.item())

    def sum_of_squares(self):
        """sum |a|^2 over the centred rows: the distances to one zero centre"""
        zero = torch.zeros(1, self.R.d, **self.R.f64)
        self.assign(zero, part=self.ipart)
        return self.inertia()

    def relocate(self, label):
        """the rare path: every empty cluster, in ascending order, takes one far row out of its cluster's sum and count"""
        d = self.R.d
        empty = np.flatnonzero(self.sums[:, d].cpu().numpy() == 0)
        lab = label.cpu().numpy()
        for c, r in zip(empty, _relocation_rows(self.dist.cpu().numpy(), len(empty))):
            row = self.R.A[int(r), :d + 1]
            self.sums[int(lab[r])] -= row
            self.sums[int(c)] = row

    def step(self, C, C_new, label, prev):
        """one iteration from the centres C: label, dist, C_new -> (changed, shift, empty clusters before relocation)"""
        self.assign(C, label=label, prev=prev, dist=self.dist, part=self.ipart, changed=self.changed)
        self.update(label)
        changed, shift, n_empty = self.finish(C, C_new, self.changed)
        if n_empty:
            self.relocate(label)
            _, shift, _ = self.finish(C, C_new, self.changed)
        return changed, shift, n_empty

    def run(self, C0, max_iter, tol_, verbose=0):
        """sklearn's _kmeans_single_lloyd from the centres C0 (device [K, d], centred frame) -> (labels, inertia, centres, n_iter),
        labels and centres on the device"""
        C, C_new = self.C
        C.copy_(C0)
        label, prev = self.label
        prev.fill_(-1)
        strict, n_iter = False, 0
        for n_iter in range(1, max_iter + 1):
            changed, shift, _ = self.step(C, C_new, label, prev)
            C, C_new = C_new, C
            if verbose:
                print(f"Iteration {n_iter - 1}, inertia {self.inertia()}.")
            if changed == 0:
                strict = True
                if verbose:
                    print(f"Converged at iteration {n_iter - 1}: strict convergence.")
                break
            if shift <= tol_:
                if verbose:
                    print(f"Converged at iteration {n_iter - 1}: center shift {shift} within tolerance {tol_}.")
                break
            label, prev = prev, label
        if not strict:
            self.assign(C, label=label, dist=self.dist, part=self.ipart)
        return label, self.inertia(), C, n_iter


class KMeans:
    """sklearn.cluster.KMeans (algorithm="lloyd", unit sample weights) fitted on the GPU.

    X may be a numpy array or a torch tensor, on the CPU or the device, of shape [n, d]; rows are read as fp32 (fp64 input is
    rounded to fp32 once) and all arithmetic after that is fp64 (module docstring: differences from sklearn).  Fitted attributes
    are host numpy arrays with sklearn's names and shapes, so a fitted object pickles and unpickles without a GPU."""

    def __init__(self, n_clusters=8, *, init="k-means++", n_init="auto", max_iter=300, tol=1e-4, verbose=0, random_state=None,
                 copy_x=True, algorithm="lloyd"):
        self.n_clusters = n_clusters
        self.init = init
        self.n_init = n_init
        self.max_iter = max_iter
        self.tol = tol
        self.verbose = verbose
        self.random_state = random_state
        self.copy_x = copy_x
        self.algorithm = algorithm

    def _init_array(self):
        return None if isinstance(self.init, str) or callable(self.init) else self.init

    def _check_parameters(self):
        if self.algorithm != "lloyd":
            raise ValueError(f"algorithm {self.algorithm!r} is not supported: only 'lloyd'")
        if callable(self.init):
            raise ValueError("a callable init is not supported: use 'k-means++', 'random' or an array")
        if isinstance(self.init, str) and self.init not in KMEANS_INITS:
            raise ValueError(f"init {self.init!r} is not supported: use one of {KMEANS_INITS} or an array")
        if not isinstance(self.n_clusters, numbers.Integral) or self.n_clusters < 1:
            raise ValueError(f"n_clusters must be an integer >= 1, got {self.n_clusters!r}")
        if self.n_clusters > _lib.KMEANS_MAX_CLUSTERS:
            raise ValueError(f"n_clusters={self.n_clusters} > {_lib.KMEANS_MAX_CLUSTERS} is not supported")
        if self.n_init != "auto" and (not isinstance(self.n_init, numbers.Integral) or self.n_init < 1):
            raise ValueError(f"n_init must be 'auto' or an integer >= 1, got {self.n_init!r}")
        if not isinstance(self.max_iter, numbers.Integral) or self.max_iter < 1:
            raise ValueError(f"max_iter must be an integer >= 1, got {self.max_iter!r}")
        if not self.tol >= 0:
            raise ValueError(f"tol must be >= 0, got {self.tol!r}")

    def _rows(self, X, fitting):
        """validated fp32 rows (host or device) -- every ValueError comes before the device is touched"""
        if fitting:
            self._check_parameters()
        if hasattr(X, "tocsr") or (torch.is_tensor(X) and X.layout != torch.strided):
            raise ValueError("sparse input is not supported")
        x = _rows32(X)
        n, d = x.shape
        if d > _lib.CV_MAX_DIM:
            raise ValueError(f"{d} features > {_lib.CV_MAX_DIM} is not supported")
        if d < 1 or n < 1:
            raise ValueError(f"Found array with shape {tuple(x.shape)}")
        if fitting:
            if n < self.n_clusters:
                raise ValueError(f"n_samples={n} should be >= n_clusters={self.n_clusters}.")
        elif d != self.n_features_in_:
            raise ValueError(f"X has {d} features, but KMeans is expecting {self.n_features_in_} features as input.")
        return x

    def _init_centres(self, d):
        """the init array as fp64 [K, d] (None for a named init), refused when its shape is wrong or a value is not finite"""
        init = self._init_array()
        if init is None:
            return None
        c = init.detach().cpu().numpy() if torch.is_tensor(init) else np.asarray(init)
        c = np.array(c, dtype=np.float64)
        if c.shape != (self.n_clusters, d):
            raise ValueError(f"The shape of the initial centers {c.shape} does not match (n_clusters, n_features) = "
                             f"({self.n_clusters}, {d}).")
        if not np.isfinite(c).all():
            raise ValueError("The initial centers contain NaN or infinity.")
        return c

    def _fit(self, X, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("sample_weight is not supported: only unit weights")
        x = self._rows(X, True)
        K = int(self.n_clusters)
        init = self._init_centres(x.shape[1])
        n_init = self.n_init
        if n_init == "auto":
            n_init = 1 if init is not None or self.init == "k-means++" else 10
        if init is not None and n_init != 1:
            warnings.warn("Explicit initial center position passed: performing only one init in KMeans instead of "
                          f"n_init={n_init}.", RuntimeWarning)
            n_init = 1
        dev = _km_device_of(x)
        with torch.cuda.device(dev):
            xt = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            rs = check_random_state(self.random_state)
            R = _Centred(xt, K, dev)
            n, d = R.n, R.d
            it = _Lloyd(R)
            tol_ = float(self.tol) * it.sum_of_squares() / (n * d)
            best = None
            for _ in range(n_init):
                if init is not None:
                    C0 = torch.from_numpy(init - R.mean[None, :]).to(dev)
                else:
                    seeds = R.kmeans_pp(rs) if self.init == "k-means++" else rs.choice(n, size=K, replace=False, p=np.ones(n) / n)
                    C0 = R.A[torch.as_tensor(np.asarray(seeds, np.int64), device=dev), :d]
                label, inertia, C, n_iter = it.run(C0, int(self.max_iter), tol_, self.verbose)
                labels = label.cpu().numpy()
                if best is None or (inertia < best[1] and not _is_same_clustering(labels, best[0], K)):
                    best = (labels, inertia, C.cpu().numpy(), n_iter)
            labels, inertia, centres, n_iter = best
            if len(np.unique(labels)) < K:
                warnings.warn(f"Number of distinct clusters ({len(np.unique(labels))}) found smaller than n_clusters ({K}). Possibly "
                              "due to duplicate points in X.", ConvergenceWarning)
            self.cluster_centers_ = centres + R.mean[None, :]
            self.labels_ = labels.astype(np.int32)
            self.inertia_ = float(inertia)
            self.n_iter_ = int(n_iter)
            self.n_features_in_ = d
            self._tol = tol_
        return self

    def fit(self, X, y=None, sample_weight=None):
        return self._fit(X, sample_weight)

    def fit_predict(self, X, y=None, sample_weight=None):
        return self._fit(X, sample_weight).labels_

    def fit_transform(self, X, y=None, sample_weight=None):
        return self._fit(X, sample_weight).transform(X)

    def _assigned(self, X, want_D=False):
        """the assignment of new rows to the fitted centres -> (labels, D [n, K] of squared distances or None, inertia)"""
        if not hasattr(self, "cluster_centers_"):
            raise RuntimeError("This KMeans instance is not fitted yet. Call 'fit' first.")
        x = self._rows(X, False)
        dev = _km_device_of(x)
        centres = np.asarray(self.cluster_centers_, np.float64)
        with torch.cuda.device(dev):
            xt = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            R = _Centred(xt, centres.shape[0], dev)
            it = _Lloyd(R, fitting=False)
            C = torch.from_numpy(np.ascontiguousarray(centres - R.mean[None, :])).to(dev)
            D = torch.empty(R.n, R.K, **R.f64) if want_D else None
            it.assign(C, label=it.label[0], D=D, part=it.ipart)
            return it.label[0].cpu().numpy(), (D.cpu().numpy() if want_D else None), it.inertia()

    def predict(self, X):
        return self._assigned(X)[0]

    def transform(self, X):
        """distances [n, K] to the centres: the correctly rounded sqrt of the squared distances"""
        return np.sqrt(self._assigned(X, want_D=True)[1])

    def score(self, X, y=None, sample_weight=None):
        if sample_weight is not None:
            raise ValueError("sample_weight is not supported: only unit weights")
        return -self._assigned(X)[2]


@_check_model_exists
def kmeans(latents, n_clusters=25, random_state=None):
    """KMeans(n_clusters, random_state=random_state) fitted to the latents -> (k_pred, model), cached as gmm() caches:
    {path}{label}_kmeans.p and .npy"""
    return KMeans(n_clusters=n_clusters, random_state=random_state).fit(latents)
