"""Latent decodability metrics of train() (reference: src/scrubvae/eval/metrics.py:231-329): cross-validated decoders of a
variable from the latents, on the device.

    linear_rand_cv(z, y_true, window=51, folds=5)     R^2 of least squares (sklearn LinearRegression + r2_score)
    mlp_rand_cv(z, y_true, window=51, folds=5)        R^2 of the 200-step AdamW MLP of train_MLP
    log_class_rand_cv(z, y_true, window=51, folds=5)  accuracy of elastic-net one-vs-rest logistic regression
    qda_rand_cv(z, y_true, window=51, folds=5)        accuracy of QuadraticDiscriminantAnalysis()

    lda_rand_cv(z, y_true, window=51, folds=5)        accuracy of LinearDiscriminantAnalysis()
    knn_class_rand_cv(z, y_true, window=51, folds=5, n_neighbors=5)   accuracy of KNeighborsClassifier(n_neighbors)
    knn_reg_rand_cv(z, y_true, window=51, folds=5, n_neighbors=5)     R^2 of KNeighborsRegressor(n_neighbors)

Each returns a list of `folds` floats in fold order, as the reference's `rand_cv` wrapper does: rows z[0::window], then
KFold(n_splits=folds, shuffle=True, random_state=100), restated here in numpy (this module does not import sklearn).  After the
downsample every pass over the rows, every factorisation and every solver iteration runs in csrc/decode.hip (fp64) or, for the
MLP, on the fp32 GEMM kernels; the results come back to the host once per call (the MLP's first call at a new size above the
GEMM autotune threshold also times its tiles once).  Class labels are read on the host first
(the class set and the row order by class are host decisions).

Differences from the reference, by design:
  - log_class_rand_cv solves each (fold, class) problem to its optimum (KKT residual <= 1e-8 of the gradient at w = 0) with a
    deterministic proximal Newton method; the reference's `saga` is randomised and stops at max_iter = 300, possibly short of it.
    A problem that does not converge within the iteration cap raises a ConvergenceWarning.
  - a latent direction with (numerically) zero variance in a training fold -- a constant or duplicated column -- gets coefficient 0
    (svae_spd_factor_solve_f64); for least squares this gives the predictions of sklearn's minimum-norm solution, for QDA the
    direction is left out of the class density (sklearn divides by its zero variance).
  - log_class_rand_cv fits, per fold, the classes present in that fold's training rows (sklearn's classes_); a class absent
    there is never predicted in that fold.
  - lda_rand_cv raises the ValueErrors of qda_rand_cv, also for a class with a single training row (sklearn's LDA accepts one).
Limits (ValueError): z_dim <= 128, <= 8 regression targets, <= 64 classes, <= 10 folds.
The two kNN probes are non-parametric: the rows go to fp64 and one exact neighbour search (csrc/knn.hip, eval/neighbors.py) with
group = fold gives every row its n_neighbors nearest training rows of its fold; uniform weights, a tied vote goes to the lowest
class, the regression mean is summed in neighbour order.  Their limits are those of kneighbors, not the ones above.

The rest of the reference's eval/metrics.py:

    mmd_estimate(X, Y, h=None)   maximum mean discrepancy of two sets of rows, squared-exponential kernel (metrics.py:332-374)
    mmd_bandwidth(X, Y)          the h that mmd_estimate uses when h is None: the squared median of all pairwise distances
    mmd_permutation_test(X, Y, h=None, n_permutations=1000, seed=0, permutations=None)
                                 is that statistic distinguishable from zero: its permutation null and p-value (not in the
                                 reference, which stops at the number)
    mmd_permutations(n, n_permutations, seed, device)   the relabellings mmd_permutation_test draws by default
    hungarian_match(x1, x2)      x1 relabelled with the labels of x2 that a maximum-weight assignment pairs them with (host)
    shannon_entropy(x)           natural-log entropy of the label histogram (host)

mmd_* take numpy arrays or torch tensors, host or device, any float dtype; the rows go to fp64 uncentred and everything runs in
csrc/mmd.hip: the distances in scipy's pdist / cdist arithmetic, the median as an exact order statistic (mmd_bandwidth is
bit-equal to the reference's np.median(...) ** 2), nothing of size n^2 stored, results bit-reproducible.  The sums are taken in
a different order from numpy's, so mmd_estimate agrees with the reference to a few units of roundoff of kxx + kyy + 2 kxy.
mmd_permutation_test recomputes the statistic under P relabellings of the pooled rows in csrc/mmd_null.hip: the kernel values do
not depend on the labels, so all P statistics are one product of the kernel matrix, generated tile by tile, with the n x P matrix
of 0 / 1 labels on the fp64 matrix cores -- one all-pairs pass per 256 permutations instead of one per permutation.  The median
bandwidth depends on the pooled distances only, so h=None costs one select.  pvalue = (1 + #{T_p >= T_0}) / (1 + P).
Differences from the reference, by design:
  - mmd_*: ValueError for nx < 2 or ny < 2 (the reference returns nan with a numpy warning), for differing feature counts, for
    non-finite rows and for an h that is not a finite positive number.  h is None with a zero median (more than half of all pairs
    coincide) follows the arithmetic, -0 / 0: the result is nan, as in the reference.
  - hungarian_match solves the assignment with its own rectangular Jonker-Volgenant solver (scipy is not a dependency); where
    several assignments share the maximum, any of them is correct and the pick may differ from scipy's.
  - the reference's shannon_entropy_torch is broken (it multiplies by x, not by the histogram) and unused: left out.
"""
from __future__ import annotations

import functools
import warnings

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _clock
from ._inputs import _finite_rows, _is_number
from ._permutation import MMD_MAX_PERMUTATIONS, _given_or_count, _on_device_or_drawn, _pvalue, mmd_permutations  # noqa: F401
from .neighbors import _knn_check, _knn_device

_RTOL_PIVOT = 1e-12   # svae_spd_factor_solve_f64: pivots <= this x max diagonal are zero directions
LOGREG_C, LOGREG_L1_RATIO = 1.0, 0.5
LOGREG_TOL = 1e-8     # KKT residual relative to max |gradient at w = 0|
LOGREG_MAX_ITER = 60  # proximal Newton iterations
LOGREG_MAX_SWEEPS = 500
MLP_STEPS, MLP_LR, MLP_BETAS, MLP_EPS, MLP_WD = 200, 1e-3, (0.9, 0.999), 1e-8, 0.01


class ConvergenceWarning(UserWarning):
    """A logistic regression problem stopped at the iteration cap above its KKT tolerance (sklearn's ConvergenceWarning)."""


def kfold_assign(n, folds):
    """fold index of each of n rows under KFold(n_splits=folds, shuffle=True, random_state=100)."""
    folds = int(folds)
    if folds < 2:
        raise ValueError(f"k-fold cross-validation requires at least 2 folds, got {folds}")
    if n < folds:
        raise ValueError(f"Cannot have number of splits n_splits={folds} greater than the number of samples: n_samples={n}.")
    idx = np.arange(n)
    np.random.RandomState(100).shuffle(idx)
    sizes = np.full(folds, n // folds, dtype=np.int64)
    sizes[: n % folds] += 1
    fold = np.empty(n, dtype=np.int64)
    start = 0
    for f, s in enumerate(sizes):
        fold[idx[start: start + s]] = f
        start += s
    return fold


_device_of = functools.partial(_device._device_of, who="the decodability metrics run on the GPU (csrc/decode.hip); no device is available")


def _rows(z, window, device):
    """z[0::window] as a contiguous fp32 [n, d] device tensor."""
    t = z if torch.is_tensor(z) else torch.from_numpy(np.asarray(z))
    t = t[0::window]
    if t.dim() != 2:
        t = t.reshape(t.shape[0], -1)
    return t.to(device=device, dtype=torch.float32).contiguous()


def _host(y, window):
    a = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    return a[0::window]


def _check_dims(n, d, folds, ny=0, k=0):
    if d > _lib.CV_MAX_DIM:
        raise ValueError(f"z_dim {d} > {_lib.CV_MAX_DIM}")
    if ny > _lib.CV_MAX_TARGETS:
        raise ValueError(f"{ny} regression targets > {_lib.CV_MAX_TARGETS}")
    if k > _lib.CV_MAX_CLASSES:
        raise ValueError(f"{k} classes > {_lib.CV_MAX_CLASSES}")
    if folds > _lib.CV_MAX_FOLDS:
        raise ValueError(f"{folds} folds > {_lib.CV_MAX_FOLDS}")


def _i32(a, device):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(device)


class _Rows:
    """Downsampled rows sorted by group (fold-major), their fold segments and the centred fp64 matrix A of csrc/decode.hip."""

    def __init__(self, x, fold, cls, K, y, device):
        n, d = x.shape
        self.n, self.d, self.K, self.device = n, d, K, device
        group = fold * K + cls
        self.perm = np.argsort(group, kind="stable")
        self.fold, self.cls = fold[self.perm], cls[self.perm]
        F = int(fold.max()) + 1
        self.folds = F
        gcount = np.bincount(group, minlength=F * K)
        self.ghi = np.cumsum(gcount)
        self.glo = self.ghi - gcount
        self.flo, self.fhi = self.glo[0::K], self.ghi[K - 1::K]
        self.ny = 0 if y is None else y.shape[1]
        self.lda = ops.pad16(d + 1 + self.ny)
        self.perm_d = _i32(self.perm, device)
        self.mean = torch.empty(d + self.ny, dtype=torch.float64, device=device)
        self.A = torch.empty(n, self.lda, dtype=torch.float64, device=device)
        check(_lib.lib().svae_cv_center(x.data_ptr(), d, d, None if y is None else y.data_ptr(), self.ny, self.ny, self.perm_d.data_ptr(),
                                        n, self.mean.data_ptr(), self.A.data_ptr(), self.lda, ops._stream()), "cv_center")
        self.fold_d, self.cls_d = _i32(self.fold, device), _i32(self.cls, device)
        self.flo_d, self.fhi_d = _i32(self.flo, device), _i32(self.fhi, device)
        self.max_fold = int((self.fhi - self.flo).max())

    def moments(self, D, lo, hi, w=None, ldw=0, skip=None, out=None):
        G = len(lo) if not torch.is_tensor(lo) else lo.numel()
        lo_d = lo if torch.is_tensor(lo) else _i32(lo, self.device)
        hi_d = hi if torch.is_tensor(hi) else _i32(hi, self.device)
        if out is None:
            out = torch.empty(G, D, D, dtype=torch.float64, device=self.device)
        check(_lib.lib().svae_cv_moments(self.A.data_ptr(), self.lda, D, lo_d.data_ptr(), hi_d.data_ptr(), G, ops._p(w), ldw, ops._p(skip),
                                         out.data_ptr(), D, ops._stream()), "cv_moments")
        return out


def spd_factor_solve(M, B=None, rtol=_RTOL_PIVOT):
    """Batched rank-revealing Cholesky (csrc/decode.hip) of fp64 device matrices M [b, n, n] (n <= 128): (L, logdet, rank, X) with
    X = M^-1 B for B [b, n, nrhs] (nrhs <= 8), pivots <= rtol * max diag treated as zero directions (coefficient 0)."""
    M = M.contiguous()
    b, n = M.shape[0], M.shape[1]
    L = torch.empty_like(M)
    logdet = torch.empty(b, dtype=torch.float64, device=M.device)
    rank = torch.empty(b, dtype=torch.int32, device=M.device)
    X, nrhs = None, 0
    if B is not None:
        B = B.contiguous()
        nrhs = B.shape[2]
        X = torch.empty_like(B)
    check(_lib.lib().svae_spd_factor_solve_f64(M.data_ptr(), n, n * n, n, b, ops._p(B), nrhs, n * nrhs, L.data_ptr(), ops._p(X),
                                               logdet.data_ptr(), rank.data_ptr(), rtol, ops._stream()), "spd_factor_solve_f64")
    return L, logdet, rank, X


def _train_blocks(M, F, K=1):
    """per (fold, class) moment blocks of the training folds: (sum over folds of the class) - (the fold's own block), fp64"""
    M = M.view(F, K, *M.shape[1:])
    tot = M[0].clone()
    for f in range(1, F):
        tot += M[f]
    return tot.unsqueeze(0) - M


def _r2_from_stats(st):
    """sklearn r2_score(multioutput="uniform_average", force_finite=True) per fold from stats [F, ny, 4]"""
    out = []
    for f in range(st.shape[0]):
        r2 = []
        for o in range(st.shape[1]):
            ss_res, sy, syy, m = st[f, o]
            ss_tot = max(syy - sy * sy / m, 0.0)
            if ss_tot <= 1e-13 * max(syy, 1e-300):  # a constant target: the exact zero of sklearn's two-pass sum
                r2.append(1.0 if ss_res == 0.0 else 0.0)
            else:
                r2.append(1.0 - ss_res / ss_tot)
        out.append(float(np.mean(r2)))
    return out


def _targets(y_true, window, device):
    y = _host(y_true, window).astype(np.float32)
    if y.ndim == 1:
        y = y[:, None]
    return torch.from_numpy(np.ascontiguousarray(y.reshape(y.shape[0], -1))).to(device)


def linear_rand_cv(z, y_true, window=51, folds=5):
    """R^2 per fold of least squares with intercept (reference metrics.py:264-269)."""
    dev = _device_of(z)
    with torch.cuda.device(dev):
        x = _rows(z, window, dev)
        y = _targets(y_true, window, dev)
        n, d = x.shape
        ny = y.shape[1]
        _check_dims(n, d, folds, ny=ny)
        fold = kfold_assign(n, folds)
        R = _Rows(x, fold, np.zeros(n, dtype=np.int64), 1, y, dev)
        D = d + 1 + ny
        T = _train_blocks(R.moments(D, R.flo, R.fhi), R.folds)[:, 0]
        cnt = T[:, d, d]
        sx, sy = T[:, :d, d], T[:, d, d + 1:]
        cxx = T[:, :d, :d] - sx[:, :, None] * sx[:, None, :] / cnt[:, None, None]
        cxy = T[:, :d, d + 1:] - sx[:, :, None] * sy[:, None, :] / cnt[:, None, None]
        _, _, _, beta = spd_factor_solve(cxx, cxy)
        xbar, ybar = sx / cnt[:, None], sy / cnt[:, None]
        c0 = (ybar - torch.einsum("fi,fio->fo", xbar, beta)).contiguous()
        stats = torch.empty(R.folds, ny, 4, dtype=torch.float64, device=dev)
        check(_lib.lib().svae_cv_r2_stats(R.A.data_ptr(), R.lda, d, ny, R.flo_d.data_ptr(), R.fhi_d.data_ptr(), R.folds, beta.data_ptr(),
                                          c0.data_ptr(), None, 0, None, stats.data_ptr(), ops._stream()), "cv_r2_stats")
        return _r2_from_stats(stats.cpu().numpy())


def _labels(y_true, window):
    y = _host(y_true, window).reshape(-1)
    classes, cls = np.unique(y, return_inverse=True)
    return classes, cls.astype(np.int64)


def _qda(z, y_true, window, folds, want_rows=False):
    dev = _device_of(z)
    with torch.cuda.device(dev):
        x = _rows(z, window, dev)
        n, d = x.shape
        classes, cls = _labels(y_true, window)
        K = len(classes)
        _check_dims(n, d, folds, k=K)
        if K < 2:
            raise ValueError(f"The number of classes has to be greater than one; got {K} class")
        fold = kfold_assign(n, folds)
        R = _Rows(x, fold, cls, K, None, dev)
        F = R.folds
        cnt_fc = (R.ghi - R.glo).reshape(F, K)
        train_cnt = cnt_fc.sum(0)[None, :] - cnt_fc
        if (train_cnt == 1).any():
            f, c = np.argwhere(train_cnt == 1)[0]
            raise ValueError(f"y has only 1 sample in class {classes[c]} (training set of fold {f}), covariance is ill defined.")
        if ((train_cnt > 0).sum(1) < 2).any():
            raise ValueError("a training fold holds fewer than two classes")
        D = d + 1
        T = _train_blocks(R.moments(D, R.glo, R.ghi), F, K).reshape(F * K, D, D)
        cnt = T[:, d, d].clamp(min=2.0)
        sx = T[:, :d, d]
        mu = (sx / cnt[:, None]).contiguous()
        cov = (T[:, :d, :d] - sx[:, :, None] * sx[:, None, :] / cnt[:, None, None]) / (cnt - 1.0)[:, None, None]
        absent = torch.as_tensor((train_cnt == 0).reshape(-1), device=dev)
        cov[absent] = torch.eye(d, dtype=torch.float64, device=dev)
        L, logdet, _, _ = spd_factor_solve(cov)
        with np.errstate(divide="ignore"):
            logprior = np.log(train_cnt / train_cnt.sum(1, keepdims=True)).reshape(-1)
        cst = (torch.as_tensor(logprior, device=dev) - 0.5 * logdet).contiguous()
        correct = torch.zeros(F, dtype=torch.int32, device=dev)
        pred = torch.empty(n, dtype=torch.int32, device=dev) if want_rows else None
        gap = torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None
        check(_lib.lib().svae_cv_qda_score(R.A.data_ptr(), R.lda, d, K, R.flo_d.data_ptr(), R.fhi_d.data_ptr(), F, R.max_fold,
                                           mu.data_ptr(), L.data_ptr(), d, cst.data_ptr(), R.cls_d.data_ptr(), correct.data_ptr(),
                                           ops._p(pred), ops._p(gap), ops._stream()), "cv_qda_score")
        acc = [float(c) / float(m) for c, m in zip(correct.cpu().numpy(), R.fhi - R.flo)]
        if not want_rows:
            return acc
        out = dict(acc=acc, perm=R.perm, fold=R.fold, pred=np.empty(n, np.int64), gap=np.empty(n))
        out["pred"][R.perm] = classes[pred.cpu().numpy()]
        out["gap"][R.perm] = gap.cpu().numpy()
        return out


def qda_rand_cv(z, y_true, window=51, folds=5):
    """Accuracy per fold of QuadraticDiscriminantAnalysis() (reference metrics.py:287-292)."""
    return _qda(z, y_true, window, folds)


def _lda(z, y_true, window, folds, want_rows=False):
    dev = _device_of(z)
    with torch.cuda.device(dev):
        x = _rows(z, window, dev)
        n, d = x.shape
        classes, cls = _labels(y_true, window)
        K = len(classes)
        _check_dims(n, d, folds, k=K)
        if K < 2:
            raise ValueError(f"The number of classes has to be greater than one; got {K} class")
        fold = kfold_assign(n, folds)
        R = _Rows(x, fold, cls, K, None, dev)
        F = R.folds
        cnt_fc = (R.ghi - R.glo).reshape(F, K)
        train_cnt = cnt_fc.sum(0)[None, :] - cnt_fc
        if (train_cnt == 1).any():
            f, c = np.argwhere(train_cnt == 1)[0]
            raise ValueError(f"y has only 1 sample in class {classes[c]} (training set of fold {f}), covariance is ill defined.")
        if ((train_cnt > 0).sum(1) < 2).any():
            raise ValueError("a training fold holds fewer than two classes")
        D = d + 1
        T = _train_blocks(R.moments(D, R.glo, R.ghi), F, K).reshape(F * K, D, D)
        cnt = T[:, d, d].clamp(min=2.0)
        sx = T[:, :d, d]
        mu = (sx / cnt[:, None]).contiguous()
        # pooled within-class scatter of each training fold over n_train - (classes present); an absent class adds zeros
        scatter = (T[:, :d, :d] - sx[:, :, None] * sx[:, None, :] / cnt[:, None, None]).view(F, K, d, d)
        pooled = scatter[:, 0].clone()
        for c in range(1, K):
            pooled += scatter[:, c]
        dof = train_cnt.sum(1) - (train_cnt > 0).sum(1)
        if (dof < 1).any():
            raise ValueError("a training fold holds no more rows than classes")
        cov = pooled / torch.as_tensor(dof, dtype=torch.float64, device=dev)[:, None, None]
        L, _, _, _ = spd_factor_solve(cov)
        LK = L[:, None].expand(F, K, d, d).contiguous()  # one factor per fold: its logdet is the same for every class and drops out
        with np.errstate(divide="ignore"):
            logprior = np.log(train_cnt / train_cnt.sum(1, keepdims=True)).reshape(-1)
        cst = torch.as_tensor(logprior, device=dev).contiguous()
        correct = torch.zeros(F, dtype=torch.int32, device=dev)
        pred = torch.empty(n, dtype=torch.int32, device=dev) if want_rows else None
        gap = torch.empty(n, dtype=torch.float64, device=dev) if want_rows else None
        check(_lib.lib().svae_cv_qda_score(R.A.data_ptr(), R.lda, d, K, R.flo_d.data_ptr(), R.fhi_d.data_ptr(), F, R.max_fold,
                                           mu.data_ptr(), LK.data_ptr(), d, cst.data_ptr(), R.cls_d.data_ptr(), correct.data_ptr(),
                                           ops._p(pred), ops._p(gap), ops._stream()), "cv_qda_score")
        acc = [float(c) / float(m) for c, m in zip(correct.cpu().numpy(), R.fhi - R.flo)]
        if not want_rows:
            return acc
        out = dict(acc=acc, perm=R.perm, fold=R.fold, pred=np.empty(n, np.int64), gap=np.empty(n))
        out["pred"][R.perm] = classes[pred.cpu().numpy()]
        out["gap"][R.perm] = gap.cpu().numpy()
        return out


def lda_rand_cv(z, y_true, window=51, folds=5):
    """Accuracy per fold of LinearDiscriminantAnalysis() (reference metrics.py:293-298): the class means and one pooled covariance
    per training fold (within-class scatter over n_train - classes), priors = the class frequencies."""
    return _lda(z, y_true, window, folds)


def _knn_cv_check(z, window, folds, n_neighbors):
    """the argument errors of the kNN probes -> (the rows z[0::window] in fp64, their folds, k, the folds as int32 groups)"""
    t = (z if torch.is_tensor(z) else np.asarray(z))[0::window]
    if t.ndim != 2:
        t = t.reshape(t.shape[0], -1)
    fold = kfold_assign(t.shape[0], folds)
    x, k, grp = _knn_check(t, n_neighbors, fold)
    return x, fold, k, grp


def _knn_cv_search(x, k, grp):
    """each row's k nearest rows of the other folds, int64 [n, k] on the device: ONE neighbour search with group = fold"""
    return _knn_device(x, k, grp)[1].long()


def _knn_class(z, y_true, window, folds, n_neighbors, want_rows=False):
    x, fold, k, grp = _knn_cv_check(z, window, folds, n_neighbors)
    n = x.shape[0]
    classes, cls = _labels(y_true, window)
    if len(cls) != n:
        raise ValueError(f"y_true gives {len(cls)} rows after the downsample, z gives {n}")
    K = len(classes)
    idx = _knn_cv_search(x, k, grp)
    cls_d = torch.from_numpy(cls).to(idx.device)
    votes = torch.zeros(n, K, dtype=torch.int64, device=idx.device)
    votes.scatter_add_(1, cls_d[idx], torch.ones_like(idx))
    # one integer key per (votes, class): its maximum is unique, the most votes and then the lowest class
    pred = (votes * K + (K - 1 - torch.arange(K, device=idx.device))[None, :]).argmax(1).cpu().numpy()
    hit = pred == cls
    acc = [float(hit[fold == f].sum()) / float((fold == f).sum()) for f in range(int(folds))]
    return dict(acc=acc, fold=fold, pred=classes[pred]) if want_rows else acc


def knn_class_rand_cv(z, y_true, window=51, folds=5, n_neighbors=5):
    """Accuracy per fold of KNeighborsClassifier(n_neighbors) with uniform weights, fitted on the other folds: the majority vote
    of the row's n_neighbors nearest training rows, a tied vote to the lowest class in np.unique order (sklearn's rule)."""
    return _knn_class(z, y_true, window, folds, n_neighbors)


def _knn_r2(y, pred):
    """sklearn's r2_score(y, pred) for [m, outputs] fp64 arrays: 1 - SS_res / SS_tot per output (for a constant target 1 where
    the fit is exact, else 0), averaged uniformly"""
    ss_res = ((y - pred) ** 2).sum(0)
    ss_tot = ((y - y.mean(0)) ** 2).sum(0)
    r2 = np.where(ss_tot != 0, 1.0 - ss_res / np.where(ss_tot != 0, ss_tot, 1.0), np.where(ss_res == 0, 1.0, 0.0))
    return float(r2.mean())


def _knn_reg(z, y_true, window, folds, n_neighbors, want_rows=False):
    x, fold, k, grp = _knn_cv_check(z, window, folds, n_neighbors)
    n = x.shape[0]
    y = _host(y_true, window).astype(np.float64)
    y = y.reshape(y.shape[0], -1)
    if y.shape[0] != n:
        raise ValueError(f"y_true gives {y.shape[0]} rows after the downsample, z gives {n}")
    if not np.isfinite(y).all():
        raise ValueError("y_true holds non-finite values")
    idx = _knn_cv_search(x, k, grp)
    yd = torch.from_numpy(np.ascontiguousarray(y)).to(idx.device)
    acc = yd[idx[:, 0]]
    for t in range(1, k):  # in neighbour order, every addition rounded on its own
        acc = acc + yd[idx[:, t]]
    pred = acc.cpu().numpy() / k  # on the host: the device's division by a scalar multiplies by its rounded reciprocal
    r2 = [_knn_r2(y[fold == f], pred[fold == f]) for f in range(int(folds))]
    return dict(r2=r2, fold=fold, pred=pred) if want_rows else r2


def knn_reg_rand_cv(z, y_true, window=51, folds=5, n_neighbors=5):
    """R^2 per fold of KNeighborsRegressor(n_neighbors) fitted on the other folds: the fp64 mean of the targets of the row's
    n_neighbors nearest training rows, summed in neighbour order; r2_score's uniform average over the outputs."""
    return _knn_reg(z, y_true, window, folds, n_neighbors)


def logreg_problems(cnt_fc):
    """The one-vs-rest problems sklearn fits on each training fold, from the per-(fold, class) row counts [F, K]: the classes
    present in the fold's training rows; two present classes make one binary problem with the second one positive.  Returns
    (pfold [P], pos [P] class index, pstart [F + 1], neg [F]: the negative class of a binary fold, else -1)."""
    F, K = cnt_fc.shape
    train = cnt_fc.sum(0)[None, :] - cnt_fc
    pfold, pos, pstart, neg = [], [], [0], []
    for f in range(F):
        present = np.nonzero(train[f] > 0)[0]
        if len(present) < 2:
            raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the training rows of fold {f} "
                             f"contain {len(present)} class(es)")
        use = present[1:] if len(present) == 2 else present
        pfold += [f] * len(use)
        pos += list(use)
        pstart.append(len(pos))
        neg.append(int(present[0]) if len(present) == 2 else -1)
    return np.array(pfold), np.array(pos), np.array(pstart), np.array(neg)


def _logreg(z, y_true, window, folds, want_rows=False):
    dev = _device_of(z)
    with torch.cuda.device(dev):
        x = _rows(z, window, dev)
        n, d = x.shape
        classes, cls = _labels(y_true, window)
        K = len(classes)
        _check_dims(n, d, folds, k=K)
        if K < 2:
            raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the data contains only one class: {classes}")
        fold = kfold_assign(n, folds)
        R = _Rows(x, fold, cls, K, None, dev)
        F = R.folds
        pf, ps, pstart_h, neg_h = logreg_problems((R.ghi - R.glo).reshape(F, K))
        P = len(pf)
        pfold, pos = _i32(pf, dev), _i32(ps, dev)
        pstart, neg = _i32(pstart_h, dev), _i32(neg_h, dev)
        D = d + 1
        L = _lib.lib()
        st = ops._stream()
        chunks = L.svae_logreg_chunks(n)
        f64 = dict(dtype=torch.float64, device=dev)
        W = torch.zeros(P, D, **f64)
        dirn = torch.zeros(P, D, **f64)
        f0, delta, kkt = (torch.zeros(P, **f64) for _ in range(3))
        g0 = torch.full((P,), -1.0, **f64)
        done = torch.zeros(P, dtype=torch.int32, device=dev)
        iters = torch.zeros(P, dtype=torch.int32, device=dev)
        part = torch.empty(P * chunks * max(D + 1, 12), **f64)
        hw = torch.empty(P, n, **f64)
        H = torch.empty(P, D, D, **f64)
        lo_all, hi_all = _i32(np.zeros(P), dev), _i32(np.full(P, n), dev)
        C, rho = LOGREG_C, LOGREG_L1_RATIO
        alpha = 1.0 - rho
        prob = (R.A.data_ptr(), R.lda, D, n, R.fold_d.data_ptr(), R.cls_d.data_ptr(), pfold.data_ptr(), pos.data_ptr(), P)
        state = (W.data_ptr(), dirn.data_ptr(), f0.data_ptr(), delta.data_ptr(), kkt.data_ptr(), g0.data_ptr(), done.data_ptr(),
                 iters.data_ptr())
        for it in range(LOGREG_MAX_ITER + 1):
            last = it == LOGREG_MAX_ITER
            check(L.svae_logreg_stats(*prob, W.data_ptr(), C, done.data_ptr(), part.data_ptr(), hw.data_ptr(), st), "logreg_stats")
            if not last:
                R.moments(D, lo_all, hi_all, w=hw, ldw=n, skip=done, out=H)
            check(L.svae_logreg_newton(*prob, part.data_ptr(), H.data_ptr(), *state, alpha, rho, LOGREG_TOL, int(last), LOGREG_MAX_SWEEPS,
                                       st), "logreg_newton")
            if last:
                break
            check(L.svae_logreg_line_search(*prob, W.data_ptr(), dirn.data_ptr(), f0.data_ptr(), delta.data_ptr(), done.data_ptr(),
                                            iters.data_ptr(), C, alpha, rho, part.data_ptr(), st), "logreg_line_search")
        correct = torch.zeros(F, dtype=torch.int32, device=dev)
        pred = torch.empty(n, dtype=torch.int32, device=dev) if want_rows else None
        check(L.svae_logreg_score(*prob, W.data_ptr(), pstart.data_ptr(), neg.data_ptr(), R.flo_d.data_ptr(), R.fhi_d.data_ptr(), F, R.max_fold, correct.data_ptr(),
                                  ops._p(pred), st), "logreg_score")
        res = torch.cat([correct.double(), kkt, g0]).cpu().numpy()
        correct_h, kkt_h, g0_h = res[:F], res[F:F + P], res[F + P:]
        bad = np.nonzero(kkt_h > LOGREG_TOL * g0_h)[0]
        if len(bad):
            warnings.warn(f"log_class_rand_cv: {len(bad)} of {P} logistic problems stopped at {LOGREG_MAX_ITER} iterations with a KKT "
                          f"residual up to {float((kkt_h[bad] / np.maximum(g0_h[bad], 1e-300)).max()):.2e} of the initial gradient",
                          ConvergenceWarning)
        acc = [float(c) / float(m) for c, m in zip(correct_h, R.fhi - R.flo)]
        if not want_rows:
            return acc
        Wh = W.cpu().numpy()
        mean = R.mean.cpu().numpy()
        coef = Wh[:, :d]
        intercept = Wh[:, d] - Wh[:, :d] @ mean  # back to raw (uncentred) latents
        out = dict(acc=acc, coef=coef, intercept=intercept, pfold=pf, pos=classes[ps], pstart=pstart_h, kkt=kkt_h, g0=g0_h,
                   iters=iters.cpu().numpy(), classes=classes, fold=fold, pred=np.empty(n, np.int64))
        out["pred"][R.perm] = classes[pred.cpu().numpy()]
        return out


def log_class_rand_cv(z, y_true, window=51, folds=5):
    """Accuracy per fold of LogisticRegression(penalty="elasticnet", l1_ratio=0.5, multi_class="ovr", C=1) at its optimum
    (reference metrics.py:272-284)."""
    return _logreg(z, y_true, window, folds)


_MLP_CONVS = {}


def _linear_conv(device, rows, c_in, c_out):
    """fp32 Linear geometry of the MLP decoder, one per (device, rows, c_in, c_out) for the process: a size above the autotune
    threshold times its tiles on its first call only, later calls reuse the choice (the fp32 kernels' results do not depend on the
    tile: include/scrubvae_hip.h, svae_conv_desc.tile)."""
    key = (device.index, rows, c_in, c_out)
    cv = _MLP_CONVS.get(key)
    if cv is None:
        cv = _MLP_CONVS[key] = ops.Conv(rows, 1, c_in, c_out, 1, pieces=0)
    return cv


def mlp_init(d, ny):
    """Initial weights of the reference's MLP(d, ny) (model/disentangle.py:568-580): three nn.Linear drawn in order from torch's
    global generator -> list of (weight [out, in], bias [out])."""
    lins = [torch.nn.Linear(d, d), torch.nn.Linear(d, d), torch.nn.Linear(d, ny)]
    return [(l.weight.detach().clone(), l.bias.detach().clone()) for l in lins]


def mlp_rand_cv(z, y_true, window=51, folds=5, init=None):
    """R^2 per fold of train_MLP (reference metrics.py:295-329): MLP(d, ny) = Linear-ReLU-Linear-ReLU-Linear, AdamW(lr 1e-3,
    weight_decay 0.01), 200 full-batch steps on MSELoss(reduction="sum") over the training rows, fp32 on the GEMM kernels.
    The initial weights are drawn fold by fold as the reference does (mlp_init); `init` (a list of `folds` mlp_init results)
    overrides them."""
    dev = _device_of(z)
    with torch.cuda.device(dev):
        x = _rows(z, window, dev)
        y = _targets(y_true, window, dev)
        n, d = x.shape
        ny = y.shape[1]
        _check_dims(n, d, folds, ny=ny)
        fold = kfold_assign(n, folds)
        if init is None:
            init = [mlp_init(d, ny) for _ in range(folds)]
        R = _Rows(x, fold, np.zeros(n, dtype=np.int64), 1, y, dev)
        F = R.folds
        dp, op = ops.pad16(d), ops.pad16(ny)
        xs = torch.zeros(n, dp, device=dev)
        xs[:, :d] = x[torch.as_tensor(R.perm, device=dev)]
        ys = y[torch.as_tensor(R.perm, device=dev)].contiguous()
        dims = [(d, d), (d, d), (d, ny)]
        convs = [_linear_conv(dev, n, i, o) for i, o in dims]
        sizes = [(cv.c_in_p * cv.c_out_p, cv.c_out_p) for cv in convs]
        total = sum(a + b for a, b in sizes)
        pre = [torch.zeros(n, cv.c_out_p, device=dev) for cv in convs]
        act = [torch.zeros(n, dp, device=dev) for _ in range(2)]
        gbuf = [torch.zeros(n, dp, device=dev) for _ in range(2)]
        dout = torch.zeros(n, op, device=dev)
        ws = torch.empty(max(cv.wgrad_workspace_bytes() for cv in convs) // 4 + 64, device=dev)
        outs = []
        mfold = torch.zeros(1, dtype=torch.int32, device=dev)
        ptrs = torch.tensor([pre[2].data_ptr(), dout.data_ptr()], dtype=torch.int64, device=dev)
        for f in range(F):
            p = torch.zeros(total, device=dev)
            g, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
            views, gviews, off = [], [], 0
            for (nw, nb), cv, (wt, bt) in zip(sizes, convs, init[f]):
                w_, b_ = p[off: off + nw].view(1, cv.c_in_p, cv.c_out_p), p[off + nw: off + nw + nb]
                gw, gb = g[off: off + nw].view(1, cv.c_in_p, cv.c_out_p), g[off + nw: off + nw + nb]
                w_[0, : wt.shape[1], : wt.shape[0]] = wt.t().to(dev, torch.float32)
                b_[: bt.shape[0]] = bt.to(dev, torch.float32)
                views.append((w_, b_))
                gviews.append((gw, gb))
                off += nw + nb
            hyper = torch.tensor([MLP_LR, 0.0, 0.0, 0.0], device=dev)
            mfold.fill_(f)
            for _ in range(MLP_STEPS):
                h = xs
                for li in range(3):
                    convs[li].fwd(h, views[li][0], views[li][1], pre[li])
                    if li < 2:
                        ops.relu_fwd(pre[li], act[li])
                        h = act[li]
                check(_lib.lib().svae_cv_mse_grad(ptrs[0:1].data_ptr(), ptrs[1:2].data_ptr(), 1, mfold.data_ptr(), ys.data_ptr(), ny, ny,
                                                  op, R.fold_d.data_ptr(), n, ops._stream()), "cv_mse_grad")
                gy = dout
                for li in (2, 1, 0):
                    xin = xs if li == 0 else act[li - 1]
                    convs[li].wgrad(xin, gy, gviews[li][0], gviews[li][1], ws)
                    if li > 0:
                        convs[li].dgrad(gy, views[li][0], gbuf[li - 1])
                        ops.relu_bwd(gbuf[li - 1], act[li - 1], gbuf[li - 1])
                        gy = gbuf[li - 1]
                ops.adam_advance(hyper, *MLP_BETAS)
                ops.adam_step_dev(p, g, m, v, hyper, MLP_BETAS[0], MLP_BETAS[1], MLP_EPS, MLP_WD, True)
            h = xs
            for li in range(3):
                convs[li].fwd(h, views[li][0], views[li][1], pre[li])
                if li < 2:
                    ops.relu_fwd(pre[li], act[li])
                    h = act[li]
            outs.append(pre[2].clone())
        optr = torch.tensor([o.data_ptr() for o in outs], dtype=torch.int64, device=dev)
        stats = torch.empty(F, ny, 4, dtype=torch.float64, device=dev)
        ymean = R.mean[d:].contiguous()
        check(_lib.lib().svae_cv_r2_stats(R.A.data_ptr(), R.lda, d, ny, R.flo_d.data_ptr(), R.fhi_d.data_ptr(), F, None, None,
                                          optr.data_ptr(), op, ymean.data_ptr(), stats.data_ptr(), ops._stream()), "cv_r2_stats")
        return _r2_from_stats(stats.cpu().numpy())


def cluster_entropy(k_preds0, k_preds1, n_components):
    """Mean per-cluster Shannon entropy (bits) of a reference clustering k_preds0 within each cluster i < n_components of
    k_preds1 (the inner loop of the reference's epoch_cluster_entropy, metrics.py:133-145): the histogram of k_preds0 over the rows
    with k_preds1 == i, bins np.arange(k_preds0.max() + 2) - 0.5, normalised by the cluster size; an empty cluster adds 0."""
    k0, k1 = np.asarray(k_preds0).reshape(-1), np.asarray(k_preds1).reshape(-1)
    bins = np.arange(k0.max() + 2) - 0.5
    entropy = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n_components):
            sel = k1 == i
            hist = np.histogram(k0[sel], bins=bins)[0] / sel.sum()
            entropy += np.nan_to_num(hist * np.log2(1 / hist)).sum()
    return float(entropy / n_components)


def shannon_entropy(x):
    """Natural-log Shannon entropy of the histogram of the labels x (reference metrics.py:377-381)."""
    counts = np.unique(np.asarray(x), return_counts=True)[1]
    hist = counts / counts.sum()
    return (hist * np.log(1 / hist)).sum()


def _contingency(x1, x2):
    """counts [len(np.unique(x1)), len(np.unique(x2))] of the label pairs: what pandas.crosstab(x1, x2) holds"""
    k1, i1 = np.unique(x1, return_inverse=True)
    k2, i2 = np.unique(x2, return_inverse=True)
    table = np.zeros((len(k1), len(k2)), dtype=np.int64)
    np.add.at(table, (i1.reshape(-1), i2.reshape(-1)), 1)
    return k1, k2, table


def max_weight_assignment(weight):
    """(row_ind, col_ind) of a maximum-weight assignment of min(rows, cols) pairs of a rectangular table, rows ascending: what
    scipy's linear_sum_assignment(weight, maximize=True) solves.  Shortest augmenting paths with potentials (Jonker-Volgenant),
    O(rows^2 cols); exact for integer tables.  Ties between optimal assignments are broken by the search order."""
    w = np.asarray(weight, dtype=np.float64)
    if w.ndim != 2:
        raise ValueError(f"expected a 2-D table, got {w.ndim}-D")
    if not np.isfinite(w).all():
        raise ValueError("the table holds non-finite entries")
    flip = w.shape[0] > w.shape[1]
    cost = -(w.T if flip else w)  # rows <= columns: every row is assigned
    nr, nc = cost.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col_of, row_of = np.full(nr, -1), np.full(nc, -1)
    for r in range(nr):
        dist = np.full(nc, np.inf)        # shortest alternating path from row r to each column, in reduced costs
        path = np.full(nc, -1)            # the row before each column on that path
        in_rows, in_cols = np.zeros(nr, dtype=bool), np.zeros(nc, dtype=bool)
        i, low, sink = r, 0.0, -1
        while sink < 0:
            in_rows[i] = True
            red = low + cost[i] - u[i] - v
            better = ~in_cols & (red < dist)
            dist[better] = red[better]
            path[better] = i
            j = int(np.argmin(np.where(in_cols, np.inf, dist)))
            low = dist[j]
            in_cols[j] = True
            if row_of[j] < 0:
                sink = j
            else:
                i = row_of[j]
        others = in_rows.copy()
        others[r] = False
        u[r] += low
        u[others] += low - dist[col_of[others]]
        v[in_cols] -= low - dist[in_cols]
        j = sink
        while True:  # augment along the path
            i = path[j]
            row_of[j] = i
            col_of[i], j = j, col_of[i]
            if i == r:
                break
    rows, cols = np.arange(nr), col_of
    if flip:
        rows, cols = cols, rows
    order = np.argsort(rows, kind="stable")
    return rows[order], cols[order]


def hungarian_match(x1, x2):
    """x1 with each label replaced by the label of x2 it is matched to (reference metrics.py:388-412): the contingency table of
    the two sequences (rows np.unique(x1), columns np.unique(x2)), a maximum-weight assignment on it (max_weight_assignment;
    where several share the maximum, any of them is correct), then the reference's relabelling with its quirks: labels of x1 left
    unmatched (more row labels than column labels) stay as they are, and a search index past the matched labels is read as 0."""
    x1, x2 = np.asarray(x1), np.asarray(x2)
    k1, k2, table = _contingency(x1, x2)
    row_ind, col_ind = max_weight_assignment(table)
    row_k, col_v = k1[row_ind], k2[col_ind]
    idx = np.searchsorted(row_k, x1)
    idx[idx == len(row_k)] = 0
    mask = row_k[idx] == x1
    return np.where(mask, col_v[idx], x1)


_MMD_CALLS = {"select": 0, "sums": 0, "null": 0}  # launches of svae_mmd_select / svae_mmd_sums / svae_mmd_null by this process


def _mmd_check(X, Y, h):
    """the argument errors of mmd_*, before any device work -> the fp64 rows (x, y)"""
    x, y = _finite_rows(X, "X"), _finite_rows(Y, "Y")
    nx, ny = x.shape[0], y.shape[0]
    if nx < 2 or ny < 2:
        raise ValueError(f"the MMD estimate needs at least 2 rows on each side, got {nx} and {ny}")
    if x.shape[1] != y.shape[1] or x.shape[1] < 1:
        raise ValueError(f"X and Y must share one feature count >= 1, got {x.shape[1]} and {y.shape[1]}")
    if h is not None and (not _is_number(h) or not h > 0):
        raise ValueError(f"h must be a finite positive number, got {h!r}")
    return x, y


def _mmd_device(X, Y, h, want_h, info=None, keep=None):
    """(h, [kxx, kyy, kxy, mmd]) on the device of X (or of Y, or the current one); want_h: stop after the bandwidth ([...] is None).
    info (a dict) receives med and the synchronised host-clock times select_s and sums_s; keep (a dict) receives the device
    tensors Z (the stacked fp64 rows) and hm (med, h)."""
    x, y = _mmd_check(X, Y, h)
    nx, ny = x.shape[0], y.shape[0]
    n, d = nx + ny, x.shape[1]
    dev = _device_of(x, y)
    with torch.cuda.device(dev):
        lib = _lib.lib()
        blocks = lib.svae_mmd_blocks(n)
        Z = torch.cat([(a if torch.is_tensor(a) else torch.from_numpy(a)).to(dev) for a in (x, y)]).contiguous()
        st = ops._stream()
        hm = torch.full((2,), float("nan") if h is None else float(h), dtype=torch.float64, device=dev)  # med, h

        clock = functools.partial(_clock, dev, info is not None)
        t0 = clock()
        if h is None:
            work = torch.empty(_lib.MMD_WORK_WORDS, dtype=torch.int64, device=dev)
            _MMD_CALLS["select"] += 1
            check(lib.svae_mmd_select(Z.data_ptr(), d, d, n, work.data_ptr(), hm.data_ptr(), st), "mmd_select")
        t1 = clock()
        out = None
        if not want_h:
            part = torch.empty(3 * blocks, dtype=torch.float64, device=dev)
            out = torch.empty(4, dtype=torch.float64, device=dev)
            _MMD_CALLS["sums"] += 1
            check(lib.svae_mmd_sums(Z.data_ptr(), d, d, n, nx, hm[1:].data_ptr(), part.data_ptr(), out.data_ptr(), st), "mmd_sums")
        t2 = clock()
        if keep is not None:
            keep.update(Z=Z, hm=hm)
        res = (hm if out is None else torch.cat([hm, out])).cpu().numpy()
        if info is not None:
            info.update(med=float(res[0]) if h is None else None, select_s=t1 - t0, sums_s=t2 - t1)
        return float(res[1]), (None if out is None else res[2:])


def mmd_bandwidth(X, Y):
    """The bandwidth mmd_estimate(X, Y) uses: np.median of the pairwise distances inside X, inside Y and across, squared --
    bit-equal to the reference's inline recipe (metrics.py:364-369)."""
    return _mmd_device(X, Y, None, True)[0]


def mmd_estimate(X, Y, h=None):
    """Estimate of the maximum mean discrepancy between the distributions X [nx, d] and Y [ny, d] were drawn from, with the kernel
    exp(-|a - b|^2 / h) (reference metrics.py:332-374; Gretton et al. 2012): mean kernel value over the pairs inside X, plus that
    inside Y, minus twice that across.  h defaults to mmd_bandwidth(X, Y)."""
    return float(_mmd_device(X, Y, h, False)[1][3])


_MMD_NULL_LAUNCH = 1024                   # permutations per svae_mmd_null launch: bounds the partials and the label scratch


class MMDPermutationResult:
    """statistic (float), pvalue (float), null_distribution (numpy [P] fp64) and h (float): scipy's permutation_test names."""
    __slots__ = ("statistic", "pvalue", "null_distribution", "h")

    def __init__(self, statistic, pvalue, null_distribution, h):
        self.statistic, self.pvalue, self.null_distribution, self.h = statistic, pvalue, null_distribution, h

    def __repr__(self):
        return (f"MMDPermutationResult(statistic={self.statistic!r}, pvalue={self.pvalue!r}, "
                f"null_distribution=<{len(self.null_distribution)} values>, h={self.h!r})")


def _mmd_label_bits(perms, nx):
    """perms [P, n] int64 (torch, any device) -> [n, ceil(P / 64)] int64 whose bit (p & 63) of word p >> 6 in row j is 1 when j is
    among perms[p, :nx] (the rows relabelled "X"); the bits past P are 0.  The layout svae_mmd_null reads."""
    P, n = perms.shape
    words = (P + 63) // 64
    member = torch.zeros(words * 64, n, dtype=torch.int64, device=perms.device)
    member[:P].scatter_(1, perms[:, :nx], 1)
    weight = torch.tensor([1 << k for k in range(63)] + [-(1 << 63)], dtype=torch.int64, device=perms.device)  # bit 63: the sign
    return (member.view(words, 64, n) * weight.view(1, 64, 1)).sum(1).t().contiguous()


def _mmd_null_device(Z, hm, nx, perms, info=None):
    """T_p [P] fp64 on the device of Z (the stacked fp64 rows, the first nx of them X) for the checked relabellings perms [P, n]
    (int64, same device), hm = (med, h) on the device.  info (a dict) receives the synchronised host-clock times pack_s (label
    bits) and null_s (the svae_mmd_null launches)."""
    dev = Z.device
    n, d = Z.shape
    P = perms.shape[0]
    lib = _lib.lib()
    st = ops._stream()
    null = torch.empty(P, dtype=torch.float64, device=dev)
    work = torch.empty(lib.svae_mmd_null_blocks(n, min(P, _MMD_NULL_LAUNCH)), dtype=torch.float64, device=dev)
    pack_s = null_s = 0.0

    clock = functools.partial(_clock, dev, info is not None)
    for p0 in range(0, P, _MMD_NULL_LAUNCH):
        count = min(_MMD_NULL_LAUNCH, P - p0)
        t0 = clock()
        bits = _mmd_label_bits(perms[p0: p0 + count], nx)
        t1 = clock()
        _MMD_CALLS["null"] += 1
        check(lib.svae_mmd_null(Z.data_ptr(), d, d, n, nx, hm[1:].data_ptr(), bits.data_ptr(), bits.shape[1], count, work.data_ptr(),
                                null[p0:].data_ptr(), st), "mmd_null")
        t2 = clock()
        pack_s, null_s = pack_s + (t1 - t0), null_s + (t2 - t1)
    if info is not None:
        info.update(pack_s=pack_s, null_s=null_s)
    return null


def mmd_permutation_test(X, Y, h=None, n_permutations=1000, seed=0, permutations=None):
    """Permutation test of the hypothesis that X [nx, d] and Y [ny, d] come from one distribution, with mmd_estimate(X, Y, h) as
    the statistic (the kernel two-sample test of Gretton et al. 2012) -> MMDPermutationResult.

    statistic is mmd_estimate(X, Y, h), bit for bit.  null_distribution[p] is the same estimator after relabelling p of the pooled
    rows Z = [X; Y]: the rows permutations[p, :nx] of Z become X, the rest Y.  pvalue = (1 + #{p: null[p] >= statistic}) / (1 + P),
    compared in fp64.  h defaults to mmd_bandwidth(X, Y), which no relabelling changes; with a zero median the statistic, the
    p-value and the null are nan, as in mmd_estimate.

    permutations: [P, n] integers, numpy or torch; every row must be a permutation of range(n) (ValueError otherwise; the rows
    are checked on the device before the null is computed).  When it is None, P = n_permutations rows are drawn by
    mmd_permutations(n, n_permutations, seed, device): the result equals the call with those permutations bit for bit.
    1 <= P <= MMD_MAX_PERMUTATIONS = 65 536.  Inputs and argument errors otherwise as for mmd_estimate."""
    x, y = _mmd_check(X, Y, h)
    nx, n, d = x.shape[0], x.shape[0] + y.shape[0], x.shape[1]
    perms, P = _given_or_count(permutations, n_permutations, n)
    dev = _device_of(x, y)
    with torch.cuda.device(dev):
        perms = _on_device_or_drawn(perms, n, P, seed, dev)
        keep = {}
        hv, out = _mmd_device(x, y, h, False, keep=keep)
        null = _mmd_null_device(keep["Z"], keep["hm"], nx, perms).cpu().numpy()
    statistic = float(out[3])
    return MMDPermutationResult(statistic, _pvalue(statistic, null), null, hv)
