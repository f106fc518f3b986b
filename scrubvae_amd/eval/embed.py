"""Two-dimensional t-SNE embedding of the latents on their exact kNN graph, on the device (csrc/tsne.hip, csrc/knn.hip).

    TSNE(n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
         n_iter_without_progress=300, min_grad_norm=1e-7, init="pca", random_state=None)
        .fit(z) / .fit_transform(z); embedding_ [n, 2] float64 numpy, kl_divergence_, n_iter_, learning_rate_
    tsne(z, **kw)                              TSNE(**kw).fit_transform(z)
    tsne_affinities(z, perplexity=30.0)        (P scipy.sparse.csr_matrix [n, n] that sums to 1, beta [n] float64)

z is [n, d], numpy or torch, host or device, any float dtype; the rows go to fp64 uncentred, as for the other eval modules.  The
embedding is what the reference's plot.scatter_cmap(data, hue, ...) takes as `data`.

This is sklearn 1.7's TSNE (its names and meanings) with an exact gradient instead of the Barnes-Hut tree:

1. Neighbours: k = min(n - 1, floor(3 perplexity)) exact nearest neighbours of every row (eval.neighbors), squared distances
   dist * dist.  This is van der Maaten's 3 x perplexity; sklearn takes int(3 perplexity + 1) = 91 at the default, one more than
   the kNN kernel holds (KNN_MAX_K = 90), so perplexity = 30.0 is the largest round value allowed.
2. Perplexity search per row: the loop of sklearn's _binary_search_perplexity in fp64 (svae_tsne_search).
3. P = P + P^T divided by its own sum (taken in a fixed order), CSR on the device with ascending columns.
4. init="pca": the first two principal components of z, each signed so that its largest-magnitude loading is positive, divided by
   the standard deviation of the first and multiplied by 1e-4; "random": 1e-4 RandomState(random_state).standard_normal((n, 2));
   an [n, 2] array is used as given.
5. sklearn's _gradient_descent schedule: 250 iterations with P * early_exaggeration, momentum 0.5 and a no-progress window of
   250, the rest with P, momentum 0.8 and n_iter_without_progress; gains + 0.2 where update * grad < 0, x 0.8 elsewhere, floor
   0.01; update and gains start afresh in the second phase; learning_rate="auto" is max(n / early_exaggeration / 4, 50).  Every 50
   iterations the KL value and the norm of the gained gradient come to the host for the two stopping rules; there is no other
   host round trip, and every launch is a plain launch on the current stream.  The gradient of row i is
   4 (exag A_i - R_i / Z): A_i the attraction over the row's CSR entries (svae_tsne_step), R_i and Z the repulsion over all n^2
   pairs (svae_tsne_repulsion).  KL = sum p log(p (1 + |y_i - y_j|^2)) + (sum p) log Z with the exaggerated p while it applies
   (sum p = early_exaggeration then), as sklearn reports it.

Differences from sklearn, by design: method / angle / metric / n_jobs do not exist (the gradient is exact, the metric Euclidean);
n_components must be 2; kl_divergence_ is evaluated once more at embedding_ itself (sklearn reports the value from before the
last update); results are bit-reproducible.  ValueError, before any device work, for every argument out of range and for
non-finite rows."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _clock, _on_device
from ._inputs import _feature_rows, _is_int, _is_number
from .neighbors import KNN_MAX_K, _knn_device

_EXPLORATION_ITER = 250      # iterations with early exaggeration (sklearn's _EXPLORATION_MAX_ITER)
_N_ITER_CHECK = 50           # iterations between two looks at the KL value and the gradient norm (sklearn's _N_ITER_CHECK)
_TSNE_CALLS = {"search": 0, "repulsion": 0, "step": 0, "sums": 0, "host_reads": 0}  # launches / device-to-host reads by this process
_TSNE_LAST = {"work": 0, "chunks": 0, "kl_checks": []}  # doubles of repulsion work, column chunks, (iteration, KL) of the last fit

_device_of = functools.partial(_device._device_of, who="t-SNE runs on the GPU (csrc/tsne.hip); no device is available")


def _tsne_neighbors(n, perplexity):
    """the argument errors of the perplexity -> k"""
    if not _is_number(perplexity):
        raise ValueError(f"perplexity must be a finite number, got {perplexity!r}")
    if perplexity <= 0:
        raise ValueError(f"perplexity must be positive, got {perplexity}")
    k = int(math.floor(3.0 * perplexity))
    if k < 1:
        raise ValueError(f"perplexity = {perplexity} asks for floor(3 perplexity) = 0 neighbours")
    if k > KNN_MAX_K:
        raise ValueError(f"perplexity = {perplexity} asks for floor(3 perplexity) = {k} neighbours; at most KNN_MAX_K = {KNN_MAX_K} "
                         f"are supported (perplexity <= {KNN_MAX_K // 3})")
    if perplexity >= n:
        raise ValueError(f"perplexity ({perplexity}) must be less than n_samples ({n})")
    return min(n - 1, k)


def _tsne_rows(z):
    x = _feature_rows(z, "z")
    n = x.shape[0]
    if n < 2:
        raise ValueError(f"t-SNE needs at least 2 rows, got {n}")
    if n > 2 ** 26:
        raise ValueError(f"at most 2^26 rows are supported, got {n}")
    return x


def _tsne_schedule(max_iter, n_iter_without_progress, early_exaggeration):
    """sklearn's two calls of _gradient_descent: (first iteration, end, momentum, factor on P, no-progress window); the second
    starts one past the iteration at which the first one stopped"""
    return [dict(it=0, max_iter=_EXPLORATION_ITER, momentum=0.5, exag=float(early_exaggeration), window=_EXPLORATION_ITER),
            dict(it=None, max_iter=int(max_iter), momentum=0.8, exag=1.0, window=int(n_iter_without_progress))]


def _auto_learning_rate(n, early_exaggeration):
    return max(n / early_exaggeration / 4.0, 50.0)


def _pca_init(x):
    """x fp64 [n, d] torch, where it is -> [n, 2]: the first two principal components of x, each signed so that its
    largest-magnitude loading is positive, divided by the standard deviation of the first and multiplied by 1e-4.  The d x d
    scatter matrix is summed in row chunks with torch's reductions (fixed order) and decomposed on the host."""
    n, d = x.shape
    xc = x - x.mean(0, keepdim=True)
    C = torch.zeros(d, d, dtype=torch.float64, device=x.device)
    rows = max(1, (1 << 24) // (d * d))
    for r0 in range(0, n, rows):
        b = xc[r0:r0 + rows]
        C = C + (b[:, :, None] * b[:, None, :]).sum(0)
    w, V = np.linalg.eigh(C.cpu().numpy())
    V = V[:, np.argsort(-w, kind="stable")[:2]].T.copy()         # [2, d]: the loadings of the two largest
    top = np.abs(V).argmax(1)
    V *= np.sign(V[np.arange(2), top])[:, None]
    Vd = torch.from_numpy(V).to(x.device)
    Y = torch.stack([(xc * Vd[0]).sum(1), (xc * Vd[1]).sum(1)], 1)
    return Y / Y[:, 0].std(unbiased=False) * 1e-4


def _search_device(d2, perplexity):
    """(P [n, k], beta [n]) fp64 on the device of d2 [n, k]"""
    n, k = d2.shape
    P = torch.empty_like(d2)
    beta = torch.empty(n, dtype=torch.float64, device=d2.device)
    _TSNE_CALLS["search"] += 1
    check(_lib.lib().svae_tsne_search(d2.data_ptr(), k, n, float(perplexity), P.data_ptr(), beta.data_ptr(), ops._stream()), "tsne_search")
    return P, beta


def _sums_device(a, b=None, out=None):
    """out[0] = sum a, out[1] = sum b in the fixed order of svae_tsne_sums, on the device"""
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=a.device)
    _TSNE_CALLS["sums"] += 1
    check(_lib.lib().svae_tsne_sums(a.data_ptr(), ops._p(b), a.numel(), out.data_ptr(), ops._stream()), "tsne_sums")
    return out


def _affinities_device(x, k, perplexity, info=None):
    """(rowptr int32 [n + 1], col int32 [nnz], val fp64 [nnz], beta [n]) on the device: steps 1 to 3 of the module docstring"""
    dev = _device_of(x)
    n = x.shape[0]
    with torch.cuda.device(dev):
        t0 = _clock(dev, info is not None)
        dist, idx = _knn_device(x, k, None)
        P, beta = _search_device(dist * dist, perplexity)
        # P + P^T: every (row, column) key occurs at most twice, so the order in which the two values meet does not matter
        rows = torch.arange(n, device=dev, dtype=torch.int64)[:, None].expand(n, k).reshape(-1)
        cols = idx.reshape(-1).to(torch.int64)
        keys = torch.cat([rows * n + cols, cols * n + rows])
        keys, inv = torch.unique(keys, sorted=True, return_inverse=True)
        val = torch.zeros(keys.numel(), dtype=torch.float64, device=dev).index_add_(0, inv, torch.cat([P.reshape(-1), P.reshape(-1)]))
        total = _sums_device(val)[0]
        val = val / torch.clamp(total, min=np.finfo(np.float64).eps)
        row = torch.div(keys, n, rounding_mode="floor")
        col = (keys - row * n).to(torch.int32)
        rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
        if info is not None:
            info.update(graph_s=_clock(dev) - t0)
    return rowptr.to(torch.int32), col, val, beta


def tsne_affinities(z, perplexity=30.0):
    """(P, beta): the symmetrised joint probabilities of t-SNE on the exact k = min(n - 1, floor(3 perplexity)) neighbour graph as
    a scipy.sparse.csr_matrix [n, n] that sums to 1 (columns ascending within a row), and every row's precision beta [n] float64
    from the perplexity search."""
    from scipy.sparse import csr_matrix
    x = _tsne_rows(z)
    n = x.shape[0]
    k = _tsne_neighbors(n, perplexity)
    rowptr, col, val, beta = _affinities_device(x, k, perplexity)
    return csr_matrix((val.cpu().numpy(), col.cpu().numpy(), rowptr.cpu().numpy()), shape=(n, n)), beta.cpu().numpy()


class _Repulsion:
    """the buffers of svae_tsne_repulsion for n rows on one device"""

    def __init__(self, n, dev, chunks=0):
        lib = _lib.lib()
        self.n, self.chunks = n, chunks
        words = lib.svae_tsne_repulsion_work(n, chunks)
        if words <= 0:
            raise ValueError(f"svae_tsne_repulsion does not take n = {n}, chunks = {chunks}")
        self.work = torch.empty(words, dtype=torch.float64, device=dev)
        self.R = torch.empty(n, 2, dtype=torch.float64, device=dev)
        self.rowq = torch.empty(n, dtype=torch.float64, device=dev)
        self.stat = torch.empty(3, dtype=torch.float64, device=dev)   # Z, then the two sums of a check
        self.Z = self.stat[:1]
        _TSNE_LAST.update(work=words, chunks=words // (3 * (-(-n // 256) * 256)))

    def __call__(self, Y):
        _TSNE_CALLS["repulsion"] += 1
        check(_lib.lib().svae_tsne_repulsion(Y.data_ptr(), self.n, self.chunks, self.work.data_ptr(), self.R.data_ptr(), self.rowq.data_ptr(),
                                             self.Z.data_ptr(), ops._stream()), "tsne_repulsion")


def _step_device(graph, exag, Y, rep, update, gains, momentum, lr, klpart, gradsq):
    rowptr, col, val = graph
    _TSNE_CALLS["step"] += 1
    check(_lib.lib().svae_tsne_step(rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), float(exag), Y.data_ptr(), rep.R.data_ptr(),
                                    rep.Z.data_ptr(), ops._p(update), ops._p(gains), float(momentum), float(lr), Y.shape[0], ops._p(klpart),
                                    ops._p(gradsq), ops._stream()), "tsne_step")


def _read_check(rep, klpart, gradsq, exag):
    """(KL, gradient norm) on the host from one read of (Z, sum klpart, sum gradsq)"""
    _sums_device(klpart, gradsq, rep.stat[1:])
    _TSNE_CALLS["host_reads"] += 1
    Z, kl, gsq = rep.stat.cpu().tolist()
    return kl + exag * math.log(Z), math.sqrt(gsq)


def _descend(graph, Y, lr, phases, min_grad_norm, info=None):
    """sklearn's two _gradient_descent calls on the device; Y [n, 2] is updated in place -> (KL at the final Y, n_iter_)"""
    dev = Y.device
    n = Y.shape[0]
    rep = _Repulsion(n, dev)
    klpart = torch.empty(n, dtype=torch.float64, device=dev)
    gradsq = torch.empty(n, dtype=torch.float64, device=dev)
    checks = []
    it = -1                                  # the last iteration made, as sklearn's _gradient_descent returns it
    t_rep = t_step = 0.0
    for ph in phases:
        first = it + 1 if ph["it"] is None else ph["it"]
        it = first                           # a phase with nothing left to do returns where it was to start (max_iter = 250)
        update = torch.zeros_like(Y)
        gains = torch.ones_like(Y)
        best, best_iter = np.finfo(np.float64).max, first
        for i in range(first, ph["max_iter"]):
            it = i
            look = (i + 1) % _N_ITER_CHECK == 0
            t0 = _clock(dev, info is not None)
            rep(Y)
            t1 = _clock(dev, info is not None)
            _step_device(graph, ph["exag"], Y, rep, update, gains, ph["momentum"], lr, klpart if look else None, gradsq if look else None)
            if info is not None:
                t_rep, t_step = t_rep + (t1 - t0), t_step + (_clock(dev) - t1)
            if look:
                kl, gnorm = _read_check(rep, klpart, gradsq, ph["exag"])
                checks.append((i, kl))
                if kl < best:
                    best, best_iter = kl, i
                elif i - best_iter > ph["window"]:
                    break
                if gnorm <= min_grad_norm:
                    break
    rep(Y)
    _step_device(graph, 1.0, Y, rep, None, None, 0.0, 0.0, klpart, gradsq)
    kl, _ = _read_check(rep, klpart, gradsq, 1.0)
    _TSNE_LAST.update(kl_checks=checks)
    if info is not None:
        info.update(repulsion_s=t_rep, step_s=t_step, iterations=it + 1)
    return kl, it


class TSNE:
    """sklearn.manifold.TSNE's arguments and fitted attributes with an exact gradient on the device (module docstring);
    n_components must be 2."""

    def __init__(self, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, init="pca", random_state=None):
        self.n_components = n_components
        self.perplexity = perplexity
        self.early_exaggeration = early_exaggeration
        self.learning_rate = learning_rate
        self.max_iter = max_iter
        self.n_iter_without_progress = n_iter_without_progress
        self.min_grad_norm = min_grad_norm
        self.init = init
        self.random_state = random_state

    def _check(self, z):
        """the argument errors, before any device work -> (fp64 rows, k, init: "pca" or a float64 [n, 2] numpy array, lr)"""
        if self.n_components != 2:
            raise ValueError(f"n_components must be 2, got {self.n_components!r}")
        x = _tsne_rows(z)
        n, d = x.shape
        k = _tsne_neighbors(n, self.perplexity)
        if not _is_int(self.max_iter) or self.max_iter < _EXPLORATION_ITER:
            raise ValueError(f"max_iter must be an integer >= {_EXPLORATION_ITER}, got {self.max_iter!r}")
        if not isinstance(self.early_exaggeration, (int, float, np.integer, np.floating)) or not self.early_exaggeration >= 1 \
                or not math.isfinite(self.early_exaggeration):
            raise ValueError(f"early_exaggeration must be at least 1, got {self.early_exaggeration!r}")
        if not _is_int(self.n_iter_without_progress) or self.n_iter_without_progress < -1:
            raise ValueError(f"n_iter_without_progress must be an integer >= -1, got {self.n_iter_without_progress!r}")
        if not isinstance(self.min_grad_norm, (int, float, np.integer, np.floating)) or not self.min_grad_norm >= 0:
            raise ValueError(f"min_grad_norm must be a number >= 0, got {self.min_grad_norm!r}")
        if isinstance(self.learning_rate, str):
            if self.learning_rate != "auto":
                raise ValueError(f'learning_rate must be "auto" or a positive number, got {self.learning_rate!r}')
            lr = _auto_learning_rate(n, self.early_exaggeration)
        else:
            if not _is_number(self.learning_rate) or not self.learning_rate > 0:
                raise ValueError(f'learning_rate must be "auto" or a positive number, got {self.learning_rate!r}')
            lr = float(self.learning_rate)
        if isinstance(self.init, str):
            if self.init == "pca":
                if d < 2:
                    raise ValueError('init="pca" needs at least 2 features')
                init = "pca"
            elif self.init == "random":
                init = 1e-4 * np.random.RandomState(self.random_state).standard_normal((n, 2))
            else:
                raise ValueError(f"'init' must be 'pca', 'random', or an array, got {self.init!r}")
        else:
            init = self.init.detach().cpu().numpy() if torch.is_tensor(self.init) else np.asarray(self.init)
            if init.shape != (n, 2):
                raise ValueError(f"an init array must be [n, 2] = ({n}, 2), got shape {tuple(init.shape)}")
            if init.dtype.kind not in "fiu":
                raise ValueError(f"an init array must hold numbers, got {init.dtype}")
            init = np.array(init, dtype=np.float64)
            if not np.isfinite(init).all():
                raise ValueError("the init array holds non-finite values")
        return x, k, init, lr

    def fit(self, z, y=None, *, info=None):
        """info (a dict) receives the synchronised host-clock times graph_s, repulsion_s, step_s and the iteration count"""
        x, k, init, lr = self._check(z)
        dev = _device_of(x)
        with torch.cuda.device(dev):
            x = _on_device(x, dev)
            rowptr, col, val, _ = _affinities_device(x, k, self.perplexity, info)
            Y = (_pca_init(x) if isinstance(init, str) else torch.from_numpy(init).to(dev)).contiguous()
            phases = _tsne_schedule(self.max_iter, self.n_iter_without_progress, self.early_exaggeration)
            kl, it = _descend((rowptr, col, val), Y, lr, phases, self.min_grad_norm, info)
            self.embedding_ = Y.cpu().numpy()
        self.kl_divergence_ = kl
        self.n_iter_ = it
        self.learning_rate_ = lr
        self.n_features_in_ = x.shape[1]
        return self

    def fit_transform(self, z, y=None):
        return self.fit(z).embedding_


def tsne(z, **kw):
    """TSNE(**kw).fit_transform(z): the [n, 2] float64 embedding"""
    return TSNE(**kw).fit_transform(z)
