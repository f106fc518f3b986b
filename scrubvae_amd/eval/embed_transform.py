"""Place new latents into a fitted two-dimensional t-SNE map, on the device (csrc/tsne.hip, csrc/knn.hip).

    TSNEMap(z_ref, embedding, *, perplexity=30.0)      the reference rows [n, d] and their map [n, 2]
    TSNEMap.from_fit(tsne, z)                          from a fitted eval.TSNE and the rows it was fitted on
        .transform(z_new, *, max_iter=250, learning_rate=0.1, momentum=0.8, exaggeration=1.0, max_grad_norm=0.25,
                   init="weighted", batch_rows=1 << 18, info=None)  ->  [m, 2] float64 numpy
        kl_rows_ [m], grad_norm_rows_ [m], neighbors_ [m, k] after a transform
    tsne_transform(z_ref, embedding, z_new, *, perplexity=30.0, **kw)      TSNEMap(...).transform(z_new, **kw)

A map is fitted on a subsample (the exact gradient of eval.TSNE costs n^2 per iteration); this puts the rest of the recording,
another animal, or another model's latents of the same windows on it.  The map itself never moves, and the new rows do not see
each other: every new row is a 2-D optimisation of its own in the field of the n fixed map points (openTSNE's `transform`).

1. Neighbours: the k = min(n, floor(3 perplexity)) nearest reference rows of every new row (svae_knn_cross: no row left out).
2. Perplexity search on dist * dist (svae_tsne_search): the conditional P_e|i of row i over its k neighbours.  It is not
   symmetrised; each row sums to 1.
3. init="weighted": y_i = sum_e P_ie Yref[idx_ie], added in neighbour order; an [m, 2] array is used as given.
4. max_iter iterations, the count fixed, of
     svae_tsne_cross_repulsion:  R_i = sum_j q q (y_i - yref_j), rowq_i = sum_j q over all n map points, q = 1 / (1 + |y_i - yref_j|^2);
     svae_tsne_place_step:       g_i = 2 (exaggeration A_i - R_i / rowq_i), A_i the attraction of the k neighbours; |g_i| clipped to
                                 max_grad_norm (0: no clip); sklearn's gains; update = momentum update - learning_rate g; y_i += update.
   At exaggeration 1 g_i is the exact gradient of the row's objective sum_e P_ie log(P_ie / q_e|i), q_e|i = q_ie / rowq_i.
5. One more evaluation at the returned positions, at exaggeration 1 and without the clip: kl_rows_ (that objective) and
   grad_norm_rows_ (|g_i|).

The rows go through in batches of batch_rows to bound memory (the repulsion's work is 3 x chunks x batch_rows doubles).  Rows are
independent and the repulsion picks its column split from n alone, so neither the batch size nor the order or number of the new
rows changes a bit of any row's result.  Inside a batch there is no device-to-host read between the first and the last launch;
every launch is a plain launch on the current stream.  ValueError, before any device work, for every argument out of range and for
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
from ._inputs import _feature_rows, _finite_rows, _is_int, _is_number
from .embed import _search_device, _tsne_neighbors
from .neighbors import _knn_cross_device

_MAX_ROWS = 2 ** 26          # rows of the map, and rows of a batch (svae_tsne_cross_repulsion)
# launches and device-to-host reads by this process
_PLACE_CALLS = {"knn": 0, "search": 0, "repulsion": 0, "step": 0, "host_reads": 0}
# of the last transform: doubles of repulsion work and column chunks of a batch, the batches made, and per host read the
# (launches of its batch made before it, launches of the whole batch)
_PLACE_LAST = {"work": 0, "chunks": 0, "batches": 0, "reads_at": []}

_device_of = functools.partial(_device._device_of, who="the t-SNE map runs on the GPU (csrc/tsne.hip); no device is available")


def _number(v, name, ok, want):
    if not _is_number(v) or not ok(v):
        raise ValueError(f"{name} must be {want}, got {v!r}")
    return float(v)


def _integer(v, name, least):
    if not _is_int(v) or v < least:
        raise ValueError(f"{name} must be an integer >= {least}, got {v!r}")
    return int(v)


def _plane(a, rows, name):
    """an [rows, 2] array of finite numbers -> float64 numpy"""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.shape != (rows, 2):
        raise ValueError(f"{name} must be [{rows}, 2], got shape {tuple(a.shape)}")
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{name} must hold numbers, got {a.dtype}")
    a = np.array(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"{name} holds non-finite values")
    return a


class _CrossRepulsion:
    """the buffers of svae_tsne_cross_repulsion for m queries against a map of n points on one device"""

    def __init__(self, m, Yref, chunks=0):
        lib = _lib.lib()
        self.m, self.Yref, self.chunks = m, Yref, chunks
        words = lib.svae_tsne_cross_repulsion_work(m, Yref.shape[0], chunks)
        if words <= 0:
            raise ValueError(f"svae_tsne_cross_repulsion does not take m = {m}, n = {Yref.shape[0]}, chunks = {chunks}")
        self.work = torch.empty(words, dtype=torch.float64, device=Yref.device)
        self.R = torch.empty(m, 2, dtype=torch.float64, device=Yref.device)
        self.rowq = torch.empty(m, dtype=torch.float64, device=Yref.device)
        _PLACE_LAST.update(work=words, chunks=words // (3 * (-(-m // 256) * 256)))

    def __call__(self, Y):
        _PLACE_CALLS["repulsion"] += 1
        check(_lib.lib().svae_tsne_cross_repulsion(Y.data_ptr(), self.m, self.Yref.data_ptr(), self.Yref.shape[0], self.chunks,
                                                   self.work.data_ptr(), self.R.data_ptr(), self.rowq.data_ptr(), ops._stream()),
              "tsne_cross_repulsion")


def _place_step(idx, P, exag, Y, rep, update, gains, momentum, lr, max_grad_norm, klrow, gradsq):
    _PLACE_CALLS["step"] += 1
    check(_lib.lib().svae_tsne_place_step(idx.data_ptr(), P.data_ptr(), idx.shape[1], float(exag), Y.data_ptr(), rep.Yref.data_ptr(),
                                          rep.R.data_ptr(), rep.rowq.data_ptr(), ops._p(update), ops._p(gains), float(momentum), float(lr),
                                          float(max_grad_norm), Y.shape[0], ops._p(klrow), ops._p(gradsq), ops._stream()), "tsne_place_step")


def _weighted_init(idx, P, Yref):
    """y_i = sum_e P_ie Yref[idx_ie], every product and every addition rounded on its own, in neighbour order"""
    Y = torch.zeros(idx.shape[0], 2, dtype=torch.float64, device=Yref.device)
    for e in range(idx.shape[1]):
        Y = Y + P[:, e:e + 1] * Yref[idx[:, e].long()]
    return Y


class TSNEMap:
    """A fitted map: the reference rows z_ref [n, d] and their embedding [n, 2] (module docstring).  They go to the device at the
    first transform and stay there."""

    def __init__(self, z_ref, embedding, *, perplexity=30.0):
        x = _feature_rows(z_ref, "z_ref")
        n = x.shape[0]
        if n < 1:
            raise ValueError("z_ref must have at least one row")
        if n > _MAX_ROWS:
            raise ValueError(f"at most 2^26 reference rows are supported, got {n}")
        _tsne_neighbors(n, perplexity)                                # its errors; the row count here is n, not n - 1
        self.n_neighbors_ = min(n, int(math.floor(3.0 * perplexity)))
        self.perplexity = perplexity
        self._x = x
        self._y = _plane(embedding, n, "embedding")
        self._dev = None

    @classmethod
    def from_fit(cls, tsne, z):
        """the map of a fitted eval.TSNE and the rows z it was fitted on"""
        if getattr(tsne, "embedding_", None) is None:
            raise ValueError("from_fit needs a fitted TSNE (no embedding_)")
        return cls(z, tsne.embedding_, perplexity=tsne.perplexity)

    def _check(self, z_new, max_iter, learning_rate, momentum, exaggeration, max_grad_norm, init, batch_rows):
        q = _finite_rows(z_new, "z_new")
        m = q.shape[0]
        if q.shape[1] != self._x.shape[1]:
            raise ValueError(f"z_new has {q.shape[1]} features, the map's rows have {self._x.shape[1]}")
        if m < 1:
            raise ValueError("z_new must have at least one row")
        max_iter = _integer(max_iter, "max_iter", 0)
        lr = _number(learning_rate, "learning_rate", lambda v: v > 0, "a positive number")
        momentum = _number(momentum, "momentum", lambda v: 0 <= v < 1, "a number in [0, 1)")
        exag = _number(exaggeration, "exaggeration", lambda v: v >= 1, "a number >= 1")
        clip = _number(max_grad_norm, "max_grad_norm", lambda v: v >= 0, "a number >= 0 (0: no clip)")
        batch_rows = min(_integer(batch_rows, "batch_rows", 1), _MAX_ROWS)
        if isinstance(init, str):
            if init != "weighted":
                raise ValueError(f"'init' must be 'weighted' or an [m, 2] array, got {init!r}")
        else:
            init = _plane(init, m, "an init array")
        return q, max_iter, lr, momentum, exag, clip, init, batch_rows

    def _device(self, q):
        """(X [n, d], Yref [n, 2]) on the device of the first transform's rows (or the current one)"""
        if self._dev is None:
            dev = _device_of(q, self._x)
            with torch.cuda.device(dev):
                self._dev = (_on_device(self._x, dev), torch.from_numpy(self._y).to(dev).contiguous())
        return self._dev

    def transform(self, z_new, *, max_iter=250, learning_rate=0.1, momentum=0.8, exaggeration=1.0, max_grad_norm=0.25, init="weighted",
                  batch_rows=1 << 18, info=None):
        """The positions [m, 2] of the rows of z_new on the map.  info (a dict) receives the synchronised host-clock times knn_s,
        search_s, repulsion_s and step_s, summed over the batches."""
        q, max_iter, lr, momentum, exag, clip, init, batch_rows = self._check(z_new, max_iter, learning_rate, momentum, exaggeration,
                                                                              max_grad_norm, init, batch_rows)
        X, Yref = self._device(q)
        dev, m, k, timed = X.device, q.shape[0], self.n_neighbors_, info is not None
        out = np.empty((m, 2)), np.empty(m), np.empty(m), np.empty((m, k), dtype=np.int64)
        t = dict(knn_s=0.0, search_s=0.0, repulsion_s=0.0, step_s=0.0)
        _PLACE_LAST.update(batches=0, reads_at=[])
        with torch.cuda.device(dev):
            for b0 in range(0, m, batch_rows):
                b1 = min(m, b0 + batch_rows)
                rows = b1 - b0
                Q = _on_device(q[b0:b1], dev)
                Y0 = None if isinstance(init, str) else torch.from_numpy(init[b0:b1]).to(dev).contiguous()
                rep = _CrossRepulsion(rows, Yref)
                update = torch.zeros(rows, 2, dtype=torch.float64, device=dev)
                gains = torch.ones(rows, 2, dtype=torch.float64, device=dev)
                klrow = torch.empty(rows, dtype=torch.float64, device=dev)
                gradsq = torch.empty(rows, dtype=torch.float64, device=dev)
                before = sum(_PLACE_CALLS[c] for c in ("knn", "search", "repulsion", "step"))
                c0 = _clock(dev, timed)
                _PLACE_CALLS["knn"] += 1
                dist, idx = _knn_cross_device(X, Q, k)
                c1 = _clock(dev, timed)
                _PLACE_CALLS["search"] += 1
                P, _ = _search_device(dist * dist, self.perplexity)
                c2 = _clock(dev, timed)
                Y = _weighted_init(idx, P, Yref) if Y0 is None else Y0
                for _ in range(max_iter):
                    s0 = _clock(dev, timed)
                    rep(Y)
                    s1 = _clock(dev, timed)
                    _place_step(idx, P, exag, Y, rep, update, gains, momentum, lr, clip, None, None)
                    if timed:
                        t["repulsion_s"] += s1 - s0
                        t["step_s"] += _clock(dev) - s1
                rep(Y)
                _place_step(idx, P, 1.0, Y, rep, None, None, 0.0, 0.0, 0.0, klrow, gradsq)
                made = sum(_PLACE_CALLS[c] for c in ("knn", "search", "repulsion", "step")) - before
                _PLACE_CALLS["host_reads"] += 1
                _PLACE_LAST["reads_at"].append((made, 2 + 2 * (max_iter + 1)))
                _PLACE_LAST["batches"] += 1
                out[0][b0:b1] = Y.cpu().numpy()
                out[1][b0:b1] = klrow.cpu().numpy()
                out[2][b0:b1] = torch.sqrt(gradsq).cpu().numpy()
                out[3][b0:b1] = idx.cpu().numpy()
                t["knn_s"] += c1 - c0
                t["search_s"] += c2 - c1
        self.kl_rows_, self.grad_norm_rows_, self.neighbors_ = out[1], out[2], out[3]
        if timed:
            info.update(t, iterations=max_iter, batches=_PLACE_LAST["batches"])
        return out[0]


def tsne_transform(z_ref, embedding, z_new, *, perplexity=30.0, **kw):
    """TSNEMap(z_ref, embedding, perplexity=perplexity).transform(z_new, **kw): the [m, 2] float64 positions of the new rows"""
    return TSNEMap(z_ref, embedding, perplexity=perplexity).transform(z_new, **kw)
