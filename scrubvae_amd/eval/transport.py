"""Entropic optimal transport between two sets of latents, on the device (csrc/ot.hip): how two sets differ geometrically, and
which region of one corresponds to which region of the other, when the sets hold different rows.

    sinkhorn(X, Y, *, epsilon=None, cost="sqeuclidean", a=None, b=None, scaling=0.5, tol=1e-6, max_iter=1000, check_every=10)
        -> SinkhornResult: value, transport_cost, f, g, epsilon, n_iter, marginal_error, converged and the methods
           apply(V), barycentric_map(), apply_transposed(V), barycentric_map_transposed(), flow(labels_y)
    sinkhorn_divergence(X, Y, **the same)   -> SinkhornDivergence(value, ot_xy, ot_xx, ot_yy, cross)
    transport_flow(result, labels_x, labels_y) -> (ids_x, ids_y, mass [Kx, Ky])

X [nx, d] and Y [ny, d] are numpy or torch, host or device, float32 or float64; the rows go to fp64 uncentred, as for mmd_*.  The
cost is c_ij = |x_i - y_j|^2 ("sqeuclidean") or |x_i - y_j| ("euclidean") in the arithmetic of csrc/pair_tiles.h; a and b are
positive weights that sum to 1 (default uniform).  Nothing of size nx x ny is stored: every pass regenerates the cost tile by tile.

The solve is Sinkhorn's in the log domain.  With potentials f [nx], g [ny] starting at 0, a sweep is
    f_i <- -eps_t log sum_j b_j exp((g_j - c_ij) / eps_t)         one svae_ot_softmin pass over the rows of X
    g_j <- -eps_t log sum_i a_i exp((f_i - c_ij) / eps_t)         the same over the rows of Y, with the new f
alternating, not averaged.  eps_t = max(epsilon, D scaling^t) at sweep t anneals from the scale of the data, D = the squared
length of the bounding-box diagonal of X and Y together (the length itself for the Euclidean cost); scaling=None disables it.  At
every check_every-th of the sweeps run at eps_t == epsilon the error err = sum_i a_i |exp((f_i - f_i_new) / eps) - 1| is read: the
L1 violation of the row marginals by the plan (f, g) held before the update, and the only host read inside the loop.  The loop
stops at err <= tol, or at max_iter sweeps with a ConvergenceWarning; tol=0 asks for a fixed schedule of max_iter sweeps (no early
stop, no warning).  One more pass over the rows of X then gives the row marginals r_i = a_i exp((f_i - f~_i) / eps) and the mean
cost cbar_i of every row's plan, and from them
    value           sum a f + sum b g: the entropic cost <P, C> + eps KL(P | a x b), exact in the dual since the last update was g's
    transport_cost  sum_i r_i cbar_i = <P, C>
    marginal_error  sum_i |r_i - a_i|, of the plan returned
epsilon=None takes 0.05 x the median cost over all pairs of the stacked rows (svae_mmd_select's exact median).  The 0.05 is an
interface default, not a measured optimum: a smaller epsilon is closer to the unregularised cost and needs more sweeps.

sinkhorn_divergence is OT(X, Y) - OT(X, X) / 2 - OT(Y, Y) / 2 with one epsilon and one annealing scale for the three problems.
The two self problems run the symmetric averaged update f <- (f + softmin(f)) / 2 on one potential (the alternating update crawls
on a symmetric problem), stopped at max |f_new - f| <= tol eps on the same check schedule; their value is 2 sum a f.  When Y is X
the value is exactly 0.0 and no device work is done.

Elementwise updates of the potentials are torch fp64 ops on the device; every sum that enters a reported number is
svae_tsne_sums' fixed-order compensated sum.  Every result is bit-reproducible."""
from __future__ import annotations

import functools
import warnings

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _on_device
from ._inputs import _finite_rows, _int_labels, _is_int, _is_number
from .metrics import ConvergenceWarning

OT_MAX_COLS = _lib.OT_MAX_COLS   # columns of V per svae_ot_apply launch; wider V is handled in slices
_KINDS = {"sqeuclidean": 0, "euclidean": 1}
_EPSILON_FACTOR = 0.05           # epsilon=None: this x the median cost
_OT_CALLS = {"softmin": 0, "apply": 0, "sums": 0, "select": 0}   # launches of svae_ot_softmin / _apply, svae_tsne_sums, svae_mmd_select
_OT_LAST = {"softmin_work": 0, "apply_work": 0}                  # doubles of work of the last launches

_device_of = functools.partial(_device._device_of, who="optimal transport runs on the GPU (csrc/ot.hip); no device is available")


# ---- arguments, before any device work --------------------------------------------------------------------------------------------
def _number(v, name, lo_open=None, integer=False):
    ok = _is_int(v) if integer else _is_number(v)
    if not ok or (lo_open is not None and not v > lo_open):
        raise ValueError(f"{name} must be a finite {'integer' if integer else 'number'}" + (f" > {lo_open}" if lo_open is not None else "") +
                         f", got {v!r}")
    return int(v) if integer else float(v)


def _weights(w, n, name):
    """None (uniform) or positive weights [n] that sum to 1 -> fp64 numpy on the host"""
    if w is None:
        return np.full(n, 1.0 / n)
    w = w.detach().cpu().numpy() if torch.is_tensor(w) else np.asarray(w)
    if w.ndim != 1 or w.shape[0] != n or w.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be [{n}] numbers, got shape {tuple(w.shape)} of {w.dtype}")
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not (np.isfinite(w).all() and (w > 0).all()) or abs(float(w.sum()) - 1.0) > 1e-9:
        raise ValueError(f"{name} must hold finite positive weights that sum to 1")
    return w


def _ot_check(X, Y, epsilon, cost, a, b, scaling, tol, max_iter, check_every):
    x, y = _finite_rows(X, "X"), _finite_rows(Y, "Y")
    nx, ny = x.shape[0], y.shape[0]
    if nx < 1 or ny < 1 or nx >= 1 << 26 or ny >= 1 << 26:
        raise ValueError(f"X and Y need between 1 and 2^26 - 1 rows each, got {nx} and {ny}")
    if x.shape[1] != y.shape[1] or x.shape[1] < 1:
        raise ValueError(f"X and Y must share one feature count >= 1, got {x.shape[1]} and {y.shape[1]}")
    if cost not in _KINDS:
        raise ValueError(f"cost must be one of {sorted(_KINDS)}, got {cost!r}")
    if epsilon is not None:
        epsilon = _number(epsilon, "epsilon", 0)
    if scaling is not None:
        scaling = _number(scaling, "scaling", 0)
        if not scaling < 1:
            raise ValueError(f"scaling must lie in (0, 1), got {scaling!r}")
    tol = _number(tol, "tol")
    if tol < 0:
        raise ValueError(f"tol must be >= 0, got {tol!r}")
    max_iter, check_every = _number(max_iter, "max_iter", 0, True), _number(check_every, "check_every", 0, True)
    return x, y, epsilon, _KINDS[cost], _weights(a, nx, "a"), _weights(b, ny, "b"), scaling, tol, max_iter, check_every


# ---- the device side --------------------------------------------------------------------------------------------------------------
class _Sets:
    """the two row sets on one device with their weights, and the launches of csrc/ot.hip between them"""

    def __init__(self, x, y, a, b, kind, same=False):
        self.dev = _device_of(x, y)
        self.kind = kind
        with torch.cuda.device(self.dev):
            self.lib = _lib.lib()
            self.X = _on_device(x, self.dev)
            self.Y = self.X if same else _on_device(y, self.dev)
            self.a, self.b = torch.from_numpy(a).to(self.dev), torch.from_numpy(b).to(self.dev)
            self.loga, self.logb = torch.from_numpy(np.log(a)).to(self.dev), torch.from_numpy(np.log(b)).to(self.dev)   # the host's log
        self.nx, self.ny, self.d = self.X.shape[0], self.Y.shape[0], self.X.shape[1]
        self._work = None

    def _buffer(self, words):
        if self._work is None or self._work.numel() < words:
            self._work = torch.empty(words, dtype=torch.float64, device=self.dev)
        return self._work

    def softmin(self, Q, C, off, eps, cbar=False):
        """L [m] (and cbar [m]) of the rows Q against the candidates C with the column offsets `off`"""
        m, n = Q.shape[0], C.shape[0]
        words = self.lib.svae_ot_softmin_work(m, n)
        work = self._buffer(words)
        L = torch.empty(m, dtype=torch.float64, device=self.dev)
        cb = torch.empty(m, dtype=torch.float64, device=self.dev) if cbar else None
        _OT_CALLS["softmin"] += 1
        _OT_LAST["softmin_work"] = words
        check(self.lib.svae_ot_softmin(Q.data_ptr(), self.d, m, C.data_ptr(), self.d, n, self.d, off.data_ptr(), 1.0 / eps, self.kind,
                                       work.data_ptr(), L.data_ptr(), cb.data_ptr() if cbar else None, ops._stream()), "ot_softmin")
        return (L, cb) if cbar else L

    def potential(self, Q, C, pot, logw, eps, cbar=False):
        """-(eps L) of the rows Q from the potential `pot` and the log weights of the candidates C"""
        off = torch.mul(pot, 1.0 / eps).add_(logw)
        if cbar:
            L, cb = self.softmin(Q, C, off, eps, True)
            return torch.mul(L, eps).neg_(), L, cb
        return torch.mul(self.softmin(Q, C, off, eps), eps).neg_()

    def apply(self, Q, C, pot, logw, eps, L, V):
        """[m, c] = exp(v - L) V for V [n, c] on the device, in slices of OT_MAX_COLS columns"""
        m, n, c = Q.shape[0], C.shape[0], V.shape[1]
        off = torch.mul(pot, 1.0 / eps).add_(logw)
        out = torch.empty((m, c), dtype=torch.float64, device=self.dev)
        words = self.lib.svae_ot_apply_work(m, n, min(c, OT_MAX_COLS))
        work = self._buffer(words)
        _OT_LAST["apply_work"] = words
        for s in range(0, c, OT_MAX_COLS):
            w = min(OT_MAX_COLS, c - s)
            Vs = V[:, s:s + w].contiguous()
            _OT_CALLS["apply"] += 1
            check(self.lib.svae_ot_apply(Q.data_ptr(), self.d, m, C.data_ptr(), self.d, n, self.d, off.data_ptr(), 1.0 / eps, self.kind,
                                         L.data_ptr(), Vs.data_ptr(), w, w, work.data_ptr(), out[:, s:].data_ptr(), c, ops._stream()),
                  "ot_apply")
        return out

    def sums(self, u, v=None):
        """(sum u, sum v) as host floats: svae_tsne_sums' fixed order"""
        out = torch.zeros(2, dtype=torch.float64, device=self.dev)
        _OT_CALLS["sums"] += 1
        check(self.lib.svae_tsne_sums(u.data_ptr(), v.data_ptr() if v is not None else None, u.numel(), out.data_ptr(), ops._stream()),
              "tsne_sums")
        res = out.cpu().numpy()
        return float(res[0]), float(res[1])


def _median_epsilon(x, y, kind, dev):
    """0.05 x the median cost over all pairs of the stacked rows"""
    with torch.cuda.device(dev):
        lib = _lib.lib()
        Z = torch.cat([_on_device(t, dev) for t in (x, y)]).contiguous()
        if Z.shape[0] < 2:
            raise ValueError("epsilon=None needs at least two rows in all; pass epsilon")
        hm = torch.empty(2, dtype=torch.float64, device=dev)
        work = torch.empty(_lib.MMD_WORK_WORDS, dtype=torch.int64, device=dev)
        _OT_CALLS["select"] += 1
        check(lib.svae_mmd_select(Z.data_ptr(), Z.shape[1], Z.shape[1], Z.shape[0], work.data_ptr(), hm.data_ptr(), ops._stream()), "mmd_select")
        med = float(hm.cpu()[kind ^ 1])   # hm[1] = med^2 for the squared cost, hm[0] = med for the Euclidean one
    eps = _EPSILON_FACTOR * med
    if not eps > 0:
        raise ValueError("the median cost is 0 (all rows equal?): pass epsilon")
    return eps


def _box_scale(S, kind):
    """D of the annealing: from the bounding box of X and Y together, its d corners' differences summed on the host"""
    lo = torch.minimum(S.X.min(dim=0).values, S.Y.min(dim=0).values).cpu().numpy()
    hi = torch.maximum(S.X.max(dim=0).values, S.Y.max(dim=0).values).cpu().numpy()
    s = float(((hi - lo) ** 2).sum())
    return float(np.sqrt(s)) if kind else s


def _eps_at(t, epsilon, D, scaling):
    return epsilon if scaling is None else max(epsilon, D * scaling ** t)


def _not_converged(what, max_iter, err, tol):
    warnings.warn(f"{what} stopped at max_iter = {max_iter} sweeps with error {err:.3e} > tol = {tol:.3e}", ConvergenceWarning, stacklevel=3)


def _solve_cross(S, epsilon, D, scaling, tol, max_iter, check_every):
    """the alternating sweeps -> (f, g on the device, n_iter, converged)"""
    f = torch.zeros(S.nx, dtype=torch.float64, device=S.dev)
    g = torch.zeros(S.ny, dtype=torch.float64, device=S.dev)
    k, n_iter, converged, err = 0, 0, False, float("nan")
    for t in range(max_iter):
        eps_t = _eps_at(t, epsilon, D, scaling)
        f_new = S.potential(S.X, S.Y, g, S.logb, eps_t)
        check_now = False
        if eps_t == epsilon:
            k += 1
            check_now = k % check_every == 0
        if check_now:
            ratio = torch.sub(f, f_new).mul_(1.0 / eps_t)
            err = S.sums(torch.exp(ratio).sub_(1.0).abs_().mul_(S.a))[0]   # the only host read inside the loop
        f = f_new
        g = S.potential(S.Y, S.X, f, S.loga, eps_t)
        n_iter = t + 1
        if check_now and tol > 0 and err <= tol:
            converged = True
            break
    if not converged and tol > 0:
        _not_converged("sinkhorn", max_iter, err, tol)
    return f, g, n_iter, converged


def _solve_self(S, epsilon, D, scaling, tol, max_iter, check_every):
    """the symmetric averaged update on one potential -> (f on the device, value = 2 sum a f, n_iter, converged)"""
    f = torch.zeros(S.nx, dtype=torch.float64, device=S.dev)
    k, n_iter, converged, delta = 0, 0, False, float("nan")
    for t in range(max_iter):
        eps_t = _eps_at(t, epsilon, D, scaling)
        f_new = S.potential(S.X, S.X, f, S.loga, eps_t).add_(f).mul_(0.5)   # (f + softmin(f)) / 2: the sum commutes
        check_now = False
        if eps_t == epsilon:
            k += 1
            check_now = k % check_every == 0
        if check_now:
            delta = float(torch.sub(f_new, f).abs_().max())   # a maximum: exact whatever the order; reduced on the device
        f = f_new
        n_iter = t + 1
        if check_now and tol > 0 and delta <= tol * epsilon:
            converged = True
            break
    if not converged and tol > 0:
        _not_converged("sinkhorn_divergence (self problem)", max_iter, delta, tol * epsilon)
    return f, 2.0 * S.sums(torch.mul(S.a, f))[0], n_iter, converged


class SinkhornResult:
    """What sinkhorn() returns.  value, transport_cost, marginal_error, epsilon: floats; f [nx], g [ny]: the potentials, fp64 numpy;
    n_iter: sweeps run; converged: whether err <= tol was reached.  The methods multiply the row-normalised transport plan with
    columns on the device; the rows of X and Y stay there for them."""

    def __init__(self, sets, f, g, L, r, epsilon, value, transport_cost, marginal_error, n_iter, converged):
        self._sets, self._f, self._g, self._L, self._LT, self._r = sets, f, g, L, None, r
        self.f, self.g = f.cpu().numpy(), g.cpu().numpy()
        self.epsilon, self.value, self.transport_cost, self.marginal_error = epsilon, value, transport_cost, marginal_error
        self.n_iter, self.converged = n_iter, converged

    def __repr__(self):
        return (f"SinkhornResult(value={self.value:.6g}, transport_cost={self.transport_cost:.6g}, epsilon={self.epsilon:.6g}, "
                f"n_iter={self.n_iter}, marginal_error={self.marginal_error:.3g}, converged={self.converged})")

    def _columns(self, V, n, name):
        v = _finite_rows(V, name)
        if v.shape[0] != n or v.shape[1] < 1:
            raise ValueError(f"{name} must be [{n}, c] with c >= 1, got shape {tuple(v.shape)}")
        return (v if torch.is_tensor(v) else torch.from_numpy(v)).to(self._sets.dev)

    def _apply(self, Vd):
        S = self._sets
        with torch.cuda.device(S.dev):
            return S.apply(S.X, S.Y, self._g, S.logb, self.epsilon, self._L, Vd)

    def _apply_transposed(self, Vd):
        S = self._sets
        with torch.cuda.device(S.dev):
            if self._LT is None:
                self._LT = S.softmin(S.Y, S.X, torch.mul(self._f, 1.0 / self.epsilon).add_(S.loga), self.epsilon)
            return S.apply(S.Y, S.X, self._f, S.loga, self.epsilon, self._LT, Vd)

    def apply(self, V):
        """[nx, c] fp64 numpy: every row of X's plan, normalised to sum 1, times V [ny, c]: the plan-weighted mean of V's rows"""
        return self._apply(self._columns(V, self._sets.ny, "V")).cpu().numpy()

    def apply_transposed(self, V):
        """[ny, c]: the same for the rows of Y, with the roles swapped, V [nx, c]"""
        return self._apply_transposed(self._columns(V, self._sets.nx, "V")).cpu().numpy()

    def barycentric_map(self):
        """[nx, d]: where the plan sends every row of X, apply(Y)"""
        return self._apply(self._sets.Y).cpu().numpy()

    def barycentric_map_transposed(self):
        """[ny, d]: where the plan sends every row of Y, apply_transposed(X)"""
        return self._apply_transposed(self._sets.X).cpu().numpy()

    def flow(self, labels_y):
        """(ids, share [nx, K]): the share of each X row's mass that lands in each label of Y; every distinct value of labels_y [ny]
        (any integer dtype, numpy or torch) is a label, in np.unique order"""
        S = self._sets
        ids, inv = np.unique(_int_labels(labels_y, S.ny), return_inverse=True)
        with torch.cuda.device(S.dev):
            lab = torch.from_numpy(inv.reshape(-1).astype(np.int64)).to(S.dev)
            onehot = (lab[:, None] == torch.arange(len(ids), device=S.dev)[None, :]).to(torch.float64)
        return ids, self._apply(onehot).cpu().numpy()

    def row_marginals(self):
        """r [nx]: the mass the returned plan gives every row of X (a up to marginal_error)"""
        return self._r.cpu().numpy()


def _sinkhorn(x, y, epsilon, kind, a, b, scaling, tol, max_iter, check_every, keep=None):
    S = _Sets(x, y, a, b, kind)
    with torch.cuda.device(S.dev):
        if epsilon is None:
            epsilon = _median_epsilon(x, y, kind, S.dev)
        D = _box_scale(S, kind)
        f, g, n_iter, converged = _solve_cross(S, epsilon, D, scaling, tol, max_iter, check_every)
        ft, L, cbar = S.potential(S.X, S.Y, g, S.logb, epsilon, cbar=True)
        ratio = torch.exp(torch.sub(f, ft).mul_(1.0 / epsilon))
        r = torch.mul(S.a, ratio)
        cost, merr = S.sums(torch.mul(r, cbar), torch.sub(ratio, 1.0).abs_().mul_(S.a))
        value = S.sums(torch.mul(S.a, f))[0] + S.sums(torch.mul(S.b, g))[0]
    if keep is not None:
        keep.update(epsilon=epsilon, D=D)
    return SinkhornResult(S, f, g, L, r, epsilon, value, cost, merr, n_iter, converged)


def sinkhorn(X, Y, *, epsilon=None, cost="sqeuclidean", a=None, b=None, scaling=0.5, tol=1e-6, max_iter=1000, check_every=10):
    """The entropic optimal transport between the rows X [nx, d] with weights a and Y [ny, d] with weights b (module docstring) ->
    SinkhornResult.  epsilon=None: 0.05 x the median cost of the stacked rows, an interface default and not a measured optimum."""
    return _sinkhorn(*_ot_check(X, Y, epsilon, cost, a, b, scaling, tol, max_iter, check_every))


class SinkhornDivergence:
    """value = ot_xy - ot_xx / 2 - ot_yy / 2; cross: the SinkhornResult of X against Y (None when Y is X)"""

    def __init__(self, value, ot_xy, ot_xx, ot_yy, cross):
        self.value, self.ot_xy, self.ot_xx, self.ot_yy, self.cross = value, ot_xy, ot_xx, ot_yy, cross

    def __repr__(self):
        return f"SinkhornDivergence(value={self.value!r}, ot_xy={self.ot_xy!r}, ot_xx={self.ot_xx!r}, ot_yy={self.ot_yy!r})"


def sinkhorn_divergence(X, Y, *, epsilon=None, cost="sqeuclidean", a=None, b=None, scaling=0.5, tol=1e-6, max_iter=1000, check_every=10):
    """The Sinkhorn divergence OT(X, Y) - OT(X, X) / 2 - OT(Y, Y) / 2: zero for equal sets, positive otherwise, in the units of the
    cost.  One epsilon and one annealing scale serve the three problems; the self problems run the symmetric averaged update.
    When Y is X the value is exactly 0.0 and no device work is done."""
    x, y, epsilon, kind, a, b, scaling, tol, max_iter, check_every = _ot_check(X, Y, epsilon, cost, a, b, scaling, tol, max_iter, check_every)
    if Y is X:
        if not np.array_equal(a, b):
            raise ValueError("Y is X with different weights a and b: pass a copy of X")
        return SinkhornDivergence(0.0, None, None, None, None)
    keep = {}
    cross = _sinkhorn(x, y, epsilon, kind, a, b, scaling, tol, max_iter, check_every, keep)
    S = cross._sets
    selves = []
    for rows, w in ((S.X, a), (S.Y, b)):
        T = _Sets(rows, rows, w, w, kind, same=True)
        with torch.cuda.device(T.dev):
            selves.append(_solve_self(T, keep["epsilon"], keep["D"], scaling, tol, max_iter, check_every)[1])
    return SinkhornDivergence(cross.value - selves[0] / 2 - selves[1] / 2, cross.value, selves[0], selves[1], cross)


def transport_flow(result, labels_x, labels_y):
    """(ids_x, ids_y, mass [Kx, Ky]): the transport plan aggregated by cluster, result.flow(labels_y) weighted by the row marginals
    and summed per label of X.  mass sums to 1 (up to result.marginal_error): the soft counterpart of hungarian_match for two sets
    that do not share rows."""
    if not isinstance(result, SinkhornResult):
        raise ValueError("result must be what sinkhorn() returned")
    lx = _int_labels(labels_x, result._sets.nx)
    ids_x, inv = np.unique(lx, return_inverse=True)
    inv = inv.reshape(-1)
    ids_y, share = result.flow(labels_y)
    r = result.row_marginals()
    mass = np.stack([(r[inv == k, None] * share[inv == k]).sum(axis=0) for k in range(len(ids_x))])
    return ids_x, ids_y, mass
