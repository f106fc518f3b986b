"""Density map of a 2-D embedding and its watershed regions: the behaviour-map step after t-SNE (csrc/density.hip).

    density_map(y, *, bandwidth="scott", n_neighbors=None, grid_size=256, extent=None, pad=3.0)
                                                    DensityGrid(density [gy, gx] float64 numpy, xs [gx], ys [gy], bandwidth)
    density_regions(density, *, min_density=0.0)    (regions [gy, gx] int32, peaks [R, 2] int64 as (b, a)), on the host
    DensityMap(bandwidth="scott", n_neighbors=None, grid_size=256, extent=None, pad=3.0, min_density=0.01)
                                                    fit / fit_predict / predict: every row labelled by the basin it falls in

y is [n, 2], numpy or torch, host or device, any float dtype; the rows go to fp64 as for the other eval modules.  It is what
TSNE.embedding_ holds.  The grid is xs[a] = xmin + a dx with dx = (xmax - xmin) / (gx - 1), and ys[b] likewise: each node is that
one product and one sum in fp64, on the host and in the kernel alike (not a linspace).  extent = (xmin, xmax, ymin, ymax)
defaults to the bounding box of y widened by pad x the largest bandwidth.  grid_size is an int or (gx, gy), each side 2 to
DENSITY_MAX_GRID = 1024.  The density has the image convention density[b, a]:

    density[b, a] = (1 / n) sum_i (1 / (2 pi h_i^2)) exp(-((xs[a] - y[i, 0])^2 + (ys[b] - y[i, 1])^2) / (2 h_i^2))

bandwidth is a positive float (one h for all rows), an [n] array of positive h_i, or
    "scott"   n^(-1 / 6) sqrt((var_x + var_y) / 2) with ddof = 1: Scott's factor for two dimensions times the pooled deviation.  It
              is reduced where y lives, so its last bit may differ between a host and a device copy of one y; every other
              bandwidth gives equal bytes for both.
    "knn"     h_i = the distance of row i to its n_neighbors-th neighbour in the embedding (eval.neighbors.kneighbors): narrow
              kernels where the map is dense, wide ones where it is sparse.  ValueError if any h_i is 0 (duplicated rows).

What matches which library: with a float bandwidth the density is exp(sklearn.neighbors.KernelDensity(bandwidth=h, rtol=0,
atol=0).fit(y).score_samples(nodes)), which is itself only good to about 1e-7 relative; this one is exact up to the roundoff of
an fp64 sum (a few units of roundoff times the exponent, tests/density_checks.py has the bound) and bit-reproducible from run
to run and from device to device.  On a grid without exact ties the peaks of density_regions are the cells where
scipy.ndimage.maximum_filter(density, size=3) == density.

Differences by design:
  - No binning and no FFT blur (MotionMapper's recipe): the exact positions are used, which is what allows a bandwidth per row.
  - No cutoff, no tree, no tolerance: every point contributes to every node; a contribution that underflows is exactly 0.
  - sklearn has no per-row bandwidth; scipy.stats.gaussian_kde uses the full covariance, "scott" here is isotropic.
  - density_regions is steepest ascent on the 8-neighbour grid, not skimage's flooding watershed: every cell points to the cell of
    its 3 x 3 window (clipped at the border) with the greatest key, where the key is (density, the lower flat index wins);
    following the pointers ends at a root, and a region is the set of cells that end at one root.  The roots are numbered
    0..R-1 by descending peak density, then by flat index.  Cells with density < min_density x density.max() get -1, and a root
    below that threshold (its whole basin is then -1) is not numbered.  A constant grid is one region.

Errors: ValueError, before any device work, for y that is not [n >= 1, 2] or holds non-finite values, a bandwidth that is not
positive and finite (or "scott" with fewer than 2 rows or no spread), a grid side outside 2..1024, an empty or non-finite extent,
a negative pad, n_neighbors without "knn" or "knn" without it; after the neighbour search for a zero "knn" bandwidth.
RuntimeError when no device is available: there is no host path.

DensityMap.labels_ holds -1 for rows in no region, which is what silhouette_score(..., noise_label=-1) leaves out, and what
cluster_entropy and hungarian_match take as one more label, unchanged:

    emb = TSNE(perplexity=30).fit_transform(z)
    lab = DensityMap(bandwidth="knn", n_neighbors=10).fit_predict(emb)
    score = silhouette_score(z, lab, noise_label=-1)
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check
from . import _device
from ._device import _on_device
from ._inputs import _finite_rows, _is_int

DENSITY_MAX_GRID = _lib.DENSITY_MAX_GRID  # the cap on each side of the grid
_DENSITY_CALLS = {"grid": 0}              # launches of svae_density_grid by this process
_DENSITY_LAST = {"work": 0}               # bytes of work of the last run

DensityGrid = namedtuple("DensityGrid", ["density", "xs", "ys", "bandwidth"])

_device_of = functools.partial(_device._device_of, who="the density map runs on the GPU (csrc/density.hip); no device is available")


# ---- argument checks, before any device work ------------------------------------------------------------------------------------
def _is_number(v):
    """a number, finite or not: the range checks below refuse inf and nan in their own words"""
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def _den_rows(y):
    x = _finite_rows(y, "y")
    if x.shape[1] != 2 or x.shape[0] < 1:
        raise ValueError(f"y must be [n >= 1, 2], got shape {tuple(x.shape)}")
    if x.shape[0] > 2 ** 30:
        raise ValueError(f"at most 2^30 rows are supported, got {x.shape[0]}")
    return x


def _den_grid_size(grid_size):
    g = (grid_size, grid_size) if _is_number(grid_size) else tuple(grid_size) if isinstance(grid_size, (tuple, list)) else None
    if g is None or len(g) != 2 or not all(_is_int(v) for v in g):
        raise ValueError(f"grid_size must be an int or (gx, gy), got {grid_size!r}")
    gx, gy = int(g[0]), int(g[1])
    if not (2 <= gx <= DENSITY_MAX_GRID and 2 <= gy <= DENSITY_MAX_GRID):
        raise ValueError(f"each side of the grid must be 2 to {DENSITY_MAX_GRID}, got {gx} x {gy}")
    return gx, gy


def _scott(x):
    """n^(-1 / 6) sqrt((var_x + var_y) / 2), ddof = 1"""
    n = x.shape[0]
    if n < 2:
        raise ValueError('bandwidth="scott" needs at least 2 rows')
    var = x.var(dim=0, unbiased=True).cpu().numpy() if torch.is_tensor(x) else x.var(axis=0, ddof=1)
    return float(n ** (-1.0 / 6.0) * math.sqrt((float(var[0]) + float(var[1])) / 2.0))


def _den_bandwidth(bandwidth, n_neighbors, x):
    """-> (h float or None, h_rows fp64 [n] numpy or torch or None, k for "knn" or None)"""
    n = x.shape[0]
    if isinstance(bandwidth, str):
        if bandwidth not in ("scott", "knn"):
            raise ValueError(f'bandwidth must be a positive number, an [n] array, "scott" or "knn", got {bandwidth!r}')
        if bandwidth == "knn":
            if not _is_int(n_neighbors):
                raise ValueError(f'bandwidth="knn" needs an integer n_neighbors, got {n_neighbors!r}')
            from .neighbors import KNN_MAX_K
            if not 1 <= n_neighbors <= min(n - 1, KNN_MAX_K):
                raise ValueError(f"n_neighbors must be 1 to min(n - 1, {KNN_MAX_K}) with n = {n}, got {n_neighbors}")
            return None, None, int(n_neighbors)
    if n_neighbors is not None:
        raise ValueError('n_neighbors belongs to bandwidth="knn"')
    if isinstance(bandwidth, str):
        h = _scott(x)
    elif _is_number(bandwidth):
        h = float(bandwidth)
    else:
        rows = bandwidth.detach().to(torch.float64) if torch.is_tensor(bandwidth) else np.ascontiguousarray(bandwidth, dtype=np.float64)
        if rows.ndim != 1 or rows.shape[0] != n:
            raise ValueError(f"a bandwidth array must be [n = {n}], got shape {tuple(rows.shape)}")
        _den_check_rows_h(rows)
        return None, rows, None
    s = 1.0 / (2.0 * (h * h)) if math.isfinite(h) and h > 0 and h * h > 0 else 0.0
    if not (s > 0 and math.isfinite(s)):
        raise ValueError(f"the bandwidth must be positive and finite (and its square too), got {h!r}")
    return h, None, None


def _den_check_rows_h(rows):
    """every h_i > 0 with 1 / (2 h_i^2) positive and finite (the square neither underflows nor overflows); nan fails h > 0"""
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        s = 1.0 / (2.0 * (rows * rows))
    if not (bool((rows > 0).all()) and bool((s > 0).all()) and bool((s < math.inf).all())):
        raise ValueError("every bandwidth must be positive and finite (and its square too)")


def _den_extent(extent, pad, x, hmax):
    if extent is None:
        if not _is_number(pad) or not (math.isfinite(pad) and pad >= 0):
            raise ValueError(f"pad must be a finite number >= 0, got {pad!r}")
        lo, hi = (x.min(dim=0).values.cpu().numpy(), x.max(dim=0).values.cpu().numpy()) if torch.is_tensor(x) else (x.min(axis=0), x.max(axis=0))
        m = float(pad) * hmax
        extent = (float(lo[0]) - m, float(hi[0]) + m, float(lo[1]) - m, float(hi[1]) + m)
    if not isinstance(extent, (tuple, list, np.ndarray)) or len(extent) != 4 or not all(_is_number(v) for v in extent):
        raise ValueError(f"extent must be (xmin, xmax, ymin, ymax), got {extent!r}")
    xmin, xmax, ymin, ymax = (float(v) for v in extent)
    if not (all(math.isfinite(v) for v in (xmin, xmax, ymin, ymax)) and xmax > xmin and ymax > ymin):
        raise ValueError(f"the extent is empty or not finite: {(xmin, xmax, ymin, ymax)!r}")
    return xmin, xmax, ymin, ymax


def _den_nodes(lo, hi, g):
    """(step, nodes [g]): lo + a step in fp64, the arithmetic of the kernel"""
    step = (hi - lo) / (g - 1)
    if not (step > 0 and math.isfinite(step)):
        raise ValueError(f"the extent ({lo!r}, {hi!r}) is too narrow or too wide for {g} nodes")
    return step, lo + np.arange(g, dtype=np.float64) * step


# ---- the device side ------------------------------------------------------------------------------------------------------------
def _density_device(x, h, h_rows, x0, dx, gx, y0, dy, gy, info=None):
    """D fp64 [gy, gx] on the device of x (fp64 rows [n, >= 2], numpy or torch; columns 0 and 1 are the points).  info (a dict)
    receives the synchronised host-clock time density_s of the launch."""
    dev = _device_of(x)
    with torch.cuda.device(dev):
        lib = _lib.lib()
        Y = x.to(dev) if torch.is_tensor(x) else _on_device(x, dev)
        if Y.stride(1) != 1 or Y.stride(0) < 2:
            Y = Y.contiguous()
        n = Y.shape[0]
        hr = None if h_rows is None else _on_device(h_rows, dev)
        nbytes = lib.svae_density_work(n, gx, gy)
        if nbytes <= 0:
            raise ValueError(f"density: sizes out of range (n={n} grid {gx} x {gy})")
        work = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.float64, device=dev)
        D = torch.empty((gy, gx), dtype=torch.float64, device=dev)
        st = ops._stream()
        t0 = _device._clock(dev, info is not None)
        _DENSITY_CALLS["grid"] += 1
        check(lib.svae_density_grid(Y.data_ptr(), Y.stride(0), n, None if hr is None else hr.data_ptr(), 0.0 if h is None else h,
                                    x0, dx, gx, y0, dy, gy, work.data_ptr(), D.data_ptr(), st), "density_grid")
        if info is not None:
            info.update(density_s=_device._clock(dev) - t0)
        _DENSITY_LAST.update(work=nbytes)
    return D


def _density_map(y, bandwidth, n_neighbors, grid_size, extent, pad, info=None):
    x = _den_rows(y)
    gx, gy = _den_grid_size(grid_size)
    h, h_rows, k = _den_bandwidth(bandwidth, n_neighbors, x)
    if extent is not None:
        extent = _den_extent(extent, pad, x, 0.0)       # a given extent is checked before the neighbour search
    elif not _is_number(pad) or not (math.isfinite(pad) and pad >= 0):
        raise ValueError(f"pad must be a finite number >= 0, got {pad!r}")
    if k is not None:
        from .neighbors import _knn_device
        dist, _ = _knn_device(x, k, None)
        h_rows = dist[:, k - 1].contiguous()
        if not bool((h_rows > 0).all()):
            raise ValueError(f"a row's {k}-th neighbour is at distance 0: duplicated rows give no \"knn\" bandwidth; raise n_neighbors")
        _den_check_rows_h(h_rows)
    hmax = h if h_rows is None else float(h_rows.max())
    xmin, xmax, ymin, ymax = extent if extent is not None else _den_extent(None, pad, x, hmax)
    dx, xs = _den_nodes(xmin, xmax, gx)
    dy, ys = _den_nodes(ymin, ymax, gy)
    D = _density_device(x, h, h_rows, xmin, dx, gx, ymin, dy, gy, info)
    bw = h if h_rows is None else (h_rows.cpu().numpy() if torch.is_tensor(h_rows) else h_rows)
    return DensityGrid(D.cpu().numpy(), xs, ys, bw)


def density_map(y, *, bandwidth="scott", n_neighbors=None, grid_size=256, extent=None, pad=3.0):
    """The Gaussian kernel density of the rows of y [n, 2] on a regular grid, exact and bit-reproducible: DensityGrid(density
    [gy, gx] float64, xs [gx], ys [gy], bandwidth: the float or the [n] array used).  See the module docstring."""
    return _density_map(y, bandwidth, n_neighbors, grid_size, extent, pad)


# ---- regions: host numpy --------------------------------------------------------------------------------------------------------
def _den_grid_array(density):
    D = density.detach().cpu().numpy() if torch.is_tensor(density) else np.asarray(density)
    if D.ndim != 2 or D.shape[0] < 1 or D.shape[1] < 1 or D.dtype.kind not in "fiu":
        raise ValueError(f"density must be a 2-D array of numbers, got shape {D.shape} of {D.dtype}")
    D = np.ascontiguousarray(D, dtype=np.float64)
    if not np.isfinite(D).all():
        raise ValueError("density holds non-finite values")
    return D


def density_regions(density, *, min_density=0.0):
    """(regions [gy, gx] int32, peaks [R, 2] int64 as (b, a)): steepest ascent on the 8-neighbour grid.  Every cell points to the
    cell of its 3 x 3 window (clipped at the border) with the greatest key (density, the lower flat index wins); following the
    pointers ends at a root.  The roots with density >= min_density x density.max() are numbered 0..R-1 by descending density,
    then by flat index; regions holds each cell's root number, and -1 where density < min_density x density.max().  A constant
    grid is one region; on a grid without ties the roots are the cells where scipy.ndimage.maximum_filter(size=3) == density."""
    D = _den_grid_array(density)
    if not _is_number(min_density) or not 0 <= min_density <= 1:
        raise ValueError(f"min_density must be in [0, 1], got {min_density!r}")
    gy, gx = D.shape
    flat = np.arange(gy * gx, dtype=np.int64).reshape(gy, gx)
    P = np.full((gy + 2, gx + 2), -np.inf)
    P[1:-1, 1:-1] = D
    F = np.zeros((gy + 2, gx + 2), dtype=np.int64)
    F[1:-1, 1:-1] = flat
    best, ptr = np.full((gy, gx), -np.inf), flat.copy()
    for db in (0, 1, 2):              # ascending flat index: a strict > keeps the lower index on equal densities
        for da in (0, 1, 2):
            v = P[db:db + gy, da:da + gx]
            take = v > best
            best = np.where(take, v, best)
            ptr = np.where(take, F[db:db + gy, da:da + gx], ptr)
    ptr = ptr.reshape(-1)
    while True:                       # pointer jumping: the path length halves every round
        nxt = ptr[ptr]
        if np.array_equal(nxt, ptr):
            break
        ptr = nxt
    d = D.reshape(-1)
    thr = min_density * d.max()
    roots = np.flatnonzero((ptr == flat.reshape(-1)) & (d >= thr))
    roots = roots[np.lexsort((roots, -d[roots]))]
    number = np.full(gy * gx, -1, dtype=np.int32)
    number[roots] = np.arange(len(roots), dtype=np.int32)
    regions = np.where(d >= thr, number[ptr], np.int32(-1)).astype(np.int32).reshape(gy, gx)
    return regions, np.stack([roots // gx, roots % gx], axis=1).astype(np.int64)


class DensityMap:
    """Label the rows of a 2-D embedding by the basin of the density map they fall in (MotionMapper's watershed step).
    fit(y): density_map with the constructor's arguments, then density_regions(min_density).  Attributes: density_ [gy, gx], xs_
    [gx], ys_ [gy], bandwidth_, regions_ [gy, gx] int32, peaks_ [R, 2] float64 (x, y) in data coordinates, labels_ [n] int64,
    region_counts_ [R] int64.  predict(y_new) labels each row by the region of its nearest grid node, rint((x - xs_[0]) / dx)
    with dx = (xs_[-1] - xs_[0]) / (gx - 1); -1 outside the extent or in a cell of no region.  labels_ feeds silhouette_score(..., noise_label=-1), cluster_entropy and
    hungarian_match unchanged."""

    def __init__(self, bandwidth="scott", n_neighbors=None, grid_size=256, extent=None, pad=3.0, min_density=0.01):
        self.bandwidth, self.n_neighbors, self.grid_size, self.extent, self.pad = bandwidth, n_neighbors, grid_size, extent, pad
        self.min_density = min_density

    def fit(self, y, info=None):
        if not _is_number(self.min_density) or not 0 <= self.min_density <= 1:
            raise ValueError(f"min_density must be in [0, 1], got {self.min_density!r}")
        g = _density_map(y, self.bandwidth, self.n_neighbors, self.grid_size, self.extent, self.pad, info)
        self.density_, self.xs_, self.ys_, self.bandwidth_ = g
        self.regions_, cells = density_regions(g.density, min_density=self.min_density)
        self.peaks_ = np.stack([self.xs_[cells[:, 1]], self.ys_[cells[:, 0]]], axis=1).reshape(-1, 2)
        self.labels_ = self.predict(y)
        self.region_counts_ = np.bincount(self.labels_[self.labels_ >= 0], minlength=len(cells)).astype(np.int64)
        return self

    def fit_predict(self, y):
        return self.fit(y).labels_

    def predict(self, y_new):
        if not hasattr(self, "regions_"):
            raise RuntimeError("DensityMap.predict before fit")
        x = _den_rows(y_new)
        p = x.cpu().numpy() if torch.is_tensor(x) else x
        xs, ys = self.xs_, self.ys_
        dx, dy = (xs[-1] - xs[0]) / (len(xs) - 1), (ys[-1] - ys[0]) / (len(ys) - 1)
        inside = (p[:, 0] >= xs[0]) & (p[:, 0] <= xs[-1]) & (p[:, 1] >= ys[0]) & (p[:, 1] <= ys[-1])
        a = np.clip(np.rint((p[:, 0] - xs[0]) / dx), 0, len(xs) - 1).astype(np.int64)
        b = np.clip(np.rint((p[:, 1] - ys[0]) / dy), 0, len(ys) - 1).astype(np.int64)
        return np.where(inside, self.regions_[b, a], -1).astype(np.int64)
