"""Generators, the numpy restatement and the gates of the density map (scrubvae_amd/eval/density.py, csrc/density.hip), used by
test_density_cpu.py (against sklearn and scipy) and test_gpu_density.py (against the kernel).

density_ref is the definition, not separable: per cell the sum over the points of c_i exp(-((x_a - Y[i, 0])^2 + (y_b - Y[i, 1])^2) /
(2 h_i^2)) with everything from the fp64 inputs on in np.longdouble, rounded to fp64 once.

density_gate is derived from the arithmetic the kernel performs, not measured.  u = 2^-53.  Per point and axis the kernel forms
    e = fl(x_a - Y[i, 0])  (1 rounding),  q = fl(e e)  (e twice, 1 more),  s = fl(1 / fl(2 fl(h h)))  (2; the doubling is exact),
    arg = fl(q s)  (1):  a relative error of at most 6 u in arg, so exp(arg) is off by the factor 1 + 6 u |arg| to first order;
the two axes add, which gives c1 = 6 against |arg_i| = the whole exponent of the term.  Then, relative to the term:
    the device exp, documented to 1 ulp <= 2 u, once per axis                                 4 u
    c_i = fl(s fl(1 / pi)): s carries 2 u, the constant 1, the product 1                      4 u
    c_i times the y factor (per point, or once per cell for a common h)                       1 u
    the product of the two factors in the MFMA                                                1 u
    the closing sum + comp of the compensated sum, and the division by n                      2 u
    the rounding of the long-double reference to fp64                                         1 u
so c0 = 13.  Every term is positive, so ANY order of adding n of them is within (n - 1) u of their sum to first order: the bound
does not depend on tiles, chunks or slices.  The long-double sum itself is within n 2^-64 = n u / 2048 of the truth.  Together
    gate = 1.001 u (sum_i t_i (6 |arg_i| + 13) + (n - 1 + n / 2048) sum_i t_i) / n + floor
with 1.001 for the second-order terms (k u < 1e-9 for every k here).  floor covers what underflow loses: a factor, the product
c_i B or the product A B that falls below DBL_MIN may be flushed to zero, each at most DBL_MIN times the remaining factors <=
max(1, c_i), and the closing scale may round into the subnormals: floor = DBL_MIN (1 + 3 mean_i max(1, c_i)).  The gate has no
division, so exact zeros compare clean."""
import functools

import numpy as np

EPS = 2.0 ** -53
C1, C0 = 6.0, 13.0
DBL_MIN = np.finfo(np.float64).tiny
LD = np.longdouble
PI_LD = LD(4) * np.arctan(LD(1))
LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63   # otherwise there is no truth to hold a value to

# the constants of csrc/density.hip that the sizes below are chosen against
TILE, CHUNK, MAX_SLICES, BLOCKS = 128, 32, 128, 512


def slices(n, gx, gy):
    """(slices, chunks per slice) of csrc/density.hip's den_plan"""
    tiles = -(-gx // TILE) * -(-gy // TILE)
    nchunks = -(-n // CHUNK)
    want = min(nchunks, MAX_SLICES, -(-BLOCKS // tiles))
    cps = -(-nchunks // want)
    return -(-nchunks // cps), cps


def nodes(lo, hi, g):
    """lo + a step, step = (hi - lo) / (g - 1): one product and one sum in fp64"""
    step = (hi - lo) / (g - 1)
    return lo + np.arange(g, dtype=np.float64) * step


def blobs(n, seed=5, spread=1.0):
    """n points around three separated centres (n // 3 each, the rest at the last), general fp64 values"""
    g = np.random.default_rng(seed)
    mu = np.array([[-6.0, -4.0], [5.5, -3.0], [0.5, 6.0]])
    which = np.minimum(np.arange(n) // max(n // 3, 1), 2)
    return mu[which] + spread * g.normal(size=(n, 2))


def decades(n, seed=9):
    """per-point bandwidths spread over three decades, 0.03 to 30"""
    return 0.03 * 10.0 ** (3.0 * np.random.default_rng(seed).random(n))


def _terms(y, h, X, Y):
    """(D, W) long double at the cells (X[j], Y[j]): D = sum_i t_i / n and W = sum_i t_i |arg_i| / n"""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    hh = np.broadcast_to(np.asarray(h, np.float64), (n,)).astype(LD)
    q = LD(2) * hh * hh
    c = LD(1) / (PI_LD * q)
    X, Y = np.asarray(X, np.float64).astype(LD), np.asarray(Y, np.float64).astype(LD)
    D, W = np.zeros(X.shape, LD), np.zeros(X.shape, LD)
    step = max(1, 2_000_000 // max(X.size, 1))
    for i0 in range(0, n, step):
        px, py = y[i0:i0 + step, 0].astype(LD), y[i0:i0 + step, 1].astype(LD)
        ex, ey = X[:, None] - px[None, :], Y[:, None] - py[None, :]
        arg = (ex * ex + ey * ey) / q[None, i0:i0 + step]
        t = c[None, i0:i0 + step] * np.exp(-arg)
        D += t.sum(axis=1)
        W += (t * arg).sum(axis=1)
    return D / LD(n), W / LD(n)


def _cells(grid, cells):
    xs, ys = grid
    if cells is None:
        b, a = np.divmod(np.arange(len(ys) * len(xs)), len(xs))
        return xs[a], ys[b], (len(ys), len(xs))
    b, a = cells
    return xs[np.asarray(a)], ys[np.asarray(b)], np.shape(b)


def density_ref(y, h, grid, cells=None):
    """the definition at every node of grid = (xs, ys) as fp64 [gy, gx], or at the cells (b [m], a [m]) alone as [m]"""
    X, Y, shape = _cells(grid, cells)
    return _terms(y, h, X, Y)[0].astype(np.float64).reshape(shape)


def density_gate(y, h, grid, cells=None):
    """the per-cell bound of the module docstring, fp64, the shape of density_ref"""
    return ref_and_gate(y, h, grid, cells)[1]


def ref_and_gate(y, h, grid, cells=None):
    """both from one pass"""
    X, Y, shape = _cells(grid, cells)
    D, W = _terms(y, h, X, Y)
    n = len(y)
    hh = np.broadcast_to(np.asarray(h, np.float64), (n,))
    floor = DBL_MIN * (1.0 + 3.0 * float(np.maximum(1.0, 1.0 / (2.0 * np.pi * hh * hh)).mean()))
    g = LD(1.001 * EPS) * (LD(C1) * W + LD(C0 + n - 1 + n / 2048.0) * D) + LD(floor)
    return D.astype(np.float64).reshape(shape), g.astype(np.float64).reshape(shape)


# ---- regions: a per-cell uphill walk, a different algorithm from the nine shifted views and pointer jumping ------------------------
def regions_ref(D, min_density=0.0):
    """(regions [gy, gx] int32, peaks [R, 2] int64 as (b, a)) by walking uphill from every cell, one step at a time"""
    D = np.asarray(D, np.float64)
    gy, gx = D.shape
    rows = D.tolist()
    root = [[None] * gx for _ in range(gy)]

    def up(b, a):
        bb, ba, bv = b, a, rows[b][a]
        for nb in range(max(b - 1, 0), min(b + 2, gy)):
            for na in range(max(a - 1, 0), min(a + 2, gx)):
                v = rows[nb][na]
                if v > bv or (v == bv and nb * gx + na < bb * gx + ba):
                    bb, ba, bv = nb, na, v
        return bb, ba

    for b in range(gy):
        for a in range(gx):
            path, cur = [], (b, a)
            while root[cur[0]][cur[1]] is None:
                nxt = up(*cur)
                if nxt == cur:
                    root[cur[0]][cur[1]] = cur
                    break
                path.append(cur)
                cur = nxt
            r = root[cur[0]][cur[1]]
            for p in path:
                root[p[0]][p[1]] = r
    thr = min_density * D.max()
    peaks = sorted({r for line in root for r in line if D[r] >= thr}, key=lambda r: (-D[r], r[0] * gx + r[1]))
    number = {r: k for k, r in enumerate(peaks)}
    regions = np.full((gy, gx), -1, dtype=np.int32)
    for b in range(gy):
        for a in range(gx):
            if D[b, a] >= thr:
                regions[b, a] = number[root[b][a]]
    return regions, np.array(peaks, dtype=np.int64).reshape(-1, 2)


def labels_ref(y, xs, ys, regions):
    """each point's region: the nearest node by rint((x - xs[0]) / dx), dx = (xs[-1] - xs[0]) / (gx - 1); -1 outside the extent"""
    dx, dy = (xs[-1] - xs[0]) / (len(xs) - 1), (ys[-1] - ys[0]) / (len(ys) - 1)
    out = np.full(len(y), -1, dtype=np.int64)
    for i, (px, py) in enumerate(np.asarray(y, np.float64)):
        if xs[0] <= px <= xs[-1] and ys[0] <= py <= ys[-1]:
            a, b = int(np.rint((px - xs[0]) / dx)), int(np.rint((py - ys[0]) / dy))
            out[i] = regions[min(b, len(ys) - 1), min(a, len(xs) - 1)]
    return out


# ---- the label cases: three blobs of 200 points, the grids and bandwidths whose margins test_density_cpu.py asserts ---------------
#               name          gx   gy   h    min_density
LABEL_CASES = {"96x103": (96, 103, 1.0, 0.05),
               "70x33": (70, 33, 1.0, 0.05),
               "256x256": (256, 256, 0.8, 0.05)}
LABEL_PAD = 3.0


@functools.lru_cache(maxsize=None)
def label_case(name):
    """(y, h, (xs, ys), min_density, D, G): the reference density and its gate, computed once"""
    gx, gy, h, md = LABEL_CASES[name]
    y = blobs(600)
    lo, hi = y.min(axis=0), y.max(axis=0)
    m = LABEL_PAD * h
    grid = (nodes(float(lo[0]) - m, float(hi[0]) + m, gx), nodes(float(lo[1]) - m, float(hi[1]) + m, gy))
    D, G = ref_and_gate(y, h, grid)
    for v in (y, D, G) + grid:
        v.setflags(write=False)
    return y, h, grid, md, D, G


def margins(D, G, min_density):
    """(window, threshold, peaks): the smallest of (D_best - D_j) - 2 (G_best + G_j) over the cells j != best of every 3 x 3 window
    centred on a cell at or above the threshold; the smallest of |D_c - thr| - 2 (G_c + min_density G_max) over all cells; the
    smallest of the same difference between two numbered peaks.  All three positive: a density within G of D everywhere has the
    regions, the peaks and their order of D.  Also returns the smallest relative window gap, for the record."""
    gy, gx = D.shape
    thr = min_density * D.max()
    gmax = G.reshape(-1)[np.argmax(D)]
    P = np.full((gy + 2, gx + 2), -np.inf)
    P[1:-1, 1:-1] = D
    Q = np.zeros((gy + 2, gx + 2))
    Q[1:-1, 1:-1] = G
    win = np.stack([P[db:db + gy, da:da + gx] for db in range(3) for da in range(3)])
    gat = np.stack([Q[db:db + gy, da:da + gx] for db in range(3) for da in range(3)])
    k = np.argmax(win, axis=0)
    best, gbest = np.take_along_axis(win, k[None], 0)[0], np.take_along_axis(gat, k[None], 0)[0]
    slack = (best[None] - win) - 2.0 * (gbest[None] + gat)
    other = np.arange(9)[:, None, None] != k[None]
    live = (D >= thr)[None] & other & np.isfinite(win)
    window = float(slack[live].min())
    rel = float(((best[None] - win) / best[None])[live].min())
    threshold = float((np.abs(D - thr) - 2.0 * (G + min_density * gmax)).min())
    _, pk = regions_ref(D, min_density)
    d, g = D[pk[:, 0], pk[:, 1]], G[pk[:, 0], pk[:, 1]]
    peaks = min((float(d[i] - d[j] - 2.0 * (g[i] + g[j])) for i in range(len(pk)) for j in range(i + 1, len(pk))), default=np.inf)
    return window, threshold, peaks, rel
