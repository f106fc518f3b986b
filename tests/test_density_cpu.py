"""The density map without a GPU: the restatement of tests/density_checks.py pinned to sklearn's KernelDensity, density_regions
held to the per-cell uphill walk with exact equality and to scipy's maximum filter, the decision margins that let
test_gpu_density.py demand equal labels, the bandwidth formulas, predict's rounding, argument errors before any device work and
the C-ABI exports."""
import os
import re

import numpy as np
import pytest
import torch

from tests import density_checks as DC
from tests.test_rank_cpu import untouched

needs_longdouble = pytest.mark.skipif(not DC.LONGDOUBLE, reason="np.longdouble is no wider than fp64 here: no truth to hold the value to")


@needs_longdouble
@pytest.mark.parametrize("h", [1.0, 0.35])
def test_restatement_is_sklearn(h):
    """sklearn's KernelDensity(rtol=0, atol=0) against the long-double sum, on the cells with density >= 1e-9 max.  The tolerance is
    sklearn's own error (it sums in log space through a tree), not ours: measured on these inputs (three blobs of 200 points, a 40 x
    37 grid) the largest relative difference is 1.9e-7 at h = 1 (1346 cells) and 8.8e-7 at h = 0.35 (688 cells), both in the far
    tails; it varies with the tree's leaf order, so the test allows 4 x the larger one, 3.6e-6."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    y = DC.blobs(600)
    grid = (DC.nodes(-11.0, 10.0, 40), DC.nodes(-9.0, 10.5, 37))
    D = DC.density_ref(y, h, grid)
    X, Y = np.meshgrid(*grid)
    kd = neighbors.KernelDensity(bandwidth=h, rtol=0, atol=0).fit(y)
    S = np.exp(kd.score_samples(np.stack([X.ravel(), Y.ravel()], axis=1))).reshape(D.shape)
    live = D >= 1e-9 * D.max()
    rel = float((np.abs(S - D) / D)[live].max())
    print(f"h={h}: sklearn vs the long-double sum on {int(live.sum())} cells: largest relative difference {rel:.3e}")
    assert live.sum() > 500 and rel <= 3.6e-6


def plateau():
    """an exact plateau (the 2 x 3 block of 5s), duplicate peaks (two 7s apart, two 9s side by side) and a zero corner"""
    D = np.ones((9, 11))
    D[1:3, 1:4] = 5.0
    D[6, 2] = D[6, 8] = 7.0
    D[2, 7] = D[2, 8] = 9.0
    D[7:, 9:] = 0.0
    return D


def ridge():
    """two bumps joined by a saddle: a threshold between the saddle and the lower peak cuts the basin of neither, one above
    the lower peak removes it"""
    b, a = np.mgrid[0:21, 0:30]
    return np.exp(-((a - 8) ** 2 + (b - 10) ** 2) / 18.0) + 0.6 * np.exp(-((a - 21) ** 2 + (b - 9) ** 2) / 12.0)


GRIDS = {"constant": (np.full((7, 5), 0.25), 0.0), "two wide": (np.random.default_rng(3).random((40, 2)), 0.0),
         "two high": (np.random.default_rng(4).random((2, 33)), 0.3), "plateau": (plateau(), 0.0), "plateau cut": (plateau(), 0.5),
         "ridge": (ridge(), 0.0), "ridge cut low": (ridge(), 0.3), "ridge cut high": (ridge(), 0.7), "one cell": (np.ones((1, 1)), 0.0),
         "random": (np.random.default_rng(8).random((37, 29)), 0.2)}


@pytest.mark.parametrize("name", GRIDS)
def test_regions_equal_the_uphill_walk(name):
    from scrubvae_amd.eval import density_regions
    D, md = GRIDS[name]
    r, p = density_regions(D, min_density=md)
    rr, pp = DC.regions_ref(D, md)
    assert r.dtype == np.int32 and p.dtype == np.int64 and r.shape == D.shape and p.shape == (len(p), 2)
    assert np.array_equal(r, rr) and np.array_equal(p, pp)
    assert np.array_equal(density_regions(torch.from_numpy(D), min_density=md)[0], r)
    if name == "constant" or name == "one cell":
        assert (r == 0).all() and np.array_equal(p, [[0, 0]])
    if name == "plateau":        # each plateau is one region rooted at its lowest flat index; equal peaks numbered by flat index
        assert p.tolist()[:4] == [[2, 7], [6, 2], [6, 8], [1, 1]] and r[2, 8] == 0 and (r[1:3, 1:4] == 3).all() and (r >= 0).all()
    if name == "plateau cut":    # threshold 4.5: the ones and the zero corner are in no region
        assert len(p) == 4 and (r[D < 4.5] == -1).all() and (r[D >= 4.5] >= 0).all()
    if name == "ridge":
        assert len(p) == 2 and p.tolist() == [[10, 8], [9, 21]]
    if name == "ridge cut low":  # the threshold cuts the joined basin in two islands, both kept
        assert len(p) == 2 and (r[10, 8:22] == -1).any() and set(np.unique(r)) == {-1, 0, 1}
    if name == "ridge cut high":  # the lower peak is below the threshold: not numbered
        assert len(p) == 1 and set(np.unique(r)) == {-1, 0}


@pytest.mark.parametrize("name", ["random", "two wide", "two high", "70x33", "96x103"])
def test_roots_are_the_maximum_filter_peaks(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    from scrubvae_amd.eval import density_regions
    if name in DC.LABEL_CASES and not DC.LONGDOUBLE:
        pytest.skip("np.longdouble is no wider than fp64 here")
    D = DC.label_case(name)[4] if name in DC.LABEL_CASES else GRIDS[name][0]
    assert len(np.unique(D)) == D.size                       # tie-free
    _, p = density_regions(D)
    b, a = np.nonzero(ndimage.maximum_filter(D, size=3, mode="nearest") == D)
    assert sorted(map(tuple, p.tolist())) == sorted(zip(b.tolist(), a.tolist()))


@needs_longdouble
@pytest.mark.parametrize("name", DC.LABEL_CASES)
def test_label_cases_have_decision_margins(name):
    """What lets test_gpu_density.py demand equal regions, peaks and labels: a density within the gate of the reference everywhere
    takes every decision of density_regions as the reference does (density_checks.margins)."""
    from scrubvae_amd.eval import density_regions
    y, h, grid, md, D, G = DC.label_case(name)
    window, threshold, peaks, rel = DC.margins(D, G, md)
    print(f"{name}: window slack {window:.3e} threshold slack {threshold:.3e} peak slack {peaks:.3e}; smallest relative window gap "
          f"{rel:.3e}; largest gate / density {float((G / D).max()) / DC.EPS:.0f} u")
    assert window > 0 and threshold > 0 and peaks > 0
    r, p = density_regions(D, min_density=md)
    rr, pp = DC.regions_ref(D, md)
    assert np.array_equal(r, rr) and np.array_equal(p, pp) and len(p) == 3
    lab = DC.labels_ref(y, grid[0], grid[1], rr)
    assert set(np.unique(lab)) <= {-1, 0, 1, 2} and (np.bincount(lab[lab >= 0]) > 150).all()


def test_gate_scales_with_the_exponent():
    """far from the points the gate grows relative to the density by 6 u per unit of the exponent, and an exact zero has the floor"""
    y = np.array([[0.0, 0.0]])
    grid = (DC.nodes(0.0, 60.0, 7), DC.nodes(0.0, 1.0, 2))
    D, G = DC.ref_and_gate(y, 1.0, grid)
    arg = grid[0] ** 2 / 2.0
    live = D[0] > 0
    assert np.allclose(G[0][live] / D[0][live] / DC.EPS, 1.001 * (6 * arg + 13 + 1 / 2048)[live], rtol=1e-6)
    assert D[0, -1] == 0.0 and 0 < G[0, -1] < 1e-300


def test_bandwidth_rules(monkeypatch):
    from scrubvae_amd.eval import density as DM
    untouched(monkeypatch)
    y = DC.blobs(301)
    want = 301 ** (-1.0 / 6.0) * np.sqrt((y[:, 0].var(ddof=1) + y[:, 1].var(ddof=1)) / 2.0)
    for form in (y, torch.from_numpy(y)):
        h, rows, k = DM._den_bandwidth("scott", None, DM._den_rows(form))
        assert rows is None and k is None and abs(h - want) <= 4 * DC.EPS * want
    assert DM._den_bandwidth(0.5, None, y) == (0.5, None, None) and DM._den_bandwidth(2, None, y) == (2.0, None, None)
    assert DM._den_bandwidth("knn", 7, y) == (None, None, 7)
    hr = DC.decades(301)
    for form in (hr, torch.from_numpy(hr), hr.astype(np.float32)):
        h, rows, k = DM._den_bandwidth(form, None, y)
        assert h is None and k is None and np.array_equal(np.asarray(rows), np.asarray(form, dtype=np.float64))
    # the default extent: the bounding box widened by pad x the largest bandwidth; the nodes of the kernel
    ext = DM._den_extent(None, 3.0, y, 2.0)
    assert ext == (y[:, 0].min() - 6.0, y[:, 0].max() + 6.0, y[:, 1].min() - 6.0, y[:, 1].max() + 6.0)
    dx, xs = DM._den_nodes(-1.0, 2.0, 8)
    assert dx == 3.0 / 7 and xs.tobytes() == DC.nodes(-1.0, 2.0, 8).tobytes() == (-1.0 + np.arange(8.0) * (3.0 / 7)).tobytes()
    assert DM._den_grid_size(64) == (64, 64) and DM._den_grid_size((70, 33)) == (70, 33) and DM._den_grid_size([2, 1024]) == (2, 1024)


def test_knn_bandwidth_is_the_kth_distance(monkeypatch):
    """h_i = column n_neighbors - 1 of the neighbour distances, and a zero distance is refused (no device: the search is replaced)"""
    from scrubvae_amd.eval import density as DM
    from scrubvae_amd.eval import neighbors
    y = DC.blobs(40)
    seen = {}

    def dists(x):
        return np.sort(np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1)), axis=1)

    def fake_knn(x, k, grp, info=None):
        return torch.from_numpy(dists(np.asarray(x))[:, 1:k + 1].copy()), None

    def fake_device(x, h, h_rows, *grid, info=None):
        seen.update(h=h, rows=h_rows.numpy().copy(), grid=grid)
        return torch.zeros(grid[5], grid[2], dtype=torch.float64)

    monkeypatch.setattr(neighbors, "_knn_device", fake_knn)
    monkeypatch.setattr(DM, "_density_device", fake_device)
    g = DM.density_map(y, bandwidth="knn", n_neighbors=5, grid_size=(8, 6))
    want = dists(y)[:, 5]
    assert seen["h"] is None and np.array_equal(seen["rows"], want) and np.array_equal(g.bandwidth, want)
    assert g.density.shape == (6, 8) and g.xs[0] == y[:, 0].min() - 3.0 * want.max() and seen["grid"][0] == g.xs[0]
    with pytest.raises(ValueError, match="distance 0"):
        DM.density_map(np.concatenate([y, y[:1]]), bandwidth="knn", n_neighbors=1, grid_size=8)


def test_predict_rounds_to_the_nearest_node():
    from scrubvae_amd.eval import DensityMap
    m = DensityMap()
    with pytest.raises(RuntimeError):
        m.predict(np.zeros((1, 2)))
    m.xs_, m.ys_ = DC.nodes(0.0, 3.0, 4), DC.nodes(10.0, 12.0, 3)
    m.regions_ = np.array([[0, 0, 1, 1], [2, 2, -1, 1], [2, 2, 3, 3]], dtype=np.int32)
    pts = np.array([[0.0, 10.0], [0.49, 10.49], [0.51, 10.51], [1.5, 11.5], [2.5, 10.5], [3.0, 12.0], [2.2, 11.1],   # inside
                    [-1e-9, 10.0], [3.0000001, 11.0], [1.0, 9.99], [1.0, 12.5]])                                    # outside
    want = [0, 0, 2, 3, 1, 3, -1, -1, -1, -1, -1]            # 1.5 and 2.5 are halves: rint rounds them to the even node
    assert m.predict(pts).tolist() == want == DC.labels_ref(pts, m.xs_, m.ys_, m.regions_).tolist()
    assert m.predict(torch.from_numpy(pts).float().double()).dtype == np.int64


Y8 = DC.blobs(8)
BAD = [
    dict(y=Y8[:, 0]), dict(y=Y8[:, :1]), dict(y=np.zeros((8, 3))), dict(y=Y8[:0]), dict(y=np.where(Y8 > 5, np.nan, Y8)),
    dict(y=np.where(Y8 > 5, np.inf, Y8)),
    dict(bandwidth=0.0), dict(bandwidth=-1.0), dict(bandwidth=float("nan")), dict(bandwidth=float("inf")), dict(bandwidth=1e-170),
    dict(bandwidth=1e170), dict(bandwidth=True), dict(bandwidth="silverman"), dict(bandwidth=np.ones(7)), dict(bandwidth=np.ones((8, 1))),
    dict(bandwidth=np.r_[np.ones(7), 0.0]), dict(bandwidth=np.r_[np.ones(7), np.nan]), dict(bandwidth=-np.ones(8)),
    dict(bandwidth="scott", y=Y8[:1]), dict(bandwidth="scott", y=np.ones((8, 2))),
    dict(bandwidth="knn"), dict(bandwidth="knn", n_neighbors=0), dict(bandwidth="knn", n_neighbors=8), dict(bandwidth="knn", n_neighbors=2.0),
    dict(bandwidth="knn", n_neighbors=91, y=np.zeros((200, 2))), dict(n_neighbors=3), dict(bandwidth=1.0, n_neighbors=3),
    dict(grid_size=1), dict(grid_size=1025), dict(grid_size=(64, 1)), dict(grid_size=(64, 2000)), dict(grid_size=64.0), dict(grid_size=(8, 8, 8)),
    dict(grid_size="64"), dict(grid_size=True),
    dict(extent=(0, 0, 0, 1)), dict(extent=(1, 0, 0, 1)), dict(extent=(0, 1, 2, 2)), dict(extent=(0, 1, 0)), dict(extent=(0, 1, 0, np.inf)),
    dict(extent=(0, np.nan, 0, 1)), dict(extent="box"), dict(pad=-1.0), dict(pad=float("nan")), dict(pad=None),
]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(b))
def test_argument_errors_before_device_work(bad, monkeypatch):
    """a ValueError before the library is touched: loading it fails the test"""
    from scrubvae_amd.eval import DensityMap, density_map
    untouched(monkeypatch)
    kw = dict(bandwidth=1.0, grid_size=16)
    kw.update(bad)
    y = kw.pop("y", Y8)
    with pytest.raises(ValueError):
        density_map(y, **kw)
    with pytest.raises(ValueError):
        density_map(torch.from_numpy(np.ascontiguousarray(y)), **kw)
    with pytest.raises(ValueError):
        DensityMap(**kw).fit(y)


def test_region_argument_errors():
    from scrubvae_amd.eval import DensityMap, density_regions
    for D in (np.ones(4), np.ones((2, 2, 2)), np.array([[1.0, np.nan]]), np.array([[1.0, np.inf]]), np.zeros((0, 3)), np.array([["a"]])):
        with pytest.raises(ValueError):
            density_regions(D)
    for md in (-0.1, 1.5, None, "0.1", float("nan")):
        with pytest.raises(ValueError):
            density_regions(np.ones((3, 3)), min_density=md)
        with pytest.raises(ValueError):
            DensityMap(bandwidth=1.0, min_density=md).fit(Y8)


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    lib = _lib.lib()
    work, G = lib.svae_density_work, _lib.DENSITY_MAX_GRID
    assert G == 1024
    assert work(0, 8, 8) == 0 and work(-1, 8, 8) == 0 and work(10, 1, 8) == 0 and work(10, 8, 1) == 0 and work(10, G + 1, 8) == 0
    assert work(10, 8, G + 1) == 0 and work(2 ** 30 + 1, 8, 8) == 0
    # slices x gy x gx x 8 bytes of partial grids + n x 16 bytes of per-point factors; the slices from (n, gx, gy) alone
    for n, gx, gy in ((1, 2, 2), (63, 70, 33), (1037, 96, 103), (4127, 2, 2), (4127, 300, 2), (130, G, G), (10 ** 6, 512, 512), (2 ** 30, 2, 2)):
        assert work(n, gx, gy) == DC.slices(n, gx, gy)[0] * gx * gy * 8 + 16 * n, (n, gx, gy)
    assert DC.slices(1, 2, 2) == (1, 1) and DC.slices(63, 70, 33) == (2, 1) and DC.slices(4127, 2, 2) == (65, 2)
    assert DC.slices(130, G, G) == (5, 1) and DC.slices(10 ** 6, 512, 512) == (32, 977) and DC.slices(4127, 300, 2) == (65, 2)
    fake, E = 4096, _lib.ERR_ARG

    def grid(Y=fake, ld=2, n=40, rows=None, h=1.0, x0=0.0, dx=0.5, gx=8, y0=0.0, dy=0.5, gy=8, w=fake, D=fake):
        return lib.svae_density_grid(Y, ld, n, rows, h, x0, dx, gx, y0, dy, gy, w, D, None)

    for bad, text in ((dict(Y=None), "bad rows"), (dict(ld=1), "bad rows"), (dict(n=0), "bad rows"), (dict(n=2 ** 30 + 1), "bad rows"),
                      (dict(gx=1), "bad grid"), (dict(gy=G + 1), "bad grid"), (dict(dx=0.0), "grid steps"), (dict(dy=-1.0), "grid steps"),
                      (dict(dx=float("nan")), "grid steps"), (dict(dy=float("inf")), "grid steps"), (dict(x0=float("inf")), "grid steps"),
                      (dict(y0=float("nan")), "grid steps"), (dict(h=0.0), "bandwidth"), (dict(h=-2.0), "bandwidth"),
                      (dict(h=float("nan")), "bandwidth"), (dict(h=1e-170), "bandwidth"), (dict(h=1e170), "bandwidth"),
                      (dict(w=None), "null"), (dict(D=None), "null")):
        assert grid(**bad) == E and text in _lib.last_error(), (bad, _lib.last_error())
    for bad in (dict(w=fake + 8), dict(D=fake + 4), dict(w=fake + 8, rows=fake)):
        assert grid(**bad) == _lib.ERR_ALIGN and "aligned" in _lib.last_error(), bad
    import scrubvae_amd.eval as EV
    for name in ("density_map", "density_regions", "DensityMap", "DensityGrid"):
        assert callable(getattr(EV, name))
    from scrubvae_amd.eval import density as DM
    assert DM._DENSITY_CALLS.keys() >= {"grid"}
    assert DC.TILE == 128 and DC.CHUNK == 32


def test_header_and_sources_name_the_new_pieces():
    from scrubvae_amd import build
    assert "density.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "density.hip"))
    with open(os.path.join(build.CSRC, "density.hip")) as f:
        src = f.read()
    for name, value in (("DEN_T", DC.TILE), ("DEN_CHUNK", DC.CHUNK), ("DEN_MAX_SLICES", DC.MAX_SLICES), ("DEN_BLOCKS", DC.BLOCKS)):
        assert re.search(rf"constexpr int {name} = {value};", src), name
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in src and "fixed_sum.h" in src and "asm" not in src


def test_density_needs_the_built_library(monkeypatch, tmp_path):
    """no fallback: without the library the density fails at its first load, it is not computed on the host"""
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import density as DM
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libscrubvae_hip.so"))
    monkeypatch.setattr(DM, "_device_of", lambda x: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    with pytest.raises(RuntimeError, match="not found"):
        DM._density_device(torch.from_numpy(Y8), 1.0, None, 0.0, 1.0, 4, 0.0, 1.0, 4)
