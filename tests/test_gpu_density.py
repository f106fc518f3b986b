"""density_map / DensityMap (csrc/density.hip) on the device against the long-double restatement of tests/density_checks.py.

Every cell is held to density_gate, the bound derived there from the kernel's arithmetic (6 u per unit of the exponent + 13 u + the
(n - 1) u of any summation order + an underflow floor).  The sizes are the smallest that reach each path of the kernel, whose
constants are a 128 x 128 tile, 32 points per chunk (two stages of 16, one in each LDS buffer) and at most 128 slices of the points while the grid holds fewer than 512 blocks
(density_checks.slices restates the plan):
    n = 1, 2, 20   a single partial chunk          n = 64      two full chunks, an exact multiple
    n = 63         two slices, the last partial    n = 65      three slices, the last of one point
    n = 130, 1037  5 and 33 slices of one chunk    n = 4127    129 chunks: 65 slices of two chunks, the last of one partial chunk
and the grids 2 x 2, 70 x 33 and 96 x 103 (one partial tile, both ways, non-square), 130 x 130 (2 x 2 tiles, every position of a
full tile, edge tiles of two cells) and 1024 x 1024 (64 tiles, 5 slices)."""
import numpy as np
import pytest
import torch

from tests import density_checks as DC

pytestmark = pytest.mark.gpu
needs_longdouble = pytest.mark.skipif(not DC.LONGDOUBLE, reason="np.longdouble is no wider than fp64 here: no truth to hold the value to")

BOX = (-11.0, 10.5, -9.5, 10.25)      # holds the three blobs
INNER = (-3.0, 3.5, -2.0, 3.0)        # between them: nearly every point lies outside

#         n     gx   gy   bandwidth   extent
CASES = [(1, 2, 2, "one", BOX),
         (2, 70, 33, "rows", BOX),
         (20, 130, 130, "one", BOX),
         (63, 96, 103, "one", BOX),
         (64, 70, 33, "rows", BOX),
         (65, 70, 33, "rows", INNER),
         (130, 96, 103, "rows", BOX),
         (1037, 70, 33, "one", INNER),
         (1037, 96, 103, "rows", BOX),
         (4127, 2, 2, "one", BOX),
         (4127, 70, 33, "rows", BOX)]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def bandwidth(kind, n):
    return 0.7 if kind == "one" else DC.decades(n)


def grid_of(extent, gx, gy):
    return DC.nodes(extent[0], extent[1], gx), DC.nodes(extent[2], extent[3], gy)


def held(name, got, ref, gate):
    """print the worst error / gate, then hold every cell"""
    err = np.abs(got.astype(np.longdouble) - ref.astype(np.longdouble)).astype(np.float64)
    worst = int(np.argmax(err / gate))
    print(f"density {name}: largest error / gate {float((err / gate).max()):.4f} (error {err.reshape(-1)[worst]:.3e}, value "
          f"{ref.reshape(-1)[worst]:.3e}, gate {gate.reshape(-1)[worst]:.3e}); largest relative error "
          f"{float(np.max(err[ref > 0] / ref[ref > 0]) / DC.EPS) if (ref > 0).any() else 0.0:.1f} u")
    assert np.isfinite(got).all() and (got >= 0).all()
    assert (err <= gate).all(), (name, worst, float(err.reshape(-1)[worst]), float(gate.reshape(-1)[worst]))


@needs_longdouble
@pytest.mark.parametrize("n,gx,gy,kind,extent", CASES)
def test_every_cell_within_the_derived_gate(n, gx, gy, kind, extent):
    from scrubvae_amd.eval import density as DM
    y, h = DC.blobs(n), bandwidth(kind, n)
    grid = grid_of(extent, gx, gy)
    before = DM._DENSITY_CALLS["grid"]
    g = DM.density_map(y, bandwidth=h, grid_size=(gx, gy), extent=extent)
    assert DM._DENSITY_CALLS["grid"] == before + 1
    assert DM._DENSITY_LAST["work"] == DC.slices(n, gx, gy)[0] * gx * gy * 8 + 16 * n
    assert g.density.shape == (gy, gx) and g.density.dtype == np.float64
    assert bits(g.xs) == bits(grid[0]) and bits(g.ys) == bits(grid[1]) and np.array_equal(g.bandwidth, h)
    ref, gate = DC.ref_and_gate(y, h, grid)
    held(f"n={n} {gx}x{gy} {kind}", g.density, ref, gate)


@needs_longdouble
def test_full_grid_of_1024():
    """64 tiles, 5 slices.  The long-double sum of all 2^20 cells would take 8 s, so the reference is taken at 50,000 cells drawn
    uniformly (every position within a tile and every tile many times over), the four corners and the cells on both sides of
    every tile boundary along two lines; the whole array is checked for range."""
    from scrubvae_amd.eval import density_map
    n, G = 130, 1024
    y, h = DC.blobs(n), 0.7
    g = density_map(y, bandwidth=h, grid_size=G, extent=BOX)
    rng = np.random.default_rng(11)
    edge = np.array([v for k in range(1, 8) for v in (128 * k - 1, 128 * k)])
    b = np.concatenate([rng.integers(0, G, 50000), [0, 0, G - 1, G - 1], edge, np.full(len(edge), 517)])
    a = np.concatenate([rng.integers(0, G, 50000), [0, G - 1, 0, G - 1], np.full(len(edge), 300), edge])
    ref, gate = DC.ref_and_gate(y, h, grid_of(BOX, G, G), cells=(b, a))
    held("n=130 1024x1024", g.density[b, a], ref, gate)
    assert g.density.shape == (G, G) and np.isfinite(g.density).all() and (g.density >= 0).all()
    assert g.density.max() <= 1.0 / (2.0 * np.pi * h * h)


@needs_longdouble
def test_far_tiles_are_exactly_zero():
    """a grid that runs away from the points: the near corner holds values, whole tiles far out are exactly 0 (every term
    underflows), and a grid nowhere near any point is 0 everywhere.  The gate has no division: zeros compare clean."""
    from scrubvae_amd.eval import density_map
    y = DC.blobs(65)
    extent = (0.0, 300.0, 0.0, 310.0)
    g = density_map(y, bandwidth=1.0, grid_size=(256, 140), extent=extent)
    ref, gate = DC.ref_and_gate(y, 1.0, grid_of(extent, 256, 140))
    held("far 256x140", g.density, ref, gate)
    assert (g.density[:, 128:] == 0).all() and (g.density[128:, :] == 0).all() and g.density[0, 0] > 0
    rows = DC.decades(65)
    far = density_map(y, bandwidth=rows * 0.01, grid_size=(70, 33), extent=(500.0, 700.0, 500.0, 650.0))
    assert (far.density == 0).all()


def test_inputs_of_every_kind_give_the_fp64_result():
    from scrubvae_amd.eval import density_map
    n = 130
    y32 = DC.blobs(n).astype(np.float32)
    y = y32.astype(np.float64)
    rows = DC.decades(n)
    kw = dict(grid_size=(70, 33), extent=BOX)
    for h in (0.7, rows):
        want = density_map(y, bandwidth=h, **kw)
        assert bits(density_map(y, bandwidth=h, **kw).density) == bits(want.density)                       # two calls
        for form in (y32, torch.from_numpy(y32), torch.from_numpy(y), torch.from_numpy(y).cuda(), torch.from_numpy(y32).cuda(),
                     np.asfortranarray(y)):
            assert bits(density_map(form, bandwidth=h, **kw).density) == bits(want.density)
        # rows with ld = 4: a column slice of a wider device tensor, read in place
        wide = torch.zeros(n, 4, dtype=torch.float64, device="cuda")
        wide[:, 1:3] = torch.from_numpy(y).cuda()
        wide[:, 0], wide[:, 3] = float("nan"), 1e300
        view = wide[:, 1:3]
        assert view.stride() == (4, 1)
        assert bits(density_map(view, bandwidth=h, **kw).density) == bits(want.density)
    hd = torch.from_numpy(rows).cuda()
    assert bits(density_map(y, bandwidth=hd, **kw).density) == bits(density_map(y, bandwidth=rows.astype(np.float64), **kw).density)
    # "scott" and "knn" go through the same launch: their bandwidths, then equal bytes with the bandwidth given outright
    s = density_map(y, grid_size=(70, 33))
    hs = n ** (-1.0 / 6.0) * np.sqrt((y[:, 0].var(ddof=1) + y[:, 1].var(ddof=1)) / 2.0)
    assert abs(s.bandwidth - hs) <= 4 * DC.EPS * hs and s.xs[0] == y[:, 0].min() - 3.0 * s.bandwidth
    assert bits(density_map(y, bandwidth=s.bandwidth, grid_size=(70, 33)).density) == bits(s.density)
    k = density_map(y, bandwidth="knn", n_neighbors=7, grid_size=(70, 33))
    from scrubvae_amd.eval import kneighbors
    dist, _ = kneighbors(y, 7)
    assert np.array_equal(k.bandwidth, dist[:, 6]) and bits(density_map(y, bandwidth=dist[:, 6], grid_size=(70, 33)).density) == bits(k.density)
    assert bits(density_map(torch.from_numpy(y).cuda(), bandwidth="knn", n_neighbors=7, grid_size=(70, 33)).density) == bits(k.density)


@needs_longdouble
@pytest.mark.parametrize("name", DC.LABEL_CASES)
def test_density_map_labels_equal_the_restatement(name):
    """the cases whose decision margins test_density_cpu.py asserts: within the gate, every decision is the reference's"""
    from scrubvae_amd.eval import DensityMap, density_regions
    y, h, grid, md, D, G = DC.label_case(name)
    gx, gy = len(grid[0]), len(grid[1])
    m = DensityMap(bandwidth=h, grid_size=(gx, gy), min_density=md)
    lab = m.fit_predict(torch.from_numpy(y.copy()).cuda())
    assert bits(m.xs_) == bits(grid[0]) and bits(m.ys_) == bits(grid[1]) and m.bandwidth_ == h
    held(f"labels {name}", m.density_, D, G)
    rr, pp = DC.regions_ref(D, md)
    assert np.array_equal(m.regions_, rr) and m.regions_.dtype == np.int32
    assert np.array_equal(m.peaks_, np.stack([grid[0][pp[:, 1]], grid[1][pp[:, 0]]], axis=1)) and len(m.peaks_) == 3
    want = DC.labels_ref(y, grid[0], grid[1], rr)
    assert np.array_equal(m.labels_, want) and lab is m.labels_ and m.labels_.dtype == np.int64
    assert m.region_counts_.shape == (3,) and m.region_counts_.sum() == (want >= 0).sum() and (m.region_counts_ > 150).all()
    assert np.array_equal(m.predict(y), m.labels_) and np.array_equal(m.predict(y[:7].astype(np.float32).astype(np.float64)).shape, (7,))
    # the vectorised regions of the device density equal the uphill walk of that same array
    r, p = density_regions(m.density_, min_density=md)
    r2, p2 = DC.regions_ref(m.density_, md)
    assert np.array_equal(r, r2) and np.array_equal(p, p2) and np.array_equal(r, m.regions_)


def test_tsne_then_density_map_then_silhouette():
    """the three-line use: 600 rows of three separated Gaussians in 5 dimensions, embedded by the 250 exploration iterations of
    TSNE (the fewest it allows; they already separate the blobs), cut into regions, scored"""
    from scrubvae_amd.eval import TSNE, DensityMap, silhouette_score
    g = np.random.default_rng(2)
    which = np.arange(600) // 200
    z = 8.0 * np.eye(3, 5)[which] + g.normal(size=(600, 5))
    info = {}
    emb = TSNE(max_iter=250, random_state=0).fit_transform(z)
    m = DensityMap(min_density=0.05).fit(emb, info=info)
    print(f"t-SNE -> density map: bandwidth {m.bandwidth_:.4f}, regions {len(m.peaks_)}, counts {m.region_counts_.tolist()}, "
          f"noise {(m.labels_ < 0).sum()}, density launch {info['density_s'] * 1e3:.2f} ms")
    assert len(m.peaks_) == 3 and m.density_.shape == (256, 256)
    kept = m.labels_ >= 0
    assert kept.sum() >= 540
    for c in range(3):            # each blob falls in one region
        assert len(np.unique(m.labels_[kept & (which == c)])) == 1
    score = silhouette_score(z, m.labels_, noise_label=-1)
    print(f"silhouette of the regions in latent space {score:.4f}")
    assert score > 0.5
