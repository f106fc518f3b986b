"""MMD, LDA and label matching without a GPU: the restatements of tests/mmd_checks.py pinned to scipy, sklearn and pandas, the host
functions of scrubvae_amd/eval/metrics.py against the reference's recipes, argument errors and the C-ABI exports."""
import numpy as np
import pytest

from tests import mmd_checks as MC
from tests.mmd_checks import class_rows, two_sets


def reference_distances(X, Y):
    sd = pytest.importorskip("scipy.spatial.distance")
    return sd.pdist(X, metric="euclidean"), sd.pdist(Y, metric="euclidean"), sd.cdist(X, Y, metric="euclidean").ravel()


def reference_mmd(X, Y, h=None):
    """the reference's recipe, with scipy"""
    xd, yd, xyd = reference_distances(X, Y)
    if h is None:
        h = np.median(np.concatenate((xd, yd, xyd))) ** 2
    return np.mean(np.exp(-(xd ** 2) / h)) + np.mean(np.exp(-(yd ** 2) / h)) - 2 * np.mean(np.exp(-(xyd ** 2) / h))


@pytest.mark.parametrize("d", [1, 3, 32, 37, 128])
def test_pair_dist_is_scipys(d):
    X, Y = two_sets(211, 190, d, seed=d)
    xd, yd, xyd = reference_distances(X, Y)
    assert np.array_equal(MC.upper(MC.pair_dist(X, X)), xd)
    assert np.array_equal(MC.upper(MC.pair_dist(Y, Y)), yd)
    assert np.array_equal(MC.pair_dist(X, Y).ravel(), xyd)


@pytest.mark.parametrize("nx,ny,odd", [(301, 257, True), (300, 257, False), (256, 256, False)])
def test_bandwidth_is_the_reference_median(nx, ny, odd):
    X, Y = two_sets(nx, ny, 32, seed=nx)
    n = nx + ny
    assert (n * (n - 1) // 2) % 2 == int(odd)
    xd, yd, xyd = reference_distances(X, Y)
    assert MC.bandwidth(X, Y) == np.median(np.concatenate((xd, yd, xyd))) ** 2


@pytest.mark.parametrize("nx,ny,d", [(301, 257, 32), (500, 40, 3), (64, 700, 128)])
def test_mmd_restatement_matches_the_reference_recipe(nx, ny, d):
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble is no wider than fp64 here: no truth to measure the reference's own error against")
    X, Y = two_sets(nx, ny, d, seed=d)
    for h in (None, 3.7):
        hh = MC.bandwidth(X, Y) if h is None else h
        truth, tol, u = MC.mmd_gate(X, Y, hh)
        ref = reference_mmd(X, Y, h)
        got = MC.mmd(X, Y, hh)
        print(f"nx={nx} ny={ny} d={d} h={hh:.6g}: |restatement - recipe| = {abs(got - ref) / u:.2f} u, "
              f"|recipe - truth| = {abs(float(np.longdouble(ref) - truth)) / u:.2f} u")
        assert abs(got - ref) <= tol
        assert abs(float(np.longdouble(got) - truth)) <= tol


@pytest.mark.parametrize("degenerate", [False, True])
def test_lda_scores_predict_like_sklearn(degenerate):
    da = pytest.importorskip("sklearn.discriminant_analysis")
    from tests import decode_checks as DC
    x, y = class_rows(20000, 32, 4, seed=3, degenerate=degenerate)
    near = 0
    for tr, te in DC.kfold_split(len(x), 5):
        sc = MC.lda_scores(x[tr], y[tr], x[te], np.arange(4))
        srt = np.sort(sc, 1)
        clear = (srt[:, -1] - srt[:, -2]) > 1e-6
        near += (~clear).sum()
        pred = da.LinearDiscriminantAnalysis().fit(x[tr].astype(np.float64), y[tr]).predict(x[te].astype(np.float64))
        assert np.array_equal(sc.argmax(1)[clear], pred[clear])
    assert near < 1e-3 * len(x)


def reference_match(x1, x2):
    """the reference's hungarian_match, with pandas and scipy"""
    pd = pytest.importorskip("pandas")
    so = pytest.importorskip("scipy.optimize")
    cost = np.array(pd.crosstab(x1, x2))
    row_ind, col_ind = so.linear_sum_assignment(cost, maximize=True)
    row_k, col_v = np.unique(x1)[row_ind], np.unique(x2)[col_ind]
    idx = np.searchsorted(row_k, x1)
    idx[idx == len(row_k)] = 0
    return np.where(row_k[idx] == x1, col_v[idx], x1), cost, row_ind, col_ind


def planted_labels(n, k1, k2, seed, noise=0.15):
    """x2 = a relabelling of x1 (k1 labels onto k2 label values that are not 0..K-1), `noise` of the rows redrawn"""
    g = np.random.default_rng(seed)
    names1 = np.sort(g.choice(np.arange(-5, 60), k1, replace=False))
    names2 = np.sort(g.choice(np.arange(100, 190), k2, replace=False))
    a = g.integers(0, k1, n)
    b = g.permutation(max(k1, k2))[a] % k2
    redraw = g.random(n) < noise
    b[redraw] = g.integers(0, k2, redraw.sum())
    return names1[a], names2[b]


@pytest.mark.parametrize("k1,k2", [(6, 6), (5, 8), (8, 5), (1, 4), (4, 1)])
def test_hungarian_match_is_the_reference_on_unique_optima(k1, k2):
    from scrubvae_amd.eval import hungarian_match
    x1, x2 = planted_labels(3000, k1, k2, seed=10 * k1 + k2)
    want, cost, _, _ = reference_match(x1, x2)
    r1, r2, table = MC.crosstab(x1, x2)
    assert np.array_equal(table, cost) and len(r1) == k1 and len(r2) == k2
    best, ways = MC.assignment_total(table)
    assert ways == 1  # the data must not depend on a tie order
    assert np.array_equal(hungarian_match(x1, x2), want)
    assert np.array_equal(hungarian_match(list(x1), list(x2)), want)


@pytest.mark.parametrize("k1,k2", [(30, 25), (25, 30), (1, 12), (12, 1), (40, 40)])
def test_assignment_reaches_scipys_total(k1, k2):
    so = pytest.importorskip("scipy.optimize")
    from scrubvae_amd.eval.metrics import max_weight_assignment
    x1, x2 = planted_labels(20000, k1, k2, seed=k1 + k2, noise=0.6)
    _, _, table = MC.crosstab(x1, x2)
    rows, cols = max_weight_assignment(table)
    r, c = so.linear_sum_assignment(table, maximize=True)
    assert len(rows) == min(table.shape) and len(set(rows)) == len(rows) and len(set(cols)) == len(cols)
    assert table[rows, cols].sum() == table[r, c].sum()
    g = np.random.default_rng(k1)
    for shape in ((7, 5), (5, 7), (8, 8), (1, 6)):  # small tables with many ties, against brute force
        t = g.integers(0, 4, shape)
        rows, cols = max_weight_assignment(t)
        assert t[rows, cols].sum() == MC.assignment_total(t)[0]


def test_shannon_entropy_is_the_reference_formula():
    from scrubvae_amd.eval import shannon_entropy
    g = np.random.default_rng(0)
    x = g.choice([-3, 0, 4, 17, 90], size=5000, p=[0.5, 0.2, 0.15, 0.1, 0.05])
    counts = np.unique(x, return_counts=True)[1]
    hist = counts / counts.sum()
    assert shannon_entropy(x) == (hist * np.log(1 / hist)).sum()
    assert shannon_entropy(np.zeros(10)) == 0.0
    assert abs(shannon_entropy(np.arange(8)) - np.log(8)) < 1e-15


OK2 = np.zeros((4, 3))


@pytest.mark.parametrize("X,Y,h", [
    (np.zeros((1, 3)), OK2, None),
    (OK2, np.zeros((1, 3)), None),
    (OK2, np.zeros((4, 2)), None),
    (np.zeros(4), OK2, None),
    (np.array([[0.0, 1.0, 2.0], [np.nan, 1.0, 0.0]]), OK2, None),
    (OK2, np.array([[0.0, 1.0, 2.0], [np.inf, 1.0, 0.0]]), 1.0),
    (OK2, OK2, 0.0),
    (OK2, OK2, -1.0),
    (OK2, OK2, float("nan")),
    (OK2, OK2, float("inf")),
    (OK2, OK2, "1"),
])
def test_mmd_argument_errors_before_device_work(X, Y, h):
    """this machine has no device: a ValueError, not the "no device is available" RuntimeError, shows the order"""
    from scrubvae_amd.eval import mmd_bandwidth, mmd_estimate
    with pytest.raises(ValueError):
        mmd_estimate(X, Y, h)
    if h is None:
        with pytest.raises(ValueError):
            mmd_bandwidth(X, Y)


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    lib = _lib.lib()
    assert lib.svae_mmd_blocks(1) == 0 and lib.svae_mmd_blocks(64) == 1 and lib.svae_mmd_blocks(65) == 4
    import scrubvae_amd.eval as E
    for name in ("mmd_estimate", "mmd_bandwidth", "lda_rand_cv", "hungarian_match", "shannon_entropy"):
        assert callable(getattr(E, name))
