"""mmd_estimate / mmd_bandwidth (csrc/mmd.hip) and lda_rand_cv (csrc/decode.hip) on the device against the numpy restatements of
tests/mmd_checks.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import decode_checks as DC
from tests import mmd_checks as MC
from tests.mmd_checks import class_rows, two_sets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(3001, 2003, 32), (2048, 2048, 128), (4099, 7, 1), (2, 2, 37), (1500, 1501, 3)]
needs_longdouble = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63,
                                      reason="np.longdouble is no wider than fp64 here: no truth to hold the value to")


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.mark.parametrize("nx,ny,d", SIZES)
def test_bandwidth_is_bit_equal(nx, ny, d):
    from scrubvae_amd.eval import mmd_bandwidth
    X, Y = two_sets(nx, ny, d, seed=nx + d)
    want = MC.bandwidth(X, Y)
    got = mmd_bandwidth(X, Y)
    assert isinstance(got, float) and same_bits(got, want), (got, want)
    assert same_bits(mmd_bandwidth(torch.from_numpy(X).cuda(), torch.from_numpy(Y)), want)


def tied_sets(name):
    X, Y = two_sets(900, 700, 16, seed=5)
    if name == "constant_column":
        X[:, 3] = Y[:, 3] = 2.5
    elif name == "copies":            # 600 copies of one row: 179 700 zero distances, and ties through every bin above
        X[:400] = X[500]
        Y[:200] = X[500]
    elif name == "grid":              # few distinct values per feature: the median is a heavily tied value
        X, Y = np.round(X[:, :2]), np.round(Y[:, :2])
    return X, Y


@pytest.mark.parametrize("name", ["constant_column", "copies", "grid"])
def test_bandwidth_is_bit_equal_through_ties(name):
    from scrubvae_amd.eval import mmd_bandwidth
    X, Y = tied_sets(name)
    want = MC.bandwidth(X, Y)
    assert want > 0
    assert same_bits(mmd_bandwidth(X, Y), want)


def test_zero_median_gives_zero_bandwidth_and_nan():
    from scrubvae_amd.eval import mmd_bandwidth, mmd_estimate
    X, Y = two_sets(40, 13, 5, seed=2)
    X[:] = X[0]
    Y[:10] = X[0]                     # 50 of 53 rows coincide: 1225 of 1378 pairs are 0
    assert MC.bandwidth(X, Y) == 0.0
    assert same_bits(mmd_bandwidth(X, Y), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.isnan(MC.mmd(X, Y, 0.0))
    assert np.isnan(mmd_estimate(X, Y))


def test_bandwidth_rank_at_a_large_size():
    """20 011 + 12 007 rows x 32: M = 512 560 153 (odd), so med is one of the distances and its rank is proved by counting"""
    from scrubvae_amd.eval import metrics as M
    X, Y = two_sets(20011, 12007, 32, seed=11)
    n = len(X) + len(Y)
    pairs = n * (n - 1) // 2
    assert pairs % 2 == 1
    info = {}
    h, _ = M._mmd_device(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), None, True, info)
    med = info["med"]
    assert same_bits(h, med * med)
    lt, le = MC.rank_counts(np.vstack([X, Y]), med)
    assert lt <= pairs // 2 < le, (lt, le, pairs // 2)


@needs_longdouble
@pytest.mark.parametrize("nx,ny,d", SIZES)
def test_estimate_within_eight_reference_errors(nx, ny, d):
    from scrubvae_amd.eval import metrics as M
    X, Y = two_sets(nx, ny, d, seed=nx + d)
    h = MC.bandwidth(X, Y)
    truth, tol, u = MC.mmd_gate(X, Y, h)
    before = dict(M._MMD_CALLS)
    got = M.mmd_estimate(X, Y)
    assert M._MMD_CALLS["select"] == before["select"] + 1 and M._MMD_CALLS["sums"] == before["sums"] + 1
    err = abs(float(np.longdouble(got) - truth))
    print(f"mmd_estimate nx={nx} ny={ny} d={d}: value {got:.6e}, device error {err / u:.2f} u, gate {tol / u:.2f} u")
    assert isinstance(got, float) and err <= tol, (got, float(truth), err / u, tol / u)


@needs_longdouble
@pytest.mark.parametrize("nx,ny,d,h", [(3001, 2003, 32, 10.0), (1500, 1501, 3, 0.37), (2048, 2048, 128, 4000)])
def test_estimate_with_a_given_bandwidth_runs_no_select(nx, ny, d, h):
    from scrubvae_amd.eval import metrics as M
    X, Y = two_sets(nx, ny, d, seed=nx + d)
    truth, tol, u = MC.mmd_gate(X, Y, h)
    before = dict(M._MMD_CALLS)
    got = M.mmd_estimate(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), h)
    assert M._MMD_CALLS["select"] == before["select"] and M._MMD_CALLS["sums"] == before["sums"] + 1
    err = abs(float(np.longdouble(got) - truth))
    print(f"mmd_estimate nx={nx} ny={ny} d={d} h={h}: value {got:.6e}, device error {err / u:.2f} u, gate {tol / u:.2f} u")
    assert err <= tol, (got, float(truth), err / u, tol / u)


@needs_longdouble
def test_estimate_of_a_set_against_its_copy():
    """not exactly 0: the across mean includes the zero-distance pairs (i, i)"""
    from scrubvae_amd.eval import mmd_estimate
    X, _ = two_sets(1777, 2, 32, seed=4)
    h = MC.bandwidth(X, X.copy())
    truth, tol, u = MC.mmd_gate(X, X.copy(), h)
    got = mmd_estimate(X, X.copy())
    assert truth != 0 and abs(float(np.longdouble(got) - truth)) <= tol, (got, float(truth), tol)


def test_estimate_is_bit_reproducible():
    from scrubvae_amd.eval import mmd_estimate
    X, Y = two_sets(3001, 2003, 32, seed=8)   # float32-representable values
    a = mmd_estimate(X, Y)
    assert same_bits(a, mmd_estimate(X, Y))
    xd, yd = torch.from_numpy(X.astype(np.float32)).cuda(), torch.from_numpy(Y.astype(np.float32)).cuda()
    assert same_bits(a, mmd_estimate(xd, yd))
    assert same_bits(mmd_estimate(X, Y, 50.0), mmd_estimate(xd, yd, 50.0))


@pytest.mark.parametrize("degenerate", [False, True])
def test_lda_rand_cv_matches_restatement(degenerate):
    from scrubvae_amd.eval import metrics as M
    x, y = class_rows(20000, 32, 4, seed=3, degenerate=degenerate)
    out = M._lda(torch.from_numpy(x).cuda(), y, 1, 5, want_rows=True)
    near, accs, smallest = 0, [], len(x)
    for f, (tr, te) in enumerate(DC.kfold_split(len(x), 5)):
        sc = MC.lda_scores(x[tr], y[tr], x[te], np.arange(4))
        pred = sc.argmax(1)
        srt = np.sort(sc, 1)
        clear = (srt[:, -1] - srt[:, -2]) > 1e-6
        near += (~clear).sum()
        smallest = min(smallest, len(te))
        assert np.array_equal(out["pred"][te][clear], pred[clear]), f
        accs.append((pred == y[te]).mean())
    assert near < 1e-3 * len(x)
    assert np.abs(np.array(out["acc"]) - accs).max() <= near / smallest + 1e-12
    assert M.lda_rand_cv(x, y, window=1, folds=5) == out["acc"]
    assert M.lda_rand_cv(np.repeat(x, 3, axis=0), np.repeat(y, 3), window=3, folds=5) == out["acc"]  # the window downsample


def test_product_path_does_not_need_scipy_sklearn_pandas():
    code = (
        "import sys\n"
        "for m in ('scipy', 'sklearn', 'pandas'): sys.modules[m] = None\n"
        "import numpy as np\n"
        "from scrubvae_amd.eval import mmd_estimate, mmd_bandwidth, lda_rand_cv, hungarian_match, shannon_entropy\n"
        "g = np.random.default_rng(0); x = g.normal(size=(400, 8)).astype(np.float32); y = x[:300] + 0.5\n"
        "c = g.integers(0, 3, 400)\n"
        "v = mmd_estimate(x, y); assert np.isfinite(v) and v > 0, v\n"
        "assert mmd_estimate(x, y, mmd_bandwidth(x, y)) == v\n"
        "assert len(lda_rand_cv(x, c, window=1, folds=5)) == 5\n"
        "assert (hungarian_match(c, (c + 1) % 3) == (c + 1) % 3).all() and shannon_entropy(c) > 1.0\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
