"""hsic / hsic_permutation_test (csrc/hsic.hip) on the device against the numpy restatement of tests/hsic_checks.py.

The statistic and every null value are held to the project's gate for these estimators (hsic_checks.gate_of, mmd_checks.mmd_gate
carried over): |device - truth| <= 8 max(e_ref, u), truth in np.longdouble, e_ref the fp64 restatement's own error,
u = 2^-53 (|t1| + |t2| + |t3|) of the estimator's three terms.  The kernel takes HSIC_PERMS permutations per block, the module
_HSIC_LAUNCH per launch, and a row tile's column tiles are split over at most 8 blocks."""
import numpy as np
import pytest
import torch

from tests import hsic_checks as HC
from tests.test_gpu_mmd import needs_longdouble, same_bits

pytestmark = pytest.mark.gpu

from scrubvae_amd import _lib  # noqa: E402

PC = _lib.HSIC_PERMS
#         n,   d,  q,               P
SIZES = [(301, 3, 2, 999),
         (130, 37, 1, PC + 1),                 # partial feature chunk; P one past a chunk boundary
         (131, 128, _lib.HSIC_MAX_Y, 65),      # rows not resident in LDS; widest y
         (4, 5, 1, 1),                         # the minimum for the unbiased form
         (40, 5, 3, 3),                        # one partial tile
         (1030, 1, 1, 17)]                     # more than 16 row tiles: the column range of a row tile is split over blocks
LABEL_SIZES = [SIZES[0], SIZES[-1]]


def same_array_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def report(name, got, truth, tol, u):
    err = HC.err_of(got, truth)
    worst = int(np.argmax(err / u))
    print(f"hsic {name}: {len(err)} values, worst device error {err[worst] / u[worst]:.2f} u (gate there "
          f"{tol[worst] / u[worst]:.2f} u), largest error / gate {np.max(err / tol):.3f}")
    return err


def check_case(z, y, P, seed, name):
    """statistic and null of both estimators within the gate; the matrices are built once"""
    from scrubvae_amd.eval import hsic_permutation_test
    n = len(z)
    labels = np.asarray(y).dtype.kind in "iu"
    hz, hy = HC.bandwidth(z), (None if labels else HC.bandwidth(y))
    K, L = HC.kernel_matrices(z, y, hz, hy)
    Kl, Ll = HC.kernel_matrices(z, y, hz, hy, np.longdouble)
    perms = HC.numpy_permutations(n, P, seed)
    table = np.vstack([np.arange(n)[None], perms])  # slot 0: the observed pairing
    for estimator in HC.ESTIMATORS:
        res = hsic_permutation_test(z, y, estimator=estimator, permutations=perms)
        assert same_bits(res.hz, hz) and (res.hy is None if labels else same_bits(res.hy, hy))
        assert res.null_distribution.shape == (P,) and res.null_distribution.dtype == np.float64
        truth, tol, u, _ = HC.gate_of(K, L, Kl, Ll, table, estimator)
        got = np.concatenate([[res.statistic], res.null_distribution])
        err = report(f"{name} {estimator}", got, truth, tol, u)
        assert (err <= tol).all(), (int(np.argmax(err - tol)), float((err / u).max()))
        assert res.pvalue == (1 + int((res.null_distribution >= res.statistic).sum())) / (1 + P)


@needs_longdouble
@pytest.mark.parametrize("n,d,q,P", SIZES)
def test_statistic_and_every_null_value_within_the_gate(n, d, q, P):
    z, y = HC.rows(n, d, q, seed=n + d)
    check_case(z, y, P, seed=3, name=f"n={n} d={d} q={q} P={P}")


@needs_longdouble
@pytest.mark.parametrize("n,d,q,P", LABEL_SIZES)
def test_statistic_and_every_null_value_within_the_gate_for_labels(n, d, q, P):
    z, y = HC.rows(n, d, q, seed=n + d)
    check_case(z, HC.labels_of(y, 4), P, seed=4, name=f"n={n} d={d} labels P={P}")


@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("estimator", HC.ESTIMATORS)
def test_a_null_value_depends_on_its_permutation_row_alone(labels, estimator):
    from scrubvae_amd.eval import hsic_permutation_test
    from scrubvae_amd.eval import independence as IN
    n, launch = 131, IN._HSIC_LAUNCH
    z, y = HC.rows(n, 5, 3, seed=9)
    if labels:
        y = HC.labels_of(y, 4)
    row = HC.numpy_permutations(n, 1, 77)
    others = HC.numpy_permutations(n, launch + 40, 78)
    want = hsic_permutation_test(z, y, estimator=estimator, permutations=row).null_distribution[0]   # P = 1
    assert np.isfinite(want)
    # first, last, either side of a block's chunk boundary, either side of the launch boundary
    for P, at in [(2 * PC + 3, 0), (2 * PC + 3, 2 * PC + 2), (2 * PC + 3, PC - 1), (2 * PC + 3, PC), (launch + 40, launch - 1),
                  (launch + 40, launch), (launch + 40, launch + 39)]:
        table = others[:P].copy()
        table[at] = row[0]
        before = dict(IN._HSIC_CALLS)
        got = hsic_permutation_test(z, y, estimator=estimator, permutations=table).null_distribution
        assert IN._HSIC_CALLS["cross"] - before["cross"] == 1 + -(-P // launch)
        assert same_bits(got[at], want), (P, at)
        if at:
            assert not same_bits(got[0], want)


@pytest.mark.parametrize("estimator", HC.ESTIMATORS)
def test_bit_for_bit_promises(estimator):
    from scrubvae_amd.eval import hsic, hsic_permutation_test
    n = 301
    z, y = HC.rows(n, 3, 2, seed=5)
    c = HC.labels_of(y, 4)
    ident = np.arange(n)[None]
    perms = np.vstack([HC.numpy_permutations(n, 20, 1), ident, HC.numpy_permutations(n, 20, 2)])
    for v in (y, y[:, 0], c):
        a = hsic_permutation_test(z, v, estimator=estimator, permutations=perms)
        assert same_bits(a.statistic, hsic(z, v, estimator=estimator))
        assert same_bits(a.null_distribution[20], a.statistic)          # an identity row
        b = hsic_permutation_test(z, v, estimator=estimator, permutations=perms)
        assert same_array_bits(a.null_distribution, b.null_distribution)
        assert all(same_bits(getattr(a, k), getattr(b, k)) for k in ("statistic", "pvalue", "hz", "normalized"))
    # labels: renumbered, offset, another integer dtype, on the device
    a = hsic_permutation_test(z, c, estimator=estimator, permutations=perms)
    for other in (3 - c, np.array([7, -2, 100, 5])[c], c + 1000, c.astype(np.int32), torch.from_numpy(c).cuda()):
        b = hsic_permutation_test(z, other, estimator=estimator, permutations=perms)
        assert same_array_bits(a.null_distribution, b.null_distribution)
        assert same_bits(a.statistic, b.statistic) and same_bits(a.normalized, b.normalized) and same_bits(a.pvalue, b.pvalue)
    # input kinds: float32 on the device, torch permutations
    a = hsic_permutation_test(z, y, estimator=estimator, permutations=perms)
    b = hsic_permutation_test(torch.from_numpy(z.astype(np.float32)).cuda(), torch.from_numpy(y.astype(np.float32)).cuda(),
                              estimator=estimator, permutations=torch.from_numpy(perms).cuda())
    assert same_array_bits(a.null_distribution, b.null_distribution) and same_bits(a.statistic, b.statistic)
    assert isinstance(a.statistic, float) and isinstance(a.pvalue, float) and isinstance(a.normalized, float)
    # given bandwidths: the defaults passed back in change nothing
    b = hsic_permutation_test(z, y, hz=a.hz, hy=a.hy, estimator=estimator, permutations=perms)
    assert same_array_bits(a.null_distribution, b.null_distribution) and same_bits(a.statistic, b.statistic)


def test_seed_draws_the_documented_permutations():
    from scrubvae_amd.eval import hsic_permutation_test, mmd_permutations
    z, y = HC.rows(130, 4, 2, seed=6)
    perms = mmd_permutations(130, 40, 9, "cuda")
    a = hsic_permutation_test(z, y, n_permutations=40, seed=9)
    b = hsic_permutation_test(z, y, permutations=perms)
    assert same_array_bits(a.null_distribution, b.null_distribution) and same_bits(a.pvalue, b.pvalue)
    assert not same_array_bits(a.null_distribution, hsic_permutation_test(z, y, n_permutations=40, seed=10).null_distribution)
    bad = perms.clone()
    bad[3, 7] = bad[3, 8]
    with pytest.raises(ValueError, match=r"permutations\[3\]"):
        hsic_permutation_test(z, y, permutations=bad)


@pytest.mark.parametrize("n,q", [(301, 2), (130, 1), (4, 1), (40, 3), (131, 4)])
def test_bandwidth_is_the_exact_median(n, q):
    from scrubvae_amd.eval import hsic_bandwidth
    z, y = HC.rows(n, 5, q, seed=n)
    assert same_bits(hsic_bandwidth(z), HC.bandwidth(z))
    assert same_bits(hsic_bandwidth(y), HC.bandwidth(y))
    assert same_bits(hsic_bandwidth(torch.from_numpy(y[:, 0]).cuda()), HC.bandwidth(y[:, 0]))


@pytest.mark.parametrize("estimator", HC.ESTIMATORS)
def test_a_constant_y_gives_nan_throughout(estimator):
    from scrubvae_amd.eval import hsic, hsic_permutation_test
    z, y = HC.rows(40, 5, 2, seed=2)
    y[:] = y[0]
    res = hsic_permutation_test(z, y, estimator=estimator, n_permutations=20)
    assert res.hy == 0.0 and np.isnan(res.statistic) and np.isnan(res.pvalue) and np.isnan(res.normalized)
    assert res.null_distribution.shape == (20,) and np.isnan(res.null_distribution).all()
    assert np.isnan(hsic(z, y, estimator=estimator))
    z[:] = z[0]                               # a zero median on the z side
    res = hsic_permutation_test(z, HC.labels_of(HC.rows(40, 5, 2, seed=2)[1]), estimator=estimator, n_permutations=20)
    assert res.hz == 0.0 and np.isnan(res.statistic) and np.isnan(res.pvalue) and np.isnan(res.null_distribution).all()


@needs_longdouble
@pytest.mark.parametrize("labels,a", [(False, 0.0), (False, 0.15), (False, 0.5), (True, 0.0), (True, 0.25)])
def test_pvalue_is_exact(labels, a):
    from scrubvae_amd.eval import hsic, hsic_permutation_test
    count, pvalue = (HC.PVALUE_LABELS if labels else HC.PVALUE_REAL)[a]
    c = HC.pvalue_case(a, labels)
    z, y, perms, restated, t0 = c["z"], c["y"], c["perms"], c["restated"], c["t0"]
    K, L = HC.kernel_matrices(z, y, c["hz"], c["hy"])
    Kl, Ll = HC.kernel_matrices(z, y, c["hz"], c["hy"], np.longdouble)
    truth, tol, u, _ = HC.gate_of(K, L, Kl, Ll, perms, "biased", restated)
    truth0, tol0, u0, _ = HC.gate_of(K, L, Kl, Ll, np.arange(301), "biased", t0)
    nearest = np.abs(restated - t0) - 2 * (tol + tol0)
    assert (nearest > 0).all(), "a restated null value lies within twice the summed gates of the statistic: the count is not decided"
    assert int((restated >= t0).sum()) == count
    res = hsic_permutation_test(z, y, permutations=perms)
    err = report(f"p-value case labels={labels} a={a}", res.null_distribution, truth, tol, u)
    assert (err <= tol).all()
    assert same_bits(res.statistic, hsic(z, y)) and HC.err_of(res.statistic, truth0) <= tol0
    assert res.pvalue == (1 + count) / 1000 == pvalue, (res.pvalue, count)


@needs_longdouble
def test_normalized():
    from scrubvae_amd.eval import hsic_permutation_test
    from scrubvae_amd.eval import independence as IN
    c = HC.pvalue_case(0.5, False)
    z, y, hz, hy = c["z"], c["y"], c["hz"], c["hy"]
    ident = np.arange(301)
    K, L = HC.kernel_matrices(z, y, hz, hy)
    Kl, Ll = HC.kernel_matrices(z, y, hz, hy, np.longdouble)
    for estimator in HC.ESTIMATORS:  # always the biased form
        r = IN._hsic_run(IN._hsic_check(z, y, None, None, estimator), None, None, estimator, None, 0)
        parts = {}
        for name, (A, B, Al, Bl) in dict(num=(K, L, Kl, Ll), den_z=(K, K, Kl, Kl), den_y=(L, L, Ll, Ll)).items():
            truth, tol, u, _ = HC.gate_of(A, B, Al, Bl, ident, "biased")
            print(f"hsic normalized {estimator} {name}: device error {HC.err_of(r[name], truth) / u:.2f} u (gate {tol / u:.2f} u)")
            assert HC.err_of(r[name], truth) <= tol
            parts[name] = r[name]
        want = parts["num"] / np.sqrt(parts["den_z"] * parts["den_y"])
        assert same_bits(r["normalized"], want) and 0.0 < r["normalized"] < 1.0
        res = hsic_permutation_test(z, y, estimator=estimator, n_permutations=5)
        assert same_bits(res.normalized, r["normalized"])
    # z against itself (its first HSIC_MAX_Y columns: y is at most that wide): the alignment is 1; numerator and denominators are
    # the same sums within the gate
    z = z[:, :_lib.HSIC_MAX_Y]
    hz = HC.bandwidth(z)
    K, Kl = HC.gauss_matrix(z, hz), HC.gauss_matrix(z, hz, np.longdouble)
    r = IN._hsic_run(IN._hsic_check(z, z, None, None, "biased"), None, None, "biased", None, 0)
    truth, tol, u, _ = HC.gate_of(K, K, Kl, Kl, ident, "biased")
    for name in ("num", "den_z", "den_y"):
        assert HC.err_of(r[name], truth) <= tol
    # each of the three within tol of the truth t, relative error at most e = tol / t: the ratio is within (1 + e) / (1 - e) of 1
    e = float(tol / truth)
    res = hsic_permutation_test(z, z, n_permutations=5)
    print(f"hsic normalized (z, z): 1 + {res.normalized - 1.0:.3g} (bound {(1 + e) / (1 - e) - 1:.3g})")
    assert abs(res.normalized - 1.0) <= (1 + e) / (1 - e) - 1 + 2.0 ** -51
    assert res.pvalue == 1 / 6
