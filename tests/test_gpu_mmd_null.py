"""mmd_permutation_test (csrc/mmd_null.hip) on the device against the numpy restatement of tests/mmd_null_checks.py.

Every T_p is held to the project's gate for this estimator, mmd_checks.mmd_gate's rule applied to the relabelled split:
|device - truth| <= 8 max(e_ref, u), truth in np.longdouble, e_ref the fp64 restatement's own error, u = 2^-53 (kxx + kyy + 2 kxy).
The kernel splits the permutation columns into chunks of 256 per block and 1024 per launch, and a row tile's column tiles into at
most 8 blocks."""
import functools

import numpy as np
import pytest
import torch

from tests import mmd_checks as MC
from tests import mmd_null_checks as NC
from tests.mmd_checks import two_sets
from tests.test_gpu_mmd import needs_longdouble, same_bits

pytestmark = pytest.mark.gpu

#        nx,  ny,   d,   P
SIZES = [(150, 151, 3, 999),    # many permutation chunks, partial row and column tiles
         (90, 40, 37, 257),     # partial feature chunk; P one past a 64- and a 256-boundary
         (70, 61, 128, 65),     # rows not resident in LDS
         (2, 2, 37, 1),         # the minimum
         (1030, 7, 1, 17)]      # more than 16 row tiles (3 column tiles per block), a tiny Y
OWN = (300, 290, 5, 300)        # 10 row tiles: 2 column tiles per block; 2 permutation chunks
OWN_TRUTH = [0, 1, 2, 127, 254, 255, 256, 257, 298, 299]  # first, last, both sides of the chunk boundary 255 | 256


def same_array_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def numpy_permutations(n, P, seed):
    g = np.random.default_rng(seed)
    return np.stack([g.permutation(n) for _ in range(P)])


@functools.lru_cache(maxsize=None)
def pvalue_case(shift):
    """the issue's p-value case: inputs, permutations and the restated null, computed once"""
    X, Y = two_sets(150, 151, 3, seed=7, shift=shift)
    perms = numpy_permutations(301, 999, 107)
    h = MC.bandwidth(X, Y)
    restated = NC.null_stats(X, Y, h, perms)
    for a in (X, Y, perms, restated):
        a.setflags(write=False)
    return X, Y, perms, h, restated


def report(name, got, truth, tol, u):
    err = np.abs((np.asarray(got).astype(np.longdouble) - truth).astype(np.float64))
    worst = int(np.argmax(err / u))
    print(f"mmd null {name}: {len(err)} permutations, worst device error {err[worst] / u[worst]:.2f} u (gate there "
          f"{tol[worst] / u[worst]:.2f} u), largest error / gate {np.max(err / tol):.3f}")
    return err


@needs_longdouble
@pytest.mark.parametrize("nx,ny,d,P", SIZES)
def test_every_null_value_within_eight_reference_errors(nx, ny, d, P):
    from scrubvae_amd.eval import mmd_permutation_test, mmd_permutations
    X, Y = two_sets(nx, ny, d, seed=nx + d)
    h = MC.bandwidth(X, Y)
    perms = mmd_permutations(nx + ny, P, 3, "cuda")
    res = mmd_permutation_test(X, Y, permutations=perms)
    assert same_bits(res.h, h) and res.null_distribution.shape == (P,) and res.null_distribution.dtype == np.float64
    truth, tol, u, _ = NC.null_gate(X, Y, h, perms.cpu().numpy())
    err = report(f"nx={nx} ny={ny} d={d} P={P}", res.null_distribution, truth, tol, u)
    assert (err <= tol).all(), (int(np.argmax(err - tol)), float((err / u).max()))


@needs_longdouble
def test_null_values_with_two_column_tiles_per_block_and_two_permutation_chunks():
    from scrubvae_amd.eval import mmd_permutation_test
    nx, ny, d, P = OWN
    X, Y = two_sets(nx, ny, d, seed=nx + d)
    h = 4.5
    perms = numpy_permutations(nx + ny, P, 11)
    got = mmd_permutation_test(X, Y, h, permutations=perms).null_distribution
    restated = NC.null_stats(X, Y, h, perms)
    sub = np.array(OWN_TRUTH)
    truth, tol, u, _ = NC.null_gate(X, Y, h, perms[sub], restated[sub])
    err = report(f"nx={nx} ny={ny} d={d} P={P} (truth on {len(sub)})", got[sub], truth, tol, u)
    assert (err <= tol).all(), float((err / u).max())
    # the rest against the fp64 restatement, within the sum of the two gates: each is within 8 max(e_ref, u) of the truth; e_ref
    # is not known without the truth, so take the largest seen on the subset, and u from the restated terms
    kxx, kyy, kxy = NC.null_terms(X, Y, h, perms)
    u_all = 2.0 ** -53 * (kxx + kyy + 2 * kxy)
    e_ref = np.abs((restated[sub].astype(np.longdouble) - truth).astype(np.float64))
    gate = 8 * np.maximum((e_ref / u).max() * u_all, u_all)
    diff = np.abs(got - restated)
    print(f"  all {P} against the fp64 restatement: worst {np.max(diff / u_all):.2f} u, gate {np.min(2 * gate / u_all):.2f} u")
    assert (diff <= 2 * gate).all()


@needs_longdouble
@pytest.mark.parametrize("shift,count,pvalue", [(0.0, 290, 0.291), (0.5, 0, 0.001)])
def test_pvalue_is_exact(shift, count, pvalue):
    from scrubvae_amd.eval import mmd_estimate, mmd_permutation_test
    X, Y, perms, h, restated = pvalue_case(shift)
    t0 = MC.mmd(X, Y, h)
    truth, tol, u, _ = NC.null_gate(X, Y, h, perms, restated)
    _, tol0, _ = MC.mmd_gate(X, Y, h)
    nearest = np.abs(restated - t0) - 2 * (tol + tol0)
    assert (nearest > 0).all(), "a restated T_p lies within twice the gate of T_0: the count is not decided by the restatement"
    assert int((restated >= t0).sum()) == count
    res = mmd_permutation_test(X, Y, seed=7, n_permutations=999, permutations=perms)
    err = report(f"p-value case shift={shift}", res.null_distribution, truth, tol, u)
    assert (err <= tol).all()
    assert same_bits(res.statistic, mmd_estimate(X, Y)) and abs(res.statistic - t0) <= tol0
    assert res.pvalue == (1 + count) / 1000 == pvalue, (res.pvalue, count)


@needs_longdouble
def test_identity_and_swap_reproduce_the_statistic():
    from scrubvae_amd.eval import mmd_permutation_test
    X, Y = two_sets(130, 130, 5, seed=21)
    h = MC.bandwidth(X, Y)
    n = 260
    perms = np.stack([np.arange(n), np.roll(np.arange(n), 130)])
    res = mmd_permutation_test(X, Y, permutations=perms)
    _, tol, u = MC.mmd_gate(X, Y, h)
    print(f"identity {abs(res.null_distribution[0] - res.statistic) / u:.2f} u, swap "
          f"{abs(res.null_distribution[1] - res.statistic) / u:.2f} u from the statistic (gate {tol / u:.2f} u)")
    assert abs(res.null_distribution[0] - res.statistic) <= tol
    assert abs(res.null_distribution[1] - res.statistic) <= tol
    X, Y = two_sets(150, 151, 3, seed=7)
    res = mmd_permutation_test(X, Y, permutations=np.arange(301)[None])
    _, tol, u = MC.mmd_gate(X, Y, MC.bandwidth(X, Y))
    assert abs(res.null_distribution[0] - res.statistic) <= tol
    assert res.pvalue == (1 + int(res.null_distribution[0] >= res.statistic)) / 2


def test_null_is_bit_reproducible_and_columns_are_independent():
    from scrubvae_amd.eval import mmd_permutation_test
    X, Y = two_sets(20, 21, 3, seed=1)
    perms = numpy_permutations(41, 1030, 5)   # two launches of up to 1024, five chunks of 256
    a = mmd_permutation_test(X, Y, 2.0, permutations=perms)
    b = mmd_permutation_test(X, Y, 2.0, permutations=perms)
    assert same_array_bits(a.null_distribution, b.null_distribution) and same_bits(a.pvalue, b.pvalue)
    for k in (0, 63, 64, 255, 256, 1023, 1024, 1029):
        one = mmd_permutation_test(X, Y, 2.0, permutations=perms[k: k + 1]).null_distribution
        assert same_bits(one[0], a.null_distribution[k]), k
    rev = mmd_permutation_test(X, Y, 2.0, permutations=perms[::-1].copy()).null_distribution
    assert same_array_bits(rev[::-1], a.null_distribution)
    # more than one block per column: the same at a size with partials to reduce
    X, Y = two_sets(150, 151, 3, seed=7)
    perms = numpy_permutations(301, 300, 6)
    a = mmd_permutation_test(X, Y, permutations=perms).null_distribution
    assert same_array_bits(a, mmd_permutation_test(X, Y, permutations=perms).null_distribution)
    for k in (255, 256):
        assert same_bits(mmd_permutation_test(X, Y, permutations=perms[k: k + 1]).null_distribution[0], a[k]), k


def test_seed_draws_the_documented_permutations():
    from scrubvae_amd.eval import mmd_permutation_test, mmd_permutations
    X, Y = two_sets(150, 151, 3, seed=7)
    perms = mmd_permutations(301, 300, 9, "cuda")
    assert perms.is_cuda and perms.dtype == torch.int64 and tuple(perms.shape) == (300, 301)
    assert torch.equal(perms.sort(dim=1).values, torch.arange(301, device="cuda").expand(300, 301))
    assert torch.equal(perms, mmd_permutations(301, 300, 9, torch.device("cuda", torch.cuda.current_device())))
    assert not torch.equal(perms, mmd_permutations(301, 300, 10, "cuda"))
    a = mmd_permutation_test(X, Y, n_permutations=300, seed=9)
    b = mmd_permutation_test(X, Y, permutations=perms)
    assert same_array_bits(a.null_distribution, b.null_distribution)
    assert same_bits(a.statistic, b.statistic) and same_bits(a.pvalue, b.pvalue) and same_bits(a.h, b.h)
    c = mmd_permutation_test(X, Y, n_permutations=300, seed=10)
    assert not same_array_bits(a.null_distribution, c.null_distribution)


def test_launch_counts_and_input_kinds():
    from scrubvae_amd.eval import metrics as M
    X, Y = two_sets(90, 40, 37, seed=3)   # float32-representable values
    perms = numpy_permutations(130, 1030, 2)
    before = dict(M._MMD_CALLS)
    a = M.mmd_permutation_test(X, Y, permutations=perms)
    assert M._MMD_CALLS == {"select": before["select"] + 1, "sums": before["sums"] + 1, "null": before["null"] + 2}
    assert same_bits(a.statistic, M.mmd_estimate(X, Y)) and same_bits(a.h, M.mmd_bandwidth(X, Y))
    before = dict(M._MMD_CALLS)
    b = M.mmd_permutation_test(X, Y, 30.0, permutations=perms[:1024])
    assert M._MMD_CALLS == {"select": before["select"], "sums": before["sums"] + 1, "null": before["null"] + 1}
    assert b.h == 30.0 and same_bits(b.statistic, M.mmd_estimate(X, Y, 30.0))
    assert isinstance(a.statistic, float) and isinstance(a.pvalue, float) and isinstance(a.h, float)
    assert a.pvalue == (1 + int((a.null_distribution >= a.statistic).sum())) / 1031
    xd, yd = torch.from_numpy(X.astype(np.float32)).cuda(), torch.from_numpy(Y.astype(np.float32)).cuda()
    c = M.mmd_permutation_test(xd, yd, permutations=torch.from_numpy(perms).cuda())
    assert same_array_bits(a.null_distribution, c.null_distribution)
    assert same_bits(a.statistic, c.statistic) and same_bits(a.pvalue, c.pvalue)
    e = M.mmd_permutation_test(X.astype(np.float32), torch.from_numpy(Y), permutations=perms.astype(np.int32))
    assert same_array_bits(a.null_distribution, e.null_distribution)


def test_bad_permutation_rows_are_refused_before_the_kernels():
    from scrubvae_amd.eval import metrics as M
    X, Y = two_sets(20, 21, 3, seed=1)
    perms = numpy_permutations(41, 5, 1)
    perms[3, 7] = perms[3, 8]
    before = dict(M._MMD_CALLS)
    with pytest.raises(ValueError, match=r"permutations\[3\]"):
        M.mmd_permutation_test(X, Y, permutations=perms)
    assert M._MMD_CALLS == before


def test_zero_median_gives_nan_everywhere():
    from scrubvae_amd.eval import mmd_permutation_test
    X, Y = two_sets(40, 13, 5, seed=2)
    X[:] = X[0]
    Y[:10] = X[0]                     # 50 of 53 rows coincide: the median distance is 0
    res = mmd_permutation_test(X, Y, n_permutations=70)
    assert res.h == 0.0 and np.isnan(res.statistic) and np.isnan(res.pvalue)
    assert res.null_distribution.shape == (70,) and np.isnan(res.null_distribution).all()
