"""The MMD permutation test without a GPU: the restatement of tests/mmd_null_checks.py pinned to the reference's recipe on relabelled
arrays, the label bit-packing, the permutation draw and checks on host tensors, argument errors and the C-ABI exports."""
import numpy as np
import pytest
import torch

from tests import mmd_checks as MC
from tests import mmd_null_checks as NC
from tests.mmd_checks import two_sets
from tests.test_mmd_cpu import reference_mmd


def draw(n, P, seed):
    g = np.random.default_rng(seed)
    return np.stack([g.permutation(n) for _ in range(P)])


@pytest.mark.parametrize("nx,ny,d", [(150, 151, 3), (90, 40, 37), (7, 64, 1)])
def test_restatement_is_the_reference_recipe_on_relabelled_rows(nx, ny, d):
    X, Y = two_sets(nx, ny, d, seed=d)
    Z = np.vstack([X, Y])
    perms = draw(nx + ny, 6, seed=nx)
    for h in (MC.bandwidth(X, Y), 3.7):
        got = NC.null_stats(X, Y, h, perms)
        for p, perm in enumerate(perms):
            Zp = Z[perm]
            assert got[p] == MC.mmd(Zp[:nx], Zp[nx:], h)       # the project's restatement, element for element
            assert got[p] == reference_mmd(Zp[:nx], Zp[nx:], h)  # scipy's pdist / cdist
        # the bandwidth belongs to the pooled rows: no relabelling changes it
        assert MC.bandwidth(Z[perms[0]][:nx], Z[perms[0]][nx:]) == MC.bandwidth(X, Y)


def test_identity_permutation_reproduces_the_statistic():
    X, Y = two_sets(150, 151, 3, seed=7, shift=0.0)
    h = MC.bandwidth(X, Y)
    ident = np.arange(301)[None]
    assert NC.null_stats(X, Y, h, ident)[0] == MC.mmd(X, Y, h)
    if np.finfo(np.longdouble).nmant >= 63:
        truth, tol, u, _ = NC.null_gate(X, Y, h, ident)
        t0, tol0, u0 = MC.mmd_gate(X, Y, h)
        assert truth[0] == t0 and tol[0] == tol0 and u[0] == u0


@pytest.mark.parametrize("P", [1, 63, 64, 65, 200])
def test_label_bits_match_the_membership_they_encode(P):
    from scrubvae_amd.eval import metrics as M
    n, nx = 77, 30
    perms = torch.from_numpy(draw(n, P, seed=P))
    bits = M._mmd_label_bits(perms, nx)
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (n, (P + 63) // 64) and bits.is_contiguous()
    want = np.zeros((P, n), dtype=np.int64)
    for p in range(P):
        want[p, perms[p, :nx].numpy()] = 1
    assert np.array_equal(NC.unpack_bits(bits.numpy(), P), want)
    padded = NC.unpack_bits(bits.numpy(), bits.shape[1] * 64)
    assert padded[P:].sum() == 0  # the bits past P are 0


def test_permutations_draw_on_the_host():
    from scrubvae_amd.eval import mmd_permutations
    a = mmd_permutations(301, 40, 7, "cpu")
    assert a.dtype == torch.int64 and tuple(a.shape) == (40, 301)
    assert np.array_equal(np.sort(a.numpy(), axis=1), np.tile(np.arange(301), (40, 1)))
    assert torch.equal(a, mmd_permutations(301, 40, 7, "cpu"))
    assert not torch.equal(a, mmd_permutations(301, 40, 8, "cpu"))
    assert len({tuple(r) for r in a.numpy()}) == 40
    for n, P in [(0, 3), (5, 0)]:
        with pytest.raises(ValueError):
            mmd_permutations(n, P, 0, "cpu")
    # the front end of the permutation tests: nothing given -> the count, then exactly this draw
    from scrubvae_amd.eval import _permutation as PM
    perms, P = PM._given_or_count(None, 3, 5)
    assert perms is None and P == 3
    assert torch.equal(PM._on_device_or_drawn(perms, 5, P, 7, torch.device("cpu")), mmd_permutations(5, 3, 7, "cpu"))


def test_permutation_rows_are_checked():
    from scrubvae_amd.eval import _permutation as M
    good = torch.from_numpy(draw(50, 9, seed=1))
    M._check_permutations(good)
    for bad_value in (int(good[5, 4]), 50, -1):  # a repeat, past the end, negative
        bad = good.clone()
        bad[5, 3] = bad_value
        with pytest.raises(ValueError, match=r"permutations\[5\]"):
            M._check_permutations(bad)
    # through the front end: a read-only int32 array comes back as the equal int64 tensor
    given = np.stack([np.random.default_rng(s).permutation(5) for s in range(3)]).astype(np.int32)
    given.setflags(write=False)
    perms, P = M._given_or_count(given, 1000, 5)
    assert P == 3 and perms.dtype == torch.int32
    out = M._on_device_or_drawn(perms, 5, P, 0, torch.device("cpu"))
    assert out.dtype == torch.int64 and np.array_equal(out.numpy(), given)
    # the rows are checked in chunks of 1024: row 1025 is the first row of the second chunk
    long = np.tile(np.arange(4), (1026, 1))
    long[1025, 2] = 0
    perms, P = M._given_or_count(long, 1000, 4)
    with pytest.raises(ValueError, match=r"permutations\[1025\]"):
        M._on_device_or_drawn(perms, 4, P, 0, torch.device("cpu"))


XS, YS = two_sets(4, 3, 2, seed=0)


@pytest.mark.parametrize("kwargs", [
    dict(n_permutations=0),
    dict(n_permutations=-5),
    dict(n_permutations=65537),
    dict(n_permutations=10.0),
    dict(n_permutations=True),
    dict(permutations=np.zeros((3, 6), dtype=np.int64)),          # n is 7
    dict(permutations=np.arange(7)),                               # 1-D
    dict(permutations=np.zeros((0, 7), dtype=np.int64)),
    dict(permutations=np.tile(np.arange(7.0), (2, 1))),            # not integers
    dict(h=0.0),
    dict(h=float("nan")),
])
def test_argument_errors_before_device_work(kwargs):
    """this machine has no device: a ValueError, not the "no device is available" RuntimeError, shows the order"""
    from scrubvae_amd.eval import mmd_permutation_test
    with pytest.raises(ValueError):
        mmd_permutation_test(XS, YS, **kwargs)


@pytest.mark.parametrize("X,Y", [(XS[:1], YS), (XS, YS[:, :1]), (XS, np.full((3, 2), np.inf)), (XS[0], YS)])
def test_row_errors_are_those_of_mmd_estimate(X, Y):
    from scrubvae_amd.eval import mmd_permutation_test
    with pytest.raises(ValueError):
        mmd_permutation_test(X, Y, n_permutations=10)


def test_new_exports_have_signatures():
    from scrubvae_amd import _lib
    from scrubvae_amd.eval import metrics as M
    lib = _lib.lib()
    assert lib.svae_mmd_null_blocks(1, 10) == 0 and lib.svae_mmd_null_blocks(0, 10) == 0
    assert lib.svae_mmd_null_blocks(10, 0) == 0 and lib.svae_mmd_null_blocks(10, _lib.MMD_NULL_MAX + 1) == 0
    # 3 sums x blocks x permutation columns padded to whole chunks of 256: one tile, then 2 x 2 tiles and two chunks
    assert lib.svae_mmd_null_blocks(2, 1) == 3 * 256 and lib.svae_mmd_null_blocks(64, 256) == 3 * 256
    assert lib.svae_mmd_null_blocks(65, 257) == 3 * 4 * 512
    assert lib.svae_mmd_null_blocks(4096, 1024) == 3 * 64 * 8 * 1024  # at most 8 column chunks per row tile
    import scrubvae_amd.eval as E
    assert callable(E.mmd_permutation_test) and callable(E.mmd_permutations)
    assert _lib.MMD_NULL_MAX == 65536
    assert M._MMD_CALLS.keys() >= {"select", "sums", "null"}
    r = M.MMDPermutationResult(1.0, 0.5, np.zeros(3), 2.0)
    assert (r.statistic, r.pvalue, r.h) == (1.0, 0.5, 2.0) and len(r.null_distribution) == 3
