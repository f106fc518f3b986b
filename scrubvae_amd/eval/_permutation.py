"""What the permutation tests of the eval modules share: the permutations they draw, the checks of given ones, and the p-value."""
import math

import numpy as np
import torch

from .. import _lib
from ._inputs import _is_int

MMD_MAX_PERMUTATIONS = _lib.MMD_NULL_MAX  # the cap on n_permutations: 65 536 (2.4e-5 resolves a p-value of 1.5e-5)
_CHECK_ROWS = 1024                        # rows per pass of _check_permutations: bounds the sorted copy


def mmd_permutations(n, n_permutations, seed, device):
    """[n_permutations, n] int64 on `device`, every row a uniformly drawn permutation of range(n): the argsort of uniform keys from
    a torch.Generator on that device seeded with `seed`.  Reproducible for a given seed, torch build and device type."""
    n, P = int(n), int(n_permutations)
    if n < 1 or P < 1:
        raise ValueError(f"mmd_permutations needs n >= 1 and n_permutations >= 1, got {n} and {P}")
    device = torch.device(device)
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return torch.rand(P, n, generator=g, device=device).argsort(dim=1)


def _count(n_permutations):
    if not _is_int(n_permutations):
        raise ValueError(f"n_permutations must be an integer, got {n_permutations!r}")
    if not 1 <= n_permutations <= MMD_MAX_PERMUTATIONS:
        raise ValueError(f"n_permutations must lie in [1, {MMD_MAX_PERMUTATIONS}], got {n_permutations}")
    return int(n_permutations)


def _permutation_array(permutations, n):
    """the shape and dtype errors of a given `permutations`, on the host -> an integer torch tensor [P, n] where it is"""
    if torch.is_tensor(permutations):
        t = permutations.detach()
    else:
        a = np.asarray(permutations)
        t = torch.as_tensor(a if a.flags.writeable else a.copy())  # torch refuses to share a read-only array
    if t.dim() != 2 or t.shape[1] != n or t.shape[0] < 1:
        raise ValueError(f"permutations must be [P, n = {n}] with P >= 1, got shape {tuple(t.shape)}")
    if t.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"permutations must hold integers, got {t.dtype}")
    _count(t.shape[0])
    return t


def _check_permutations(perms):
    """ValueError unless every row of perms [P, n] (a torch tensor, checked where it lives) is a permutation of range(n)"""
    n = perms.shape[1]
    want = torch.arange(n, device=perms.device, dtype=perms.dtype)
    for p0 in range(0, perms.shape[0], _CHECK_ROWS):
        ok = (perms[p0: p0 + _CHECK_ROWS].sort(dim=1).values == want).all(dim=1)
        if not bool(ok.all()):
            raise ValueError(f"permutations[{p0 + int((~ok).nonzero()[0])}] is not a permutation of range({n})")


def _given_or_count(permutations, n_permutations, n):
    """the host half of a permutation test's front end -> (the given `permutations` as _permutation_array checks them, or None;
    P, their number or the checked n_permutations)"""
    if permutations is None:
        return None, _count(n_permutations)
    perms = _permutation_array(permutations, n)
    return perms, perms.shape[0]


def _on_device_or_drawn(perms, n, P, seed, dev):
    """the device half -> int64 [P, n] on dev: the given rows (from _given_or_count) moved and checked to be permutations, or P
    rows drawn by mmd_permutations"""
    if perms is None:
        return mmd_permutations(n, P, seed, dev)
    perms = perms.to(device=dev, dtype=torch.int64)
    _check_permutations(perms)
    return perms


def _pvalue(statistic, null):
    """(1 + #{p: null[p] >= statistic}) / (1 + P) for the null [P] numpy, compared in fp64; nan for a nan statistic"""
    if math.isnan(statistic):
        return float("nan")
    return (1 + int((null >= statistic).sum())) / (1 + len(null))
