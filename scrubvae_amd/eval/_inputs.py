"""The argument checks that more than one eval feature uses: rows, labels, a variable that is either, and the two scalar
predicates.  Everything here runs where the argument lives, before any device work."""
import math

import numpy as np
import torch

from .. import _lib


def _is_int(v):
    """an int or a numpy integer, and not a bool"""
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _is_number(v):
    """an int, a float or a numpy scalar of either, not a bool, and finite"""
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)


def _finite_rows(A, name):
    """[n, d] -> fp64 rows where they are (torch tensor or numpy), checked finite"""
    if torch.is_tensor(A):
        t = A.detach()
        if t.dim() != 2:
            raise ValueError(f"{name}: expected a 2-D array of rows, got {t.dim()}-D")
        t = t.to(torch.float64)
        finite = bool(torch.isfinite(t).all()) if t.numel() else True
    else:
        t = np.asarray(A)
        if t.ndim != 2:
            raise ValueError(f"{name}: expected a 2-D array of rows, got {t.ndim}-D")
        t = np.ascontiguousarray(t, dtype=np.float64)
        finite = bool(np.isfinite(t).all())
    if not finite:
        raise ValueError(f"{name} holds non-finite values")
    return t


def _feature_rows(A, name):
    """_finite_rows with at least one feature"""
    t = _finite_rows(A, name)
    if t.shape[1] < 1:
        raise ValueError(f"{name} must have at least one feature")
    return t


def _int_labels(labels, n):
    """labels -> a 1-D integer numpy array of length n on the host"""
    if torch.is_tensor(labels):
        t = labels.detach()
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError(f"labels must hold integers, got {t.dtype}")
        lab = t.cpu().numpy()
    else:
        lab = np.asarray(labels)
        if lab.dtype.kind not in "iu":
            raise ValueError(f"labels must hold integers, got {lab.dtype}")
    if lab.ndim != 1 or lab.shape[0] != n:
        raise ValueError(f"labels must be [n = {n}], got shape {tuple(lab.shape)}")
    return lab


def _variable(y):
    """y -> ("real", fp64 rows [n, q] where they are) or ("labels", int32 numpy [n] in 0..K-1 on the host); a real y is at most
    HSIC_MAX_Y wide, the cap of the kernels that read one"""
    if torch.is_tensor(y):
        t = y.detach()
        integer = not (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool)
        floating = t.is_floating_point()
        ndim = t.dim()
    else:
        t = np.asarray(y)
        integer, floating, ndim = t.dtype.kind in "iu", t.dtype.kind == "f", t.ndim
    if integer:
        if ndim != 1:
            raise ValueError(f"integer y holds labels and must be 1-D, got {ndim}-D")
        lab = t.cpu().numpy() if torch.is_tensor(t) else t
        uniq, inv = np.unique(lab, return_inverse=True)
        if len(uniq) < 2:
            raise ValueError("labels y need at least two distinct values")
        return "labels", np.ascontiguousarray(inv.reshape(-1), dtype=np.int32)
    if not floating:
        raise ValueError(f"y must be of a floating or an integer dtype, got {t.dtype}")
    if ndim == 1:
        t = t.reshape(-1, 1)
    rows = _finite_rows(t, "y")
    if not 1 <= rows.shape[1] <= _lib.HSIC_MAX_Y:
        raise ValueError(f"real y must be [n] or [n, q] with 1 <= q <= {_lib.HSIC_MAX_Y}, got q = {rows.shape[1]}")
    return "real", rows
