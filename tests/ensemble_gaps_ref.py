"""The numpy reference of the ensemble over the valid members
(eks_ensemble_gaps; test_ensemble_gaps_host.py, test_gpu_ensemble_gaps.py)
and the masks its tests knock members out with.  Shared and read only.

Member e of a column is valid iff it is finite; with m valid members
    y  = np.nanmedian / np.nanmean over them
    ev = np.nanvar(ddof=0) / m
and both are NaN where m < min_members.
"""
import warnings

import numpy as np


def ensemble_valid(st, mode="median", min_members=1):
    """(y, ev, m) of members st (E, ...) reduced over axis 0."""
    fin = np.isfinite(st)
    x = np.where(fin, st, np.nan)
    m = fin.sum(0)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = np.nanmedian(x, axis=0) if mode == "median" else np.nanmean(x, axis=0)
        ev = np.nanvar(x, axis=0) / m
    gone = m < max(int(min_members), 1)
    y = np.where(gone, np.nan, y)
    ev = np.where(gone, np.nan, ev)
    return y, ev, m


def member_mask(seed, B, E, T, n, frac):
    """(B, E, T, n) bool: True where a member is knocked out."""
    return np.random.default_rng(seed).random((B, E, T, n)) < frac


def knock_members(st, mask, value=np.nan):
    """A copy of members (B, E, T, n) with the masked entries set to value."""
    out = st.copy()
    out[mask] = value
    return out


def planes(yev):
    """(y, ev) float64 (T, n, B) host copies of an EKS_YEV64 ``Yev``."""
    import torch
    from eks_amd import _lib
    assert yev.code == _lib.EKS_YEV64
    B, T, _, n = yev.shape
    sz = T * n * B * 8
    off = (sz + 255) // 256 * 256
    y = yev.buf[:sz].view(torch.float64).reshape(T, n, B).cpu().numpy()
    ev = yev.buf[off:off + sz].view(torch.float64).reshape(T, n, B).cpu().numpy()
    return y, ev
