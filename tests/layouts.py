"""Member and output layouts for the any-strides contract (include/eks_hip.h:
obs[b*sb + t*st + e*se + j*sj], "strides in ELEMENTS, any layout").

``make`` carves a (B, T, E, n) member view out of one larger allocation that
is filled with a poison value wherever the view does not address it, with at
least one full step of poison before the view's first and after its last
element: a kernel that is one stride off reads poison, never memory outside
the allocation, and shows it in its result.  ``make_out`` does the same for
(B, T, n) float64 outputs with a canary that must survive the call.

Every layout names the run-time guard it aims at (``expected_paths``) and
claims, as plain arithmetic on (itemsize, B, T, E, n), the value of the three
fast-path predicates of the kernels; ``predicates`` evaluates the same three
from the strides and byte offset of a tensor the way the kernels do
(k_c0_shared in smooth_impl.hpp, eks_fit_pupil.hip).  test_layouts_host.py
holds the two against each other for every layout, dtype and B.
"""
from collections import namedtuple

import numpy as np

PUPIL_N = 8

Layout = namedtuple("Layout", "name storage expected_paths strides offset aligned16 claims "
                              "shared itemsizes")
Built = namedtuple("Built", "view base layout")


def _kvec(isz, E, n):
    """k_c0_shared's compile-time half of ``vec``: float32, E*n a multiple of 4."""
    return isz == 4 and (E * n) % 4 == 0


def _claims(vec, staged, packed):
    return dict(vec=vec, staged=staged, packed=packed)


def _never(isz, B, T, E, n):
    return _claims(False, False, False)


def _bm_strides(B, T, E, n, pad_t=0, pad_b=0):
    st = E * n + pad_t
    return (T * st + pad_b, st, n, 1)


_LAYOUTS = [
    Layout("tm", "(T,E,n,B) contiguous", "canonical, every other layout is compared with it",
           lambda B, T, E, n: (1, E * n * B, n * B, B), 0, True,
           lambda isz, B, T, E, n: _claims(B == 1 and _kvec(isz, E, n), B == 1 and _kvec(isz, E, n),
                                           B == 1 and n == PUPIL_N), False, (4, 8)),
    Layout("bm", "(B,T,E,n) contiguous, 16-byte aligned base", "vec, staged and packed true",
           lambda B, T, E, n: _bm_strides(B, T, E, n), 0, True,
           lambda isz, B, T, E, n: _claims(_kvec(isz, E, n), _kvec(isz, E, n), n == PUPIL_N),
           False, (4, 8)),
    Layout("bm_off1", "bm, base one element in", "base alignment false, strides perfect",
           lambda B, T, E, n: _bm_strides(B, T, E, n), 1, False, _never, False, (4, 8)),
    Layout("bm_off2_f32", "bm, base two float32 (8 bytes) in", "half-aligned base",
           lambda B, T, E, n: _bm_strides(B, T, E, n), 2, False, _never, False, (4,)),
    Layout("bm_padT1", "bm with st = E*n + 1",
           "row stride no 16-byte multiple, vec and packed false",
           lambda B, T, E, n: _bm_strides(B, T, E, n, pad_t=1), 0, True, _never, False, (4, 8)),
    Layout("bm_padT4", "bm with st = E*n + 4", "vec true, staged false; packed true",
           lambda B, T, E, n: _bm_strides(B, T, E, n, pad_t=4), 0, True,
           lambda isz, B, T, E, n: _claims(_kvec(isz, E, n), False, n == PUPIL_N), False, (4, 8)),
    Layout("bm_padB1", "bm with sb = T*E*n + 1",
           "packed's (sb*ts) % 16 false for B > 1",
           lambda B, T, E, n: _bm_strides(B, T, E, n, pad_b=1), 0, True,
           lambda isz, B, T, E, n: _claims(_kvec(isz, E, n), _kvec(isz, E, n),
                                           n == PUPIL_N and B == 1), False, (4, 8)),
    Layout("coord_major", "(B,T,n,E), se = 1, sj = E", "sj != 1, vec and packed false",
           lambda B, T, E, n: (T * n * E, n * E, 1, E), 0, True, _never, False, (4, 8)),
    Layout("member_outer", "(E,B,T,n), se the largest stride",
           "the reference's list of models, se != n",
           lambda B, T, E, n: (T * n, n, B * T * n, 1), 0, True, _never, False, (4, 8)),
    Layout("t_inner", "(B,E,n,T), st = 1", "unit step stride",
           lambda B, T, E, n: (E * n * T, 1, n * T, T), 0, True, _never, False, (4, 8)),
    Layout("tm_padB", "(T,E,n,B+3), base one element in",
           "ragged, offset trajectory axis",
           lambda B, T, E, n: (1, E * n * (B + 3), n * (B + 3), B + 3), 1, False, _never, False,
           (4, 8)),
    Layout("shared_bm", "sb = 0, one bm trajectory expanded",
           "k_c0_shared with vec and staged true",
           lambda B, T, E, n: (0,) + _bm_strides(B, T, E, n)[1:], 0, True,
           lambda isz, B, T, E, n: _claims(_kvec(isz, E, n), _kvec(isz, E, n), n == PUPIL_N),
           True, (4, 8)),
    Layout("shared_off1", "sb = 0, one bm_off1 trajectory expanded",
           "k_c0_shared, vec false by the base",
           lambda B, T, E, n: (0,) + _bm_strides(B, T, E, n)[1:], 1, False, _never, True, (4, 8)),
    Layout("shared_padT4", "sb = 0, one bm_padT4 trajectory expanded",
           "k_c0_shared, vec true, staged false",
           lambda B, T, E, n: (0,) + _bm_strides(B, T, E, n, pad_t=4)[1:], 0, True,
           lambda isz, B, T, E, n: _claims(_kvec(isz, E, n), False, n == PUPIL_N), True, (4, 8)),
    Layout("shared_padT1", "sb = 0, one bm_padT1 trajectory expanded",
           "k_c0_shared, vec false by st alone",
           lambda B, T, E, n: (0,) + _bm_strides(B, T, E, n, pad_t=1)[1:], 0, True, _never, True,
           (4, 8)),
    Layout("shared_coord", "sb = 0, one coord_major trajectory expanded",
           "k_c0_shared, sj != 1 and se != n",
           lambda B, T, E, n: (0, n * E, 1, E), 0, True, _never, True, (4, 8)),
]
LAYOUTS = {L.name: L for L in _LAYOUTS}
NAMES = tuple(LAYOUTS)
SHARED = tuple(L.name for L in _LAYOUTS if L.shared)
UNSHARED = tuple(L.name for L in _LAYOUTS if not L.shared)

EXPECTED_PATHS_TABLE = "\n".join(f"    {L.name:13s} {L.storage}: {L.expected_paths}"
                                 for L in _LAYOUTS)


def applies(name, dtype):
    """Whether layout ``name`` is defined for ``dtype`` (bm_off2_f32: float32 only)."""
    return np.dtype(dtype).itemsize in LAYOUTS[name].itemsizes


def guard_len(B, E, n):
    """Poison elements before the view's first and after its last element: one
    step of a trajectory-innermost layout (E*n*B), rounded up to 16 bytes in
    either type so that the guard does not move the view's alignment."""
    return -(-(E * n * max(B, 1)) // 4) * 4


def predicates(strides, byte_offset, itemsize, B, E, n):
    """The kernels' fast-path predicates from a tensor's element strides and
    the byte offset of its first element from a 16-byte aligned address."""
    sb, st, se, sj = strides
    vec = (_kvec(itemsize, E, n) and sj == 1 and se == n
           and ((byte_offset | (st * 4)) & 15) == 0)
    staged = vec and st == E * n
    packed = (n == PUPIL_N and sj == 1 and se == PUPIL_N and byte_offset % 16 == 0
              and (st * itemsize) % 16 == 0 and (B == 1 or (sb * itemsize) % 16 == 0))
    return dict(vec=vec, staged=staged, packed=packed)


def expected_values(values, name):
    """The (B, T, E, n) array the view of layout ``name`` must hold: ``values``
    (B, E, T, n) transposed; a shared layout repeats trajectory 0."""
    v = np.asarray(values).transpose(0, 2, 1, 3)
    if LAYOUTS[name].shared:
        v = np.broadcast_to(v[:1], v.shape)
    return v


def build(values, layout, dtype, poison, device="cpu"):
    """``make`` returning Built(view, base, layout): ``base`` is the 1-D
    allocation the view lives in."""
    import torch
    L = LAYOUTS[layout] if isinstance(layout, str) else layout
    tdt = {4: torch.float32, 8: torch.float64}[np.dtype(dtype).itemsize]
    if not applies(L.name, dtype):
        raise ValueError(f"layout {L.name} is not defined for {np.dtype(dtype)}")
    want = np.ascontiguousarray(expected_values(values, L.name))
    B, T, E, n = want.shape
    strides = tuple(int(s) for s in L.strides(B, T, E, n))
    G = guard_len(B, E, n)
    span = 1 + sum((d - 1) * s for d, s in zip((B, T, E, n), strides))
    base = torch.full((G + L.offset + span + G,), float(poison), dtype=tdt, device=device)
    view = base.as_strided((B, T, E, n), strides, G + L.offset)
    src = torch.from_numpy(want).to(device=device, dtype=tdt)
    if L.shared:  # one trajectory's storage, written once
        view[0].copy_(src[0])
    else:
        view.copy_(src)
    return Built(view, base, L)


def make(values, layout, dtype, poison, device="cpu"):
    """values (B, E, T, n) numpy -> tensor viewed as (B, T, E, n) holding
    exactly those values in layout ``layout`` (a name of LAYOUTS), every other
    element of its allocation equal to ``poison``."""
    return build(values, layout, dtype, poison, device).view


def addressed_mask(base, view):
    """bool (numel of base,): the elements of ``base`` that ``view`` addresses."""
    import torch
    mask = torch.zeros(base.numel(), dtype=torch.bool, device=base.device)
    off = view.storage_offset() - base.storage_offset()
    mask.as_strided(tuple(view.shape), tuple(view.stride()), off).fill_(True)
    return mask


def byte_offset16(t):
    """The tensor's first element's address modulo 16: from the pointer on a
    device, from the offset inside the (aligned) allocation as well."""
    return t.data_ptr() % 16


# ---------------------------------------------------------------------------
# output views
# ---------------------------------------------------------------------------
CANARY = 0x7FF8C0FFEE15BAD5  # a NaN with a payload: no kernel computes it

OutLayout = namedtuple("OutLayout", "name storage strides offset")
_OUT = [
    OutLayout("tm", "(T,B,n) contiguous: the default", lambda B, T, n: (n, B * n, 1), 0),
    OutLayout("bm", "(B,T,n) contiguous", lambda B, T, n: (T * n, n, 1), 0),
    OutLayout("padn", "(B,T,n+1): a padded column", lambda B, T, n: (T * (n + 1), n + 1, 1), 0),
    OutLayout("off1", "the default, one element into the buffer",
              lambda B, T, n: (n, B * n, 1), 1),
    OutLayout("nbt", "(n,B,T)", lambda B, T, n: (T, 1, B * T), 0),
]
OUT_LAYOUTS = {L.name: L for L in _OUT}
OUT_NAMES = tuple(OUT_LAYOUTS)


def make_out(B, T, n, layout, device="cpu"):
    """((B, T, n) float64 view inside a canary-filled buffer, check).
    ``check()`` raises AssertionError unless every float64 of the buffer that
    the view does not address still has the canary's bit pattern.  (A
    (B, S, T, n) output is ``make_out(B * S, T, n, ...)`` unflattened.)"""
    import torch
    L = OUT_LAYOUTS[layout]
    strides = tuple(int(s) for s in L.strides(B, T, n))
    G = B * n + 8
    span = 1 + sum((d - 1) * s for d, s in zip((B, T, n), strides))
    raw = torch.full((G + L.offset + span + G,), CANARY, dtype=torch.int64, device=device)
    base = raw.view(torch.float64)
    view = base.as_strided((B, T, n), strides, G + L.offset)
    mask = addressed_mask(base, view)

    def check():
        bad = int((raw[~mask] != CANARY).sum().item())
        assert bad == 0, f"{bad} float64 outside the {layout} view were overwritten"

    return view, check
