"""tests/layouts.py on CPU tensors: every layout holds the values it was given,
has the strides and alignment it documents, is surrounded by poison with a
full step of guard on both sides, and sits on the side of the kernels'
fast-path guards (vec, staged of k_c0_shared; packed of eks_fit_pupil) that it
claims -- the predicates evaluated from the view's strides and its byte offset
inside the allocation against the layout's own closed-form claim.  The output
views and their canary check likewise, including that the check fails when a
single stray element is overwritten.  This is what shows that
test_gpu_layouts.py tests what it says.
"""
import numpy as np
import pytest

import layouts as LY

T = 13
SHAPES = [(4, 2), (5, 2), (5, 8), (4, 8), (5, 10)]  # (E, n)
POISONS = [float("nan"), 1e30]


def values(B, E, n):
    """(B, E, T, n) distinct float32-exact values."""
    return (np.arange(B * E * T * n, dtype=np.float64).reshape(B, E, T, n) + 1.0) / 8.0


def is_poison(t, poison):
    import torch
    return torch.isnan(t) if poison != poison else t == torch.tensor(poison, dtype=t.dtype)


@pytest.mark.parametrize("poison", POISONS, ids=["nan", "1e30"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", LY.NAMES)
def test_member_layout(name, dtype, B, poison):
    import torch
    if not LY.applies(name, dtype):
        with pytest.raises(ValueError):
            LY.make(values(B, 4, 2), name, dtype, poison, "cpu")
        return
    L = LY.LAYOUTS[name]
    isz = np.dtype(dtype).itemsize
    for E, n in SHAPES:
        v = values(B, E, n)
        view, base, _ = LY.build(v, name, dtype, poison, "cpu")
        assert LY.make(v, name, dtype, poison, "cpu").stride() == view.stride()
        # the view holds exactly the values
        assert view.shape == (B, T, E, n) and view.dtype == getattr(torch, np.dtype(dtype).name)
        assert np.array_equal(view.numpy(), LY.expected_values(v, name).astype(dtype))
        # strides and alignment as documented
        sb, st, se, sj = view.stride()
        assert (sb, st, se, sj) == tuple(L.strides(B, T, E, n))
        assert (sb == 0) == L.shared
        assert base.dim() == 1 and base.is_contiguous() and base.data_ptr() % 16 == 0
        off = view.storage_offset() - base.storage_offset()
        assert view.data_ptr() == base.data_ptr() + off * isz
        byte_off = off * isz % 16
        assert (byte_off == 0) == L.aligned16 == (view.data_ptr() % 16 == 0)
        if name == "bm_off2_f32":
            assert byte_off == 8
        if name in ("bm_off1", "shared_off1", "tm_padB"):
            assert byte_off == isz
        # everything the view does not address is poison, the rest is not
        mask = LY.addressed_mask(base, view)
        assert int(mask.sum()) == (1 if L.shared else B) * T * E * n
        assert bool(is_poison(base[~mask], poison).all())
        assert not bool(is_poison(base[mask], poison).any())
        # a full step of guard on both sides
        idx = torch.nonzero(mask).flatten()
        first, last = int(idx[0]), int(idx[-1])
        G = LY.guard_len(B, E, n)
        assert G >= E * n * B and G % 4 == 0
        assert first >= G and base.numel() - 1 - last >= G
        # the guards the layout aims at evaluate as claimed
        got = LY.predicates((sb, st, se, sj), byte_off, isz, B, E, n)
        assert got == L.claims(isz, B, T, E, n), (name, E, n, got)


def test_layout_table_covers_every_guard_term():
    """Per guard term one layout on which that term alone decides."""
    B, E, n = 3, 4, 8  # float32: vec compiled in (E*n % 4 == 0); the pupil's n
    P = {name: LY.LAYOUTS[name].claims(4, B, T, E, n) for name in LY.NAMES}
    assert P["bm"] == dict(vec=True, staged=True, packed=True)
    assert P["shared_bm"] == dict(vec=True, staged=True, packed=True)
    # base alignment alone
    assert P["bm_off1"] == P["bm_off2_f32"] == P["shared_off1"] == dict(
        vec=False, staged=False, packed=False)
    # the st term alone (base aligned, sj == 1, se == n)
    assert LY.LAYOUTS["bm_padT1"].aligned16 and not P["bm_padT1"]["vec"] \
        and not P["bm_padT1"]["packed"]
    # st == E*n alone
    assert P["bm_padT4"] == P["shared_padT4"] == dict(vec=True, staged=False, packed=True)
    # packed's sb term alone, and only for B > 1
    assert P["bm_padB1"] == dict(vec=True, staged=True, packed=False)
    assert LY.LAYOUTS["bm_padB1"].claims(4, 1, T, E, n)["packed"]
    # sj == 1 / se == n
    assert not any(P["coord_major"].values()) and not any(P["member_outer"].values())
    # vec is compiled out for float64 and for E*n % 4 != 0, packed is not
    assert LY.LAYOUTS["bm"].claims(8, B, T, E, n) == dict(vec=False, staged=False, packed=True)
    assert LY.LAYOUTS["bm"].claims(4, B, T, 5, 2) == dict(vec=False, staged=False, packed=False)
    # the predicates are the kernels': dropping the st term, or se >= 8 for
    # se == 8, would change the value on bm_padT1 / member_outer
    st1 = LY.LAYOUTS["bm_padT1"].strides(B, T, E, n)
    assert (st1[1] * 4) % 16 != 0 and st1[2] == n and st1[3] == 1
    mo = LY.LAYOUTS["member_outer"].strides(B, T, E, n)
    assert mo[2] > 8 and mo[3] == 1 and (mo[1] * 4) % 16 == 0 and (mo[0] * 4) % 16 == 0
    # k_c0_shared runs for sb == 0 only: its vec terms need shared layouts of their own
    assert LY.LAYOUTS["shared_padT1"].aligned16 and not P["shared_padT1"]["vec"]
    sp = LY.LAYOUTS["shared_padT1"].strides(B, T, E, n)
    assert sp[0] == 0 and (sp[1] * 4) % 16 != 0 and sp[2] == n and sp[3] == 1
    sc = LY.LAYOUTS["shared_coord"].strides(B, T, E, n)
    assert sc[0] == 0 and (sc[1] * 4) % 16 == 0 and sc[2] != n and sc[3] != 1
    assert LY.LAYOUTS["shared_coord"].aligned16 and not P["shared_coord"]["vec"]


def test_layout_table_is_in_the_gpu_module_docstring():
    import test_gpu_layouts
    assert len(LY.EXPECTED_PATHS_TABLE.splitlines()) == len(LY.NAMES)
    assert LY.EXPECTED_PATHS_TABLE in test_gpu_layouts.__doc__


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", LY.OUT_NAMES)
def test_out_layout(name, B):
    import torch
    n = 3
    view, check = LY.make_out(B, T, n, name, "cpu")
    assert view.shape == (B, T, n) and view.dtype == torch.float64
    assert view.stride() == tuple(LY.OUT_LAYOUTS[name].strides(B, T, n))
    base = view._base
    raw = base.view(torch.int64)
    assert bool((raw == LY.CANARY).all())
    check()  # untouched
    # writing every element of the view is what a kernel does: the check passes
    vals = torch.arange(B * T * n, dtype=torch.float64).reshape(B, T, n)
    view.copy_(vals)
    check()
    assert torch.equal(view, vals)
    mask = LY.addressed_mask(base, view)
    assert int(mask.sum()) == B * T * n
    idx = torch.nonzero(mask).flatten()
    assert int(idx[0]) >= B * n and base.numel() - 1 - int(idx[-1]) >= B * n
    # one stray element anywhere outside the view fails it: before, after, and
    # (where the layout has them) in a hole of the view
    stray = [int(idx[0]) - 1, int(idx[-1]) + 1, 0, base.numel() - 1]
    holes = torch.nonzero(~mask[int(idx[0]):int(idx[-1])]).flatten()
    if name == "padn":
        assert holes.numel() == B * T - 1
    if holes.numel():
        stray.append(int(idx[0]) + int(holes[0]))
    for i in stray:
        keep = raw[i].item()
        base[i] = 0.0
        with pytest.raises(AssertionError):
            check()
        raw[i] = keep
        check()
    # a value that equals the canary as a float (NaN) but not in its bits fails too
    base[0] = float("nan")
    with pytest.raises(AssertionError):
        check()
