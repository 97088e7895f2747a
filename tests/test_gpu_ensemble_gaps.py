"""The ensemble over the valid members on the device (eks_ensemble_gaps,
batch.ensemble_gaps, torch.ops.eks.ensemble_gaps), the fit from planes
(batch.fit_gaps on a Yev) and the wrappers' ``min_members`` against the numpy
reference of tests/ensemble_gaps_ref.py: np.nanmedian / np.nanmean and
np.nanvar / m over the finite members, NaN where m < min_members.

Bounds of the parity test (from a float64 numpy emulation of the device
arithmetic against that reference, E in {3, 4, 5, 8, 9, 17}, 35 % NaN, 23 779
columns: median bit-identical, mean within 2.1e-16 of max|x|, variance within
6.2e-16 relative; the bounds are about 50 x those): median y bit-equal, mean
|dy| <= 1e-14 max|x|, ev rtol 3e-14, the NaN pattern and the counts equal.

Downstream bounds are tests/test_gpu_gaps.py's (out 1e-8 px, var rtol 1e-8,
NLL rtol 1e-9), the fit's are tests/test_gpu_fit_gaps.py's.
"""
import functools
import warnings

import numpy as np
import pandas as pd
import pytest

import ensemble_gaps_ref as R
import gaps_ref as G

pytestmark = pytest.mark.gpu

OUT_TOL, RTOL, NLL_RTOL = 1e-8, 1e-8, 1e-9
MEAN_TOL, EV_RTOL = 1e-14, 3e-14
S = 0.01


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def members(n, B, T, E, seed):
    if n == 2:
        return G.members("sv", B, T, E=E, seed=seed)
    return G.members("mc", B, T, V=n // 2, E=E, seed=seed)


def layouts(st, dtype):
    """The two member layouts of the parity tests as (B, T, E, n) views:
    make_time_major's (T, E, n, B) buffer, and the (E, T, n) blocks of
    core.ensemble_handoff (one per trajectory)."""
    import torch
    from eks_amd import batch
    yield "time-major", batch.make_time_major(st, dtype=dtype)
    d = torch.from_numpy(np.ascontiguousarray(st.astype(dtype))).to("cuda")  # (B, E, T, n)
    yield "(E, T, n)", d.permute(0, 2, 1, 3)


# -- 1: parity -------------------------------------------------------------------------
def special_columns(E, mm):
    """The valid-member counts built explicitly, one column each: min_members
    - 1 and min_members, then every count 0..E."""
    return [mm - 1, mm] + list(range(E + 1))


def knocked_out(st, E, mm, seed):
    """Members (B, E, T, n) with 30 % of the members NaN, and -- each on
    columns of its own, as far as the shape has columns -- the first and the
    last frame hit, the counts of special_columns(), +inf and -inf members and
    one frame with every member NaN.  Returns (members, built): built is False
    for a shape too small to hold every special column."""
    B, _, T, n = st.shape
    rng = np.random.default_rng(seed)
    g = R.knock_members(st, R.member_mask(seed, B, E, T, n, 0.30))
    hits = [(0, 0, 0), (B - 1, T - 1, n - 1)]  # the first and the last frame
    g[0, 0, 0, 0] = np.nan
    g[B - 1, E - 1, T - 1, n - 1] = np.nan
    cols = [(b, t, j) for b in range(B) for t in range(T) for j in range(n)]
    dead = (B // 2, T // 2) if B * T >= 3 else None  # the frame with nothing valid
    free = [c for c in cols if c not in hits and (dead is None or (c[0], c[1]) != dead)]
    order = rng.permutation(len(free))
    want = special_columns(E, mm)
    for k, ci in zip(want, order):
        b, t, j = free[ci]
        valid = rng.permutation(E)[:k]
        g[b, :, t, j] = np.nan
        g[b, valid, t, j] = st[b, valid, t, j]
    for i, ci in enumerate(order[len(want):len(want) + 6]):  # a few +-inf members
        b, t, j = free[ci]
        g[b, i % E, t, j] = np.inf if i % 2 == 0 else -np.inf
        if i >= 4:  # both signs in one column
            g[b, (i + 1) % E, t, j] = -np.inf if i % 2 == 0 else np.inf
    if dead is not None:
        g[dead[0], :, dead[1], :] = np.nan
    return g, len(free) >= len(want) + 6 and dead is not None


PARITY_E = [(3, 2), (4, 2), (5, 3), (5, 5), (8, 3), (9, 1), (17, 9)]


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("E,mm", PARITY_E)
def test_parity(torch, E, mm, B):
    """Compiled (3, 4, 5, 8) and runtime (9, 17) member counts, the 8-way
    summation from E = 8 in both forms, one lane, a few, and more than a wave of trajectories; T off the
    ring's block and off the chunk grid; both member types, both modes, both
    layouts.  Every shape that has the columns for them holds every special
    column of knocked_out(); T = 300 always does."""
    from eks_amd import batch
    worst = dict(mean=0.0, ev=0.0)
    full = 0
    for T in (1, 17, 300):
        for n in (2, 8, 12):
            g, built = knocked_out(members(n, B, T, E, 1000 * E + 10 * T + n), E, mm,
                                   seed=7919 * E + 31 * T + n + B)
            xmax = float(np.abs(g[np.isfinite(g)]).max())
            ge = g.transpose(1, 0, 2, 3)  # (E, B, T, n)
            for mode in ("median", "mean"):
                y, ev, m = R.ensemble_valid(ge, mode, mm)
                if built:
                    full += 1
                    assert set(range(E + 1)) <= set(np.unique(m).tolist()), (T, n, np.unique(m))
                    assert (m == mm - 1).any() and (m == mm).any()
                    assert (m[:, 0] < E).any() and (m[:, -1] < E).any()
                    assert (m.reshape(B * T, n) == 0).all(axis=1).any()
                    assert np.isposinf(g).any() and np.isneginf(g).any()
                for dtype in (np.float32, np.float64):
                    for name, d in layouts(g, dtype):
                        what = (E, mm, B, T, n, mode, dtype.__name__, name)
                        res = batch.ensemble_gaps(d, n=n, mode=mode, min_members=mm,
                                                  want_nvalid=True)
                        assert res["yev"].shape == (B, T, E, n) and res["yev"].mode == mode
                        yd, ed = (a.transpose(2, 0, 1) for a in R.planes(res["yev"]))
                        nv = res["nvalid"].cpu().numpy().transpose(2, 0, 1)
                        np.testing.assert_array_equal(nv, m, err_msg=str(what))
                        np.testing.assert_array_equal(np.isnan(yd), np.isnan(y), err_msg=str(what))
                        np.testing.assert_array_equal(np.isnan(ed), np.isnan(ev), err_msg=str(what))
                        assert (np.isnan(y) == (m < mm)).all()
                        ok = ~np.isnan(y)
                        if mode == "median":
                            np.testing.assert_array_equal(yd, y, err_msg=str(what))
                        else:
                            dy = float(np.abs(yd[ok] - y[ok]).max()) if ok.any() else 0.0
                            worst["mean"] = max(worst["mean"], dy / xmax)
                            assert dy <= MEAN_TOL * xmax, (what, dy)
                        if ok.any():
                            pos = ok & (ev > 0)
                            np.testing.assert_array_equal(ed[ok & ~pos], ev[ok & ~pos])
                            rel = float((np.abs(ed[pos] - ev[pos]) / ev[pos]).max()) \
                                if pos.any() else 0.0
                            worst["ev"] = max(worst["ev"], rel)
                            assert rel <= EV_RTOL, (what, rel)
    print(f"[ensemble gaps] E={E} min_members={mm} B={B}: mean {worst['mean']:.2e} of max|x|, "
          f"ev rel {worst['ev']:.2e}; {full} shapes with every special column")
    assert full >= 6  # T = 300 at every n and mode


def test_nvalid_is_optional_and_the_buffer_is_reused(torch):
    from eks_amd import batch
    g = R.knock_members(members(2, 3, 40, 5, 3), R.member_mask(3, 3, 5, 40, 2, 0.3))
    d = batch.make_time_major(g, dtype=np.float32)
    a = batch.ensemble_gaps(d, n=2, min_members=3, want_nvalid=True)
    b = batch.ensemble_gaps(d, n=2, min_members=3, keep_yev=a["yev"])
    assert b["nvalid"] is None and b["yev"].buf.data_ptr() == a["yev"].buf.data_ptr()
    c = batch.ensemble_gaps(d, n=2, min_members=3)
    for p, q in zip(R.planes(a["yev"]), R.planes(c["yev"])):
        np.testing.assert_array_equal(p, q)
    # the operator returns the same planes and counts
    import eks_amd.ops  # noqa: F401
    yev, nvalid = torch.ops.eks.ensemble_gaps(d, "median", 3)
    assert yev.dtype == torch.uint8 and yev.numel() == a["yev"].buf.numel()
    op = batch.Yev(yev, 3, 40, 5, 2, a["yev"].code, "median")
    for p, q in zip(R.planes(op), R.planes(a["yev"])):
        np.testing.assert_array_equal(p, q)
    np.testing.assert_array_equal(nvalid.cpu().numpy(), a["nvalid"].cpu().numpy())
    for bad in (0, 6):
        with pytest.raises(ValueError, match="min_members"):
            batch.ensemble_gaps(d, n=2, min_members=bad)


# -- 2: bit-identity on complete data -----------------------------------------------------
@pytest.mark.parametrize("mode", ["median", "mean"])
@pytest.mark.parametrize("E", [3, 4, 5, 8])
def test_complete_columns_have_eks_ensembles_bits(torch, E, mode):
    """Gap-free members: the planes are eks_ensemble's output bit for bit.
    With gaps and min_members = E: NaN exactly where a member is not finite,
    eks_ensemble's bits elsewhere (waves that mix complete and incomplete
    columns take the general path)."""
    import eks_amd.ops  # noqa: F401
    from eks_amd import batch
    for B, T, n in ((3, 300, 2), (70, 33, 8)):
        st = members(n, B, T, E, seed=E + T)
        g = R.knock_members(st, R.member_mask(E + n, B, E, T, n, 0.05))
        g[0, 0, 3, 0] = np.inf
        g[B - 1, E - 1, T - 1, n - 1] = -np.inf
        for dtype in (np.float32, np.float64):
            for name, d in layouts(st, dtype):
                p0, v0 = (a.cpu().numpy() for a in torch.ops.eks.ensemble(d, mode))
                res = batch.ensemble_gaps(d, n=n, mode=mode, min_members=2, want_nvalid=True)
                y, ev = (a.transpose(2, 0, 1) for a in R.planes(res["yev"]))
                np.testing.assert_array_equal(y, p0, err_msg=f"{name} {dtype.__name__}")
                np.testing.assert_array_equal(ev, v0, err_msg=f"{name} {dtype.__name__}")
                assert bool((res["nvalid"] == E).all())
            for name, d in layouts(g, dtype):
                p0, v0 = (a.cpu().numpy() for a in torch.ops.eks.ensemble(d, mode))
                res = batch.ensemble_gaps(d, n=n, mode=mode, min_members=E)
                y, ev = (a.transpose(2, 0, 1) for a in R.planes(res["yev"]))
                whole = np.isfinite(g).all(axis=1)  # (B, T, n)
                assert not whole.all() and whole.any()
                np.testing.assert_array_equal(np.isnan(y), ~whole)
                np.testing.assert_array_equal(np.isnan(ev), ~whole)
                np.testing.assert_array_equal(y[whole], p0[whole])
                np.testing.assert_array_equal(ev[whole], v0[whole])


# -- 3: downstream ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def downstream_case(n):
    """B = 3, T = 131, E = 5: 30 % of the members NaN and a 40-frame run with
    nothing valid; the models of the complete members."""
    kind = "sv" if n == 2 else "mc"
    st = members(n, 3, 131, 5, seed=131 + n)
    models = [G.model_of(kind, st[b]) for b in range(3)]
    mask = R.member_mask(131 * n, 3, 5, 131, n, 0.30)
    mask[0, :, 45:85, :] = True
    mask[1, :, 3:43, :] = True
    g = R.knock_members(st, mask)
    g.setflags(write=False)
    return g, models


@pytest.mark.parametrize("n,r", [(2, 2), (8, 3)])
def test_downstream_smooth_and_sweep(torch, n, r):
    from eks_amd import batch
    g, models = downstream_case(n)
    B, E, T, _ = g.shape
    refs = []
    new_ground = 0
    for b in range(B):
        y, ev, m = R.ensemble_valid(g[b], "median", 3)
        seen = G.observed(y, ev)
        assert (ev[seen] > 0).all()  # no exact observation
        new_ground += int((seen & (m < E)).sum())
        refs.append((y, ev))
    assert new_ground > 0  # columns the all-members rule calls missing
    d = batch.make_time_major(g, dtype=np.float32)
    yev = batch.ensemble_gaps(d, n=n, min_members=3)["yev"]
    stk = lambda k, s=1.0: np.stack([mo[k] * (s if k == "Q" else 1.0) for mo in models])  # noqa: E731
    pack = lambda s=1.0: batch.pack_params(stk("m0"), stk("S0"), stk("A"), stk("Q", s), stk("C"),  # noqa: E731
                                           stk("means"))
    sm = batch.smooth_gaps(yev, pack(), n=n, r=r, want_var=True, want_nll=True, check=True)
    out, var, nll = (sm[k].cpu().numpy() for k in ("out", "var", "nll"))
    scales = (0.1, 1.0, 10.0)
    rows = torch.cat([pack(s) for s in scales]).contiguous()
    sw = batch.nll_sweep_gaps(yev, rows, K=3, n=n, r=r)
    sw_nll = sw["nll"].cpu().numpy()
    worst = dict(out=0.0, var=0.0, nll=0.0, sweep=0.0)
    for b in range(B):
        y, ev = refs[b]
        ref = G.dense(y, ev, models[b])
        assert np.isfinite(ref["out"]).all() and np.isfinite(out[b]).all()
        assert int(sm["nobs"][b]) == ref["nobs"] == int(sw["nobs"][b])
        worst["out"] = max(worst["out"], float(np.abs(out[b] - ref["out"]).max()))
        worst["var"] = max(worst["var"], float((np.abs(var[b] - ref["var"]) / ref["var"]).max()))
        worst["nll"] = max(worst["nll"], abs(nll[b] - ref["nll"]) / abs(ref["nll"]))
        for k, s in enumerate(scales):
            rk = G.dense(y, ev, dict(models[b], Q=models[b]["Q"] * s))["nll"]
            worst["sweep"] = max(worst["sweep"], abs(sw_nll[k, b] - rk) / abs(rk))
    print(f"[ensemble gaps] downstream n={n}: out {worst['out']:.3e} px, var rel "
          f"{worst['var']:.3e}, nll rel {worst['nll']:.3e}, sweep rel {worst['sweep']:.3e}; "
          f"{new_ground} columns observed with a member missing")
    assert worst["out"] <= OUT_TOL and worst["var"] <= RTOL, worst
    assert worst["nll"] <= NLL_RTOL and worst["sweep"] <= NLL_RTOL, worst
    assert int(sm["status"].abs().sum()) == 0 and int(sw["status"].abs().sum()) == 0


# -- 4: the fit from planes -------------------------------------------------------------------
FIT_SHAPES = [("singleview", 2), ("multicam", 4), ("multicam", 8), ("multicam", 12)]


def fit_members(kind, n, frac=0.03):
    """B = 4, T = 700, E = 5 members with whole columns knocked out (the
    all-members rule of eks_fit_gaps on members)."""
    st = members(n, 4, 700, 5, seed=700 + n)
    mask = np.random.default_rng(700 + n).random((4, 700, n)) < frac
    mask[0, 0] = True   # frame 0 missing: the shift comes from a later frame
    mask[0, -1] = True
    mask[1, 40:90, 0:2] = True
    mask[3] = False
    return st, G.knock_out(st, mask)


@pytest.mark.parametrize("mode,dtype,code", [("median", np.float32, "EKS_YEV32"),
                                             ("mean", np.float64, "EKS_YEV64")])
@pytest.mark.parametrize("kind,n", FIT_SHAPES)
def test_fit_from_its_own_planes_is_bit_identical(torch, kind, n, mode, dtype, code):
    from eks_amd import _lib, batch
    r = 2 if kind == "singleview" else 3
    _, g = fit_members(kind, n)
    d = batch.make_time_major(g, dtype=dtype)
    kw = dict(kind=kind, n=n, r=r, smooth_param=S, quantile_keep=25.0)
    a = batch.fit_gaps(d, mode=mode, **kw)
    assert a["yev"].code == getattr(_lib, code)
    before = a["yev"].buf.clone()
    b = batch.fit_gaps(a["yev"], **kw)
    assert b["yev"] is a["yev"]
    assert torch.equal(a["yev"].buf, before)  # nothing is written to the planes
    for k in ("params", "status", "ncomplete", "nkept"):
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert np.array_equal(x, y, equal_nan=True), (k, x, y)
    assert 0 < int(a["ncomplete"][0]) < 700 and int(a["ncomplete"][3]) == 700
    assert int(a["status"].abs().sum()) == 0
    with pytest.raises(ValueError, match="keep_yev"):
        batch.fit_gaps(a["yev"], keep_yev=a["yev"], **kw)


def host_fit(preds, ev, kind, q):
    """(model or None, ok): the wrappers' host fit on the complete frames."""
    from eks_amd import fit
    from eks_amd.smoothers import _complete_frames
    ok = _complete_frames(preds, ev)
    if not ok.any():
        return None, ok
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = fit.singleview_model if kind == "singleview" else fit.multicam_model
        return f(preds[ok], ev[ok], S, q), ok


@pytest.mark.parametrize("kind,n", FIT_SHAPES)
def test_fit_from_ensemble_gaps_planes_against_the_host_fit(torch, kind, n):
    """ensemble_gaps(min_members = 3) -> fit_gaps on its planes against the
    host fit on the frames complete in the numpy reference (the comparison and
    tolerances of tests/test_gpu_fit_gaps.py, exact counts); trajectory 1 has
    a column with two valid members in every frame: nothing complete."""
    import test_gpu_fit_gaps as FG
    from eks_amd import _lib, batch
    r, q = 2 if kind == "singleview" else 3, 25.0
    B, E, T = 4, 5, 700
    st = members(n, B, T, E, seed=900 + n)
    mask = R.member_mask(900 + n, B, E, T, n, 0.20)
    mask[1, :3, :, n - 1] = True
    mask[3] = False
    g = R.knock_members(st, mask)
    d = batch.make_time_major(g, dtype=np.float32)
    yev = batch.ensemble_gaps(d, n=n, min_members=3)["yev"]
    res = batch.fit_gaps(yev, kind=kind, n=n, r=r, smooth_param=S, quantile_keep=q, check=False)
    assert res["yev"] is yev
    params = res["params"].cpu().numpy()
    status, nc, nk = (res[k].cpu().numpy() for k in ("status", "ncomplete", "nkept"))
    counts = []
    for b in range(B):
        y, ev, _ = R.ensemble_valid(g[b], "median", 3)
        ref, ok = host_fit(y, ev, kind, q)
        assert int(nc[b]) == int(ok.sum()), (b, int(nc[b]), int(ok.sum()))
        if ref is None:
            assert b == 1 and status[b] == _lib.EKS_STATUS_SINGULAR and nk[b] == 0
            counts.append((0, 0))
            continue
        counts.append((int(ok.sum()), len(ref["keep"])))
        assert int(nk[b]) == len(ref["keep"]) and status[b] == 0, (b, int(nk[b]))
        got = FG._unpack(params[b], n, r)
        if kind == "singleview":
            for k in ("m0", "S0", "A", "Q", "C", "offset"):
                FG._close(got[k], ref[k], 1e-9)
        else:
            FG._close(got["offset"], ref["offset"], 1e-9)
            FG._close(got["A"], ref["A"], 1e-9)
            np.testing.assert_array_equal(got["m0"], ref["m0"])
            sgn = np.sign(np.sum(got["C"] * ref["C"], axis=0))
            FG._close(got["C"] * sgn, ref["C"], 1e-7)
            FG._close(got["S0"], ref["S0"], 1e-8)
            FG._close(got["Q"] * np.outer(sgn, sgn), ref["Q"], 1e-7)
    print(f"[ensemble gaps] fit from planes {kind} n={n}: (complete, kept) {counts}")
    assert counts[1] == (0, 0) and counts[3][0] == T
    assert all(c[1] >= 24 for i, c in enumerate(counts) if i != 1), counts
    with pytest.raises(ValueError, match="1 of 4 trajectories"):
        batch.fit_gaps(yev, kind=kind, n=n, r=r, smooth_param=S, quantile_keep=q)


@pytest.mark.parametrize("kind,n", [("singleview", 2), ("multicam", 8), ("multicam", 12)])
def test_full_device_chain(torch, kind, n):
    """ensemble_gaps -> fit_gaps -> select_smooth_param -> smooth_gaps without
    a host step: every output finite, every status zero."""
    from eks_amd import batch
    r = 2 if kind == "singleview" else 3
    B, E, T = 4, 5, 700
    g = R.knock_members(members(n, B, T, E, seed=300 + n),
                        R.member_mask(300 + n, B, E, T, n, 0.20))
    g[2, :, 100:140] = np.nan  # nothing valid over 40 frames
    d = batch.make_time_major(g, dtype=np.float32)
    ens = batch.ensemble_gaps(d, n=n, min_members=3, want_nvalid=True)
    fitted = batch.fit_gaps(ens["yev"], kind=kind, n=n, r=r, smooth_param=1.0, quantile_keep=25.0)
    sel = batch.select_smooth_param(ens["yev"], fitted["params"], n=n, r=r, allow_missing=True)
    sm = batch.smooth_gaps(ens["yev"], sel["params"], n=n, r=r, want_var=True, want_nll=True,
                           check=True)
    for k in ("out", "var", "nll"):
        assert bool(torch.isfinite(sm[k]).all()), k
    assert bool(torch.isfinite(fitted["params"]).all()) and bool(torch.isfinite(sel["nll"]).all())
    assert bool((sel["smooth_param"] > 0).all())
    assert int(fitted["status"].abs().sum()) == 0 and int(sm["status"].abs().sum()) == 0
    seen = int((ens["nvalid"] >= 3).sum())
    assert int(sm["nobs"].sum()) == seen == int(sel["nobs"].sum())
    assert bool((fitted["ncomplete"] > 0).all()) and bool((fitted["nkept"] > 0).all())


# -- 5: the wrappers --------------------------------------------------------------------------
def _oracle_model(kind, preds, ev, s, q):
    from oracle import eks_oracle as O
    ok = np.isfinite(preds).all(axis=1) & np.isfinite(ev).all(axis=1)
    p = (O.singleview_params if kind == "sv" else O.multicam_params)(preds[ok], ev[ok], s, q)
    return {k: p[k] for k in ("m0", "S0", "A", "Q", "C", "means")}


def test_wrapper_single_view(torch):
    from eks_amd.singleview_smoother import ensemble_kalman_smoother_single_view as sv
    T = 131
    st = members(2, 1, T, 5, seed=11)[0]  # (E, T, 2)
    # (10 % of the members: the all-members rule still leaves a third of the frames complete)
    gap = R.knock_members(st[None], R.member_mask(11, 1, 5, T, 2, 0.10))[0]
    gap[:, 50:60, :] = np.nan
    dfs = [pd.DataFrame(gap[e], columns=["nose_x", "nose_y"]) for e in range(5)]
    old = sv(dfs, "nose", 10.0, 50.0, posterior_var=True, allow_missing=True)
    same = sv(dfs, "nose", 10.0, 50.0, posterior_var=True, allow_missing=True, min_members=None)
    for k in ("markers_df", "posterior_var_df"):
        pd.testing.assert_frame_equal(old[k], same[k], check_exact=True)
    assert np.isfinite(old["nll"]) and old["nll"] == same["nll"]
    assert old["n_missing"] == same["n_missing"]
    res = sv(dfs, "nose", 10.0, 50.0, posterior_var=True, allow_missing=True, min_members=3)
    y, ev, m = R.ensemble_valid(gap, "median", 3)
    assert res["n_missing"] == int((m < 3).sum()) < old["n_missing"]
    ref = G.dense(y, ev, _oracle_model("sv", y, ev, 10.0, 50.0))
    got = res["markers_df"].to_numpy()
    var = res["posterior_var_df"].to_numpy()
    assert np.isfinite(ref["out"]).all() and np.isfinite(got[:, :2]).all()
    d_out = float(np.abs(got[:, :2] - ref["out"]).max())
    d_var = float((np.abs(var[:, :2] - ref["var"]) / ref["var"]).max())
    d_nll = abs(res["nll"] - ref["nll"]) / abs(ref["nll"])
    print(f"[ensemble gaps] single-view wrapper: out {d_out:.3e} px, var rel {d_var:.3e}, "
          f"nll rel {d_nll:.3e}; missing {res['n_missing']} (all-members rule {old['n_missing']})")
    assert d_out <= OUT_TOL and d_var <= RTOL and d_nll <= NLL_RTOL
    with pytest.raises(ValueError, match="allow_missing"):
        sv(dfs, "nose", 10.0, 50.0, min_members=3)
    with pytest.raises(ValueError, match="min_members"):
        sv(dfs, "nose", 10.0, 50.0, allow_missing=True, min_members=6)


def test_wrapper_multi_cam(torch):
    from eks_amd.multiview_pca_smoother import ensemble_kalman_smoother_multi_cam as mc
    V, T = 2, 131
    cams = [f"cam{c}" for c in range(V)]
    st = members(2 * V, 1, T, 5, seed=12)[0]  # (E, T, 4)
    gap = R.knock_members(st[None], R.member_mask(12, 1, 5, T, 2 * V, 0.05))[0]
    gap[:, 60:75, 2:4] = np.nan  # camera 1 out over 15 frames

    def frames(arr):
        return [[pd.DataFrame(arr[e][:, 2 * c:2 * c + 2], columns=["x", "y"]) for e in range(5)]
                for c in range(V)]

    old = mc(frames(gap), "paw", 10.0, 25.0, cams, allow_missing=True)
    same = mc(frames(gap), "paw", 10.0, 25.0, cams, allow_missing=True, min_members=None)
    for c in cams:
        pd.testing.assert_frame_equal(old[c + "_df"], same[c + "_df"], check_exact=True)
    res = mc(frames(gap), "paw", 10.0, 25.0, cams, posterior_var=True, allow_missing=True,
             min_members=3)
    y, ev, m = R.ensemble_valid(gap, "median", 3)
    assert res["n_missing"] == int((m < 3).sum()) < old["n_missing"]
    ref = G.dense(y, ev, _oracle_model("mc", y, ev, 10.0, 25.0))
    got = np.concatenate([res[c + "_df"].to_numpy()[:, :2] for c in cams], axis=1)
    var = np.concatenate([res["posterior_var_df"][c + "_df"].to_numpy()[:, :2] for c in cams], 1)
    assert np.isfinite(ref["out"]).all() and np.isfinite(got).all() and np.isfinite(var).all()
    d_out = float(np.abs(got - ref["out"]).max())
    d_var = float((np.abs(var - ref["var"]) / ref["var"]).max())
    print(f"[ensemble gaps] multi-camera wrapper: out {d_out:.3e} px, var rel {d_var:.3e}; "
          f"missing {res['n_missing']} (all-members rule {old['n_missing']})")
    assert d_out <= OUT_TOL and d_var <= RTOL
    with pytest.raises(ValueError, match="allow_missing"):
        mc(frames(gap), "paw", 10.0, 25.0, cams, min_members=3)


KPS = ['pupil_top_r', 'pupil_right_r', 'pupil_bottom_r', 'pupil_left_r']
KEYS = ("m0", "S0", "A", "Q", "C", "means")


def test_wrapper_pupil_and_sweep(torch):
    """The pupil wrapper and its sweep with min_members against gaps_ref.dense
    on the oracle's pupil model of the reference ensemble's complete frames
    (tests/test_gpu_gaps_sweep.py's bounds: out 1e-8 px, var and NLL rtol 1e-8
    / 1e-9)."""
    from eks_amd import fit, synthetic
    from eks_amd.pupil_smoother import ensemble_kalman_smoother_pupil as pupil
    from eks_amd.pupil_smoother import pupil_smoothing_sweep
    from oracle import eks_oracle as O
    T = 131
    st = synthetic.pupil_obs(np.random.default_rng(5), 5, T).astype(np.float64)
    gap = R.knock_members(st[None], R.member_mask(13, 1, 5, T, 8, 0.02))[0]
    gap[:, 60:75, :] = np.nan  # a blink
    frames = [pd.DataFrame(gap[e], columns=list(fit.PUPIL_KEYS)) for e in range(5)]
    A = np.diag([.9999, .999, .999])
    old = pupil(frames, KPS, "tracker", A, allow_missing=True)
    same = pupil(frames, KPS, "tracker", A, allow_missing=True, min_members=None)
    pd.testing.assert_frame_equal(old["markers_df"], same["markers_df"], check_exact=True)
    res = pupil(frames, KPS, "tracker", A, posterior_var=True, allow_missing=True, min_members=3)
    y, ev, m = R.ensemble_valid(gap, "median", 3)
    assert res["n_missing"] == int((m < 3).sum()) < old["n_missing"]
    ok = np.isfinite(y).all(axis=1) & np.isfinite(ev).all(axis=1)
    ref = G.dense(y, ev, {k: O.pupil_params(y[ok], A)[k] for k in KEYS})
    order = [fit.PUPIL_KEYS.index(f"{kp}_{c}") for kp in KPS for c in "xy"]
    xy = np.arange(12) % 3 != 2
    got = res["markers_df"].to_numpy()[:, xy]
    var = res["posterior_var_df"].to_numpy()[:, xy]
    assert np.isfinite(ref["out"]).all() and np.isfinite(got).all() and np.isfinite(var).all()
    d_out = float(np.abs(got - ref["out"][:, order]).max())
    d_var = float((np.abs(var - ref["var"][:, order]) / ref["var"][:, order]).max())
    ds, cs = [0.99, 0.9999], [0.99, 0.999]
    sw = pupil_smoothing_sweep(frames, KPS, "tracker", ds, cs, allow_missing=True, min_members=3)
    nll = np.array([[G.dense(y, ev, {k: O.pupil_params(y[ok], np.diag([d, c, c]))[k]
                                     for k in KEYS})["nll"] for c in cs] for d in ds])
    d_nll = float((np.abs(sw["nll"] - nll) / np.abs(nll)).max())
    print(f"[ensemble gaps] pupil wrapper: out {d_out:.3e} px, var rel {d_var:.3e}, sweep nll rel "
          f"{d_nll:.3e}; missing {res['n_missing']} (all-members rule {old['n_missing']})")
    assert d_out <= OUT_TOL and d_var <= RTOL and d_nll <= NLL_RTOL
    i, j = np.unravel_index(np.argmin(nll), nll.shape)
    assert sw["best"] == (ds[i], cs[j]) and sw["n_missing"] == res["n_missing"]
    with pytest.raises(ValueError, match="allow_missing"):
        pupil(frames, KPS, "tracker", A, min_members=3)
    with pytest.raises(ValueError, match="allow_missing"):
        pupil_smoothing_sweep(frames, KPS, "tracker", ds, cs, min_members=3)
