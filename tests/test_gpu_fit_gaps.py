"""The model fit through missing observations (eks_fit_gaps, batch.fit_gaps,
torch.ops.eks.fit_gaps) against the host route the wrappers take with
``allow_missing=True``: the ensemble of every frame, the complete frames
``ok = smoothers._complete_frames(preds, ev)``, and ``fit.singleview_model`` /
``fit.multicam_model`` on ``preds[ok], ev[ok]``.

Inputs come from tests/gaps_ref.py (members, knock_out, ensemble).  Every
trajectory of every case is compared; a trajectory without a complete frame
has no host model (np.percentile of nothing) and must report
EKS_STATUS_SINGULAR with no kept frame.

The host route's ensemble is numpy's (gaps_ref.ensemble) everywhere but in the
ties case.  There the reference takes the ensemble as the wrappers do, from
the device hand-off (core.ensemble_handoff): the device's variance is numpy's
to 2 ulp (csrc/ensemble.hpp: one multiplication by 1 / E^2 for numpy's two
divisions), and on members quantised to 0.25 px that decides which of the
tied worst variances equal the threshold bit for bit -- with numpy's variances
the host keeps 3, 248 and 810 frames where the device, on its own variances,
keeps 2, 246 and 808 (q = 0, 10, 33.3; measured on an MI355X), as
test_gpu_fit_mask.py's reference (core.ensemble_array) already allows for.

Tolerances are those of the device fit against the host fit
(tests/test_gpu_parity.py): single-view rtol 1e-9 on every block; multicam
offset 1e-9, C up to column sign 1e-7, S0 1e-8, Q with the sign outer product
1e-7.  The counts of complete and kept frames are exact.  The pipeline case
uses tests/test_gpu_gaps.py's bounds: out 1e-8 px, var rtol 1e-8, NLL rtol
1e-9.
"""
import warnings

import numpy as np
import pytest

import gaps_ref as G

pytestmark = pytest.mark.gpu

S = 0.01  # smooth_param of every fit here
OUT_TOL, RTOL, NLL_RTOL = 1e-8, 1e-8, 1e-9


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _unpack(p, n, r):
    o = 0
    out = {}
    for k, shp in (("m0", (r,)), ("S0", (r, r)), ("A", (r, r)), ("Q", (r, r)), ("C", (n, r)),
                   ("offset", (n,))):
        sz = int(np.prod(shp))
        out[k] = p[o:o + sz].reshape(shp)
        o += sz
    return out


def _close(a, b, rtol):
    a = np.asarray(a)
    b = np.asarray(b)
    scale = max(1.0, float(np.nanmax(np.abs(b))) if b.size and not np.isnan(b).all() else 1.0)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * scale, equal_nan=True)


def host_fit(stack, kind, q, mode="median", handoff=False):
    """(model or None, ok) of members (E, T, n): the wrappers' host route
    (``handoff``: on the device ensemble the wrappers fit on)."""
    from eks_amd import core, fit
    from eks_amd.smoothers import _complete_frames
    preds, ev = core.ensemble_handoff(stack, mode)[1:] if handoff else G.ensemble(stack, mode)
    ok = _complete_frames(preds, ev)
    if not ok.any():
        return None, ok
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = fit.singleview_model if kind == "singleview" else fit.multicam_model
        return f(preds[ok], ev[ok], S, q), ok


def device_fit(st, kind, q, mode="median", dtype=np.float32, check=False, **kw):
    from eks_amd import batch
    n = st.shape[3]
    d = batch.make_time_major(st, dtype=dtype)
    return batch.fit_gaps(d, kind=kind, n=n, r=2 if kind == "singleview" else 3, smooth_param=S,
                          quantile_keep=q, mode=mode, check=check, **kw)


def compare(res, st, kind, q, mode="median", what="", need_finite=False, handoff=False):
    """Every trajectory of members st (B, E, T, n) against the host route."""
    from eks_amd import _lib
    B, _, _, n = st.shape
    r = 2 if kind == "singleview" else 3
    params = res["params"].cpu().numpy()
    status = res["status"].cpu().numpy()
    nc = res["ncomplete"].cpu().numpy()
    nk = res["nkept"].cpu().numpy()
    kept = []
    for b in range(B):
        ref, ok = host_fit(st[b], kind, q, mode, handoff)
        assert int(nc[b]) == int(ok.sum()), (what, b, int(nc[b]), int(ok.sum()))
        if ref is None:
            assert not need_finite
            assert status[b] == _lib.EKS_STATUS_SINGULAR and nk[b] == 0, (what, b)
            kept.append(0)
            continue
        kept.append(len(ref["keep"]))
        assert int(nk[b]) == len(ref["keep"]), (what, b, int(nk[b]), len(ref["keep"]))
        assert status[b] == 0, (what, b)
        if need_finite:
            for k in ("S0", "Q", "C", "offset"):
                assert np.isfinite(ref[k]).all(), (what, b, k, "reference not finite")
        got = _unpack(params[b], n, r)
        if kind == "singleview":
            for k in ("m0", "S0", "A", "Q", "C", "offset"):
                _close(got[k], ref[k], 1e-9)
        else:
            _close(got["offset"], ref["offset"], 1e-9)
            _close(got["A"], ref["A"], 1e-9)
            np.testing.assert_array_equal(got["m0"], ref["m0"])
            # axes up to sign; S0 is sign-free, Q flips with the axis signs
            sgn = np.sign(np.sum(got["C"] * ref["C"], axis=0))
            _close(got["C"] * sgn, ref["C"], 1e-7)
            _close(got["S0"], ref["S0"], 1e-8)
            _close(got["Q"] * np.outer(sgn, sgn), ref["Q"], 1e-7)
    if B <= 8:
        print(f"[fit gaps] {what}: complete {nc.tolist()}, kept {kept}")
    else:
        print(f"[fit gaps] {what}: complete {nc.min()}..{nc.max()}, kept {min(kept)}..{max(kept)}")
    return kept


def random_mask(seed, B, T, n, frac):
    return np.random.default_rng(seed).random((B, T, n)) < frac


# -- 1: parity with gaps ---------------------------------------------------------
CASE1 = [("singleview", 1, 131, 0.20, 50.0), ("singleview", 1, 4097, 0.05, 25.0),
         ("multicam", 2, 700, 0.05, 25.0), ("multicam", 4, 700, 0.03, 25.0),
         ("multicam", 6, 700, 0.02, 25.0), ("multicam", 8, 700, 0.02, 25.0)]


def case1_members(kind, V, T, frac, E):
    n = 2 * V
    st = G.members("sv" if kind == "singleview" else "mc", 4, T, V=V, E=E)
    mask = random_mask(T + n, 4, T, n, frac)
    mask[0, 0] = True
    mask[0, -1] = True
    mask[1, 40:90, 0:2] = True
    mask[3] = False
    return G.knock_out(st, mask)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode,E", [("median", 5), ("median", 4), ("mean", 5), ("mean", 4)])
@pytest.mark.parametrize("kind,V,T,frac,q", CASE1)
def test_parity_with_gaps(torch, kind, V, T, frac, q, mode, E, dtype):
    st = case1_members(kind, V, T, frac, E)
    res = device_fit(st, kind, q, mode, dtype)
    kept = compare(res, st, kind, q, mode, f"{kind} V={V} T={T} {mode} E={E} {dtype.__name__}",
                   need_finite=True)
    assert min(kept) >= 24 and max(kept) <= 1025, kept


# -- 2: rows where the mask and the ranks can go wrong -----------------------------
@pytest.mark.parametrize("T", [2, 63, 64, 65, 1000, 4000, 4097, 8010, 70001])
def test_row_lengths(torch, T):
    """Rows shorter than a wave, exactly one mask word, ragged last words,
    lengths where the last unrolled round of the key loop ends inside a wave
    (4000, 8010), and a row past 65 536 frames (the 1024-thread form); a row
    whose first complete frame lies in the second mask word and one with a
    whole accumulation chunk missing."""
    B = 5
    st = G.members("sv", B, T, E=3, seed=T)
    if T == 2:
        mask = np.zeros((B, T, 2), bool)
        mask[1, 0, 1] = True   # one frame missing
        mask[2] = True         # both missing
        mask[3, 1, 0] = True
    else:
        mask = random_mask(T, B, T, 2, 0.05)  # ~90 % of the frames complete
        if T >= 65:
            mask[1, 0:64] = True
        if T > 48:
            mask[2, 16:48] = True
    g = G.knock_out(st, mask)
    res = device_fit(g, "singleview", 25.0, dtype=np.float64)
    compare(res, g, "singleview", 25.0, what=f"rows T={T}")
    if T == 2:
        assert res["ncomplete"].cpu().tolist() == [2, 1, 0, 1, 2]


# -- 3: both accumulation lane mappings ------------------------------------------
@pytest.mark.parametrize("B,T", [(5, 3001), (70, 300)])
def test_lane_mappings(torch, B, T):
    """(5, 3001): 64 chunks of a trajectory per wave, merged by the wave;
    (70, 300): trajectory-fastest lanes, 18 chunks."""
    g = G.knock_out(G.members("sv", B, T), random_mask(B + T, B, T, 2, 0.10))
    res = device_fit(g, "singleview", 25.0)
    compare(res, g, "singleview", 25.0, what=f"lanes B={B} T={T}")


# -- 4: ties --------------------------------------------------------------------
@pytest.mark.parametrize("q", [0.0, 10.0, 33.3, 50.0, 99.9, 100.0])
def test_ties_quantised_members(torch, q):
    """Members on a 0.25 px grid: few distinct worst variances, so the
    threshold often equals a key; the kept-frame count is the host's."""
    from eks_amd import core, synthetic
    rng = np.random.default_rng(int(q * 10) + 1)
    B, E, T = 8, 5, 3001
    st = np.stack([synthetic.singleview_obs(rng, E, T)[:, :, 0] for _ in range(B)])
    st = (np.round(st * 4.0) / 4.0).astype(np.float32).astype(np.float64)
    g = G.knock_out(st, random_mask(int(q * 10) + 2, B, T, 2, 0.10))
    res = device_fit(g, "singleview", q)
    compare(res, g, "singleview", q, what=f"ties q={q}", handoff=True)
    # numpy's ensemble marks the same frames complete and agrees to rounding
    for b in range(B):
        (y0, e0), (y1, e1) = G.ensemble(g[b]), core.ensemble_handoff(g[b])[1:]
        ok = np.isfinite(e0).all(axis=1)
        assert (ok == np.isfinite(e1).all(axis=1)).all()
        np.testing.assert_array_equal(y0[ok], y1[ok])
        np.testing.assert_allclose(e1[ok], e0[ok], rtol=1e-15)


# -- 5: the missing rule ---------------------------------------------------------
@pytest.mark.parametrize("mode", ["median", "mean"])
def test_missing_rule_nonfinite_members(torch, mode):
    """A +inf member, a -inf member and members +-1e200 (the variance
    overflows, the average stays finite) make their frame missing exactly as
    a NaN member does: the same parameter rows, bit for bit."""
    B, T = 4, 200
    st = G.members("sv", B, T, seed=55)
    a, nan = st.copy(), st.copy()
    a[0, 1, 0, 0] = np.inf       # frame 0: the shift comes from frame 1
    a[1, 2, 10, 1] = -np.inf
    a[2, 0, 20, 0], a[2, 4, 20, 0] = 1e200, -1e200
    a[3, 3, 199, 1] = np.inf     # the last frame
    for b, t in ((0, 0), (1, 10), (2, 20), (3, 199)):
        nan[b, 0, t, :] = np.nan
    y, ev = G.ensemble(a[2], mode)
    assert np.isfinite(y[20]).all() and np.isinf(ev[20, 0])
    res = device_fit(a, "singleview", 50.0, mode, np.float64)
    compare(res, a, "singleview", 50.0, mode, f"non-finite members {mode}")
    assert res["ncomplete"].cpu().tolist() == [T - 1] * B
    res_nan = device_fit(nan, "singleview", 50.0, mode, np.float64)
    assert res_nan["ncomplete"].cpu().tolist() == [T - 1] * B
    np.testing.assert_array_equal(res["params"].cpu().numpy(), res_nan["params"].cpu().numpy())
    np.testing.assert_array_equal(res["nkept"].cpu().numpy(), res_nan["nkept"].cpu().numpy())


# -- 6: degenerate rows ----------------------------------------------------------
@pytest.mark.parametrize("kind,V", [("singleview", 1), ("multicam", 4), ("multicam", 6)])
def test_degenerate_rows(torch, kind, V):
    """A row with nothing complete: EKS_STATUS_SINGULAR, no kept frame, the
    other rows bit-identical to a run without that row's gaps.  Single view
    also: a row with exactly one complete frame (offset its average, S0 = 0,
    Q NaN, status 0) and one with exactly two."""
    from eks_amd import _lib
    B, T, n = 4, 131, 2 * V
    st = G.members("sv" if kind == "singleview" else "mc", B, T, V=V)
    mask = random_mask(11 + n, B, T, n, 0.03)
    if kind == "singleview":
        mask[2] = True
        mask[2, 77] = False
        mask[3] = True
        mask[3, 5] = False
        mask[3, 100] = False
    without = G.knock_out(st, mask)
    mask[1, :, n - 1] = True  # one column gone in every frame
    g = G.knock_out(st, mask)
    res = device_fit(g, kind, 25.0)
    compare(res, g, kind, 25.0, what=f"degenerate {kind} n={n}")
    status = res["status"].cpu().numpy()
    assert status[1] == _lib.EKS_STATUS_SINGULAR and (status[[0, 2, 3]] == 0).all()
    assert int(res["nkept"][1]) == 0 and int(res["ncomplete"][1]) == 0
    if kind == "singleview":
        assert res["ncomplete"].cpu().tolist()[2:] == [1, 2]
        row = _unpack(res["params"][2].cpu().numpy(), 2, 2)
        y, _ = G.ensemble(g[2])
        np.testing.assert_array_equal(row["offset"], y[77])
        np.testing.assert_array_equal(row["S0"], np.zeros((2, 2)))
        assert np.isnan(row["Q"]).all()
    ref = device_fit(without, kind, 25.0)
    rows = [0, 2, 3]
    assert np.array_equal(res["params"].cpu().numpy()[rows], ref["params"].cpu().numpy()[rows],
                          equal_nan=True)
    for k in ("status", "ncomplete", "nkept"):
        np.testing.assert_array_equal(res[k].cpu().numpy()[rows], ref[k].cpu().numpy()[rows])
    with pytest.raises(ValueError, match="1 of 4 trajectories"):
        device_fit(g, kind, 25.0, check=True)
    device_fit(without, kind, 25.0, check=True)


# -- 7: invariant on gap-free members ----------------------------------------------
def _planes(yev):
    """The y and the ev planes' bytes of a Yev (not the alignment gap)."""
    from eks_amd import _lib
    B, T, _, n = yev.shape
    ys = 4 if yev.code == _lib.EKS_YEV32 else 8
    off = (T * n * B * ys + 255) // 256 * 256
    return yev.buf[:T * n * B * ys].cpu().numpy(), yev.buf[off:off + T * n * B * 8].cpu().numpy()


@pytest.mark.parametrize("kind,V,B,T", [("singleview", 1, 4, 700), ("multicam", 4, 4, 700),
                                        ("multicam", 6, 4, 700), ("singleview", 1, 5, 3001),
                                        ("singleview", 1, 70, 300)])
@pytest.mark.parametrize("mode,dtype", [("median", np.float32), ("mean", np.float64)])
def test_gap_free_members_bit_identical_to_fit(torch, kind, V, B, T, mode, dtype):
    from eks_amd import batch
    n, r = 2 * V, 2 if kind == "singleview" else 3
    st = G.members("sv" if kind == "singleview" else "mc", B, T, V=V)
    d = batch.make_time_major(st, dtype=dtype)
    kw = dict(kind=kind, n=n, r=r, smooth_param=S, quantile_keep=25.0, mode=mode)
    p0, s0, y0 = batch.fit(d, keep_yev=True, **kw)
    res = batch.fit_gaps(d, **kw)
    np.testing.assert_array_equal(res["params"].cpu().numpy(), p0.cpu().numpy())
    np.testing.assert_array_equal(res["status"].cpu().numpy(), s0.cpu().numpy())
    assert (res["yev"].code, res["yev"].shape, res["yev"].mode) == (y0.code, y0.shape, y0.mode)
    for a, b in zip(_planes(res["yev"]), _planes(y0)):
        np.testing.assert_array_equal(a, b)
    assert res["ncomplete"].cpu().tolist() == [T] * B
    compare(res, st, kind, 25.0, mode, f"gap-free {kind} n={n} B={B} T={T}")
    # a Yev of sufficient size is reused
    again = batch.fit_gaps(d, keep_yev=res["yev"], **kw)
    assert again["yev"].buf.data_ptr() == res["yev"].buf.data_ptr()
    np.testing.assert_array_equal(again["params"].cpu().numpy(), p0.cpu().numpy())


# -- 8: pipeline -----------------------------------------------------------------
@pytest.mark.parametrize("kind,V,T,frac", [("singleview", 1, 131, 0.20), ("multicam", 4, 700, 0.03)])
def test_pipeline_fit_gaps_then_smooth_gaps(torch, kind, V, T, frac):
    """fit_gaps -> smooth_gaps on the hand-off planes against the host fit ->
    the dense reference; and torch.ops.eks.fit_gaps returns batch.fit_gaps's
    tensors."""
    from eks_amd import batch
    n, r, q = 2 * V, 2 if kind == "singleview" else 3, 25.0
    g = case1_members(kind, V, T, frac, 5)
    B = g.shape[0]
    d = batch.make_time_major(g, dtype=np.float32)
    res = batch.fit_gaps(d, kind=kind, n=n, r=r, smooth_param=S, quantile_keep=q)
    sm = batch.smooth_gaps(res["yev"], res["params"], n=n, r=r, want_var=True, want_nll=True,
                           check=True)
    out, var, nll = (sm[k].cpu().numpy() for k in ("out", "var", "nll"))
    nobs = sm["nobs"].cpu().numpy()
    worst = dict(out=0.0, var=0.0, nll=0.0)
    for b in range(B):
        model, ok = host_fit(g[b], kind, q)
        p = dict(m0=model["m0"], S0=model["S0"], A=model["A"], Q=model["Q"], C=model["C"],
                 means=model["offset"])
        y, ev = G.ensemble(g[b])
        ref = G.dense(y, ev, p)
        for k in ("out", "var"):
            assert np.isfinite(ref[k]).all() and np.isfinite(sm[k][b].cpu().numpy()).all(), (b, k)
        assert int(nobs[b]) == ref["nobs"]
        worst["out"] = max(worst["out"], float(np.abs(out[b] - ref["out"]).max()))
        worst["var"] = max(worst["var"], float((np.abs(var[b] - ref["var"]) / ref["var"]).max()))
        worst["nll"] = max(worst["nll"], abs(nll[b] - ref["nll"]) / abs(ref["nll"]))
    print(f"[fit gaps] pipeline {kind} T={T}: out {worst['out']:.3e} px, var rel "
          f"{worst['var']:.3e}, nll rel {worst['nll']:.3e}")
    assert worst["out"] <= OUT_TOL and worst["var"] <= RTOL and worst["nll"] <= NLL_RTOL, worst
    # the operator
    import eks_amd.ops  # noqa: F401
    params, status, yev, nc, nk = torch.ops.eks.fit_gaps(d, kind, n, r, S, q, "median")
    np.testing.assert_array_equal(params.cpu().numpy(), res["params"].cpu().numpy())
    np.testing.assert_array_equal(status.cpu().numpy(), res["status"].cpu().numpy())
    np.testing.assert_array_equal(nc.cpu().numpy(), res["ncomplete"].cpu().numpy())
    np.testing.assert_array_equal(nk.cpu().numpy(), res["nkept"].cpu().numpy())
    assert yev.dtype == torch.uint8 and yev.numel() == res["yev"].buf.numel()
    op_yev = batch.Yev(yev, B, T, 5, n, res["yev"].code, "median")
    for a, b in zip(_planes(op_yev), _planes(res["yev"])):
        np.testing.assert_array_equal(a, b)
