"""The smoother through missing observations (eks_smooth_gaps,
batch.smooth_gaps, torch.ops.eks.smooth_gaps, allow_missing=True in the
wrappers) against tests/gaps_ref.py's dense reference: per step the observed
rows are selected, the innovation system is solved, the RTS recursions follow
and the NLL is summed over the observed entries.

Members come from eks_amd.synthetic as float32 unless stated; the models are
the oracle's on the complete data.  Every case asserts first that the
reference is finite everywhere, then compares every entry, and prints its
measured maxima before asserting.

Tolerances (the project's own): out 1e-8 px (the time-parallel algorithms
against algo 1); var rtol 1e-8 / atol 1e-12 (test_gpu_postvar.close); Vs
norm-wise rtol 1e-8 relative to the step's largest |entry| (off-diagonals
pass through zero: DESIGN.md); nll rtol 1e-9 (test_gpu_sweep); nobs exact.
Measured maxima on an MI355X over all cases: out 1.5e-12 px, var 4.8e-12,
Vs 6.1e-13, nll 3.7e-14 (the table per case is in DESIGN.md).
"""
import os

import numpy as np
import pandas as pd
import pytest

import gaps_ref as G

pytestmark = pytest.mark.gpu

OUT_TOL, RTOL, ATOL, NLL_RTOL = 1e-8, 1e-8, 1e-12, 1e-9


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture
def gaps_chunk():
    """eks_debug_set(EKS_DBG_GAPS_CHUNK, v) for one test, reset afterwards."""
    from eks_amd import _lib
    yield lambda v: _lib.debug_set(_lib.EKS_DBG_GAPS_CHUNK, v)
    _lib.debug_set(_lib.EKS_DBG_GAPS_CHUNK, 0)


def pack(models):
    from eks_amd import batch
    stk = lambda k: np.stack([m[k] for m in models])  # noqa: E731
    return batch.pack_params(stk("m0"), stk("S0"), stk("A"), stk("Q"), stk("C"), stk("means"))


def run(torch, st, models, n, r, dtype=np.float32, mode="median", **kw):
    from eks_amd import batch
    d = batch.make_time_major(st, dtype=dtype)
    res = batch.smooth_gaps(d, pack(models), n=n, r=r, mode=mode, want_var=True, want_Vs=True,
                            want_ms=True, want_nll=True, **kw)
    torch.cuda.synchronize()
    return res


def compare(res, refs, what, rows=None):
    """Every entry of out, var, ms, Vs, nll, nobs of the trajectories ``rows``
    (all by default) against the dense reference."""
    rows = range(len(refs)) if rows is None else rows
    got = {k: res[k].cpu().numpy() for k in ("out", "var", "ms", "Vs", "nll", "nobs")}
    worst = dict(out=0.0, var=0.0, var0=0.0, Vs=0.0, nll=0.0)
    for b in rows:
        ref = refs[b]
        for k in ("out", "var", "ms", "Vs"):
            assert np.isfinite(ref[k]).all(), (what, b, k, "reference not finite")
            assert np.isfinite(got[k][b]).all(), (what, b, k)
            assert got[k][b].shape == ref[k].shape, (what, b, k)
        assert np.isfinite(ref["nll"]) and np.isfinite(got["nll"][b]), (what, b)
        worst["out"] = max(worst["out"], float(np.abs(got["out"][b] - ref["out"]).max()),
                           float(np.abs(got["ms"][b] @ ref["C"].T + ref["off"] - ref["out"]).max()))
        zero = np.abs(ref["var"]) < 1e-20
        if (~zero).any():
            worst["var"] = max(worst["var"], float(
                (np.abs(got["var"][b] - ref["var"])[~zero] / np.abs(ref["var"][~zero])).max()))
        if zero.any():
            worst["var0"] = max(worst["var0"], float(np.abs(got["var"][b][zero]).max()))
        scale = np.abs(ref["Vs"]).max(axis=(1, 2))
        assert (scale > 0).all(), (what, b)
        worst["Vs"] = max(worst["Vs"], float(
            (np.abs(got["Vs"][b] - ref["Vs"]).max(axis=(1, 2)) / scale).max()))
        den = abs(ref["nll"]) if ref["nll"] != 0 else 1.0
        worst["nll"] = max(worst["nll"], abs(got["nll"][b] - ref["nll"]) / den)
    print(f"[gaps] {what}: out {worst['out']:.3e} px, var rel {worst['var']:.3e}, "
          f"Vs norm-wise {worst['Vs']:.3e}, nll rel {worst['nll']:.3e}")
    assert worst["out"] <= OUT_TOL, (what, worst)
    assert worst["var"] <= RTOL and worst["var0"] <= ATOL, (what, worst)
    assert worst["Vs"] <= RTOL, (what, worst)
    assert worst["nll"] <= NLL_RTOL, (what, worst)
    for b in rows:
        assert int(got["nobs"][b]) == refs[b]["nobs"], (what, b)


def reference(st, models, mode="median"):
    return G.reference(st, models, mode)


# -- 1: (2,2), serial scans, ragged last chunk; automatic; one chunk ----------------
@pytest.mark.parametrize("chunk", [8, 0, 136])
def test_singleview_chunked_auto_single(torch, gaps_chunk, chunk):
    from eks_amd import _lib
    g, models, ref, mask = G.case_sv131()
    gaps_chunk(chunk)
    L = _lib.load().eks_smooth_gaps_chunk_len(3, 131, 2)
    assert L == (chunk if chunk else L) and L % 8 == 0
    if chunk == 8:
        assert -(-131 // L) == 17
    if chunk == 136:
        assert L >= 131
    assert mask[0, 45:85].all() and mask[:2, 0].all() and mask[:2, -1].all() and not mask[2].any()
    res = run(torch, g, models, 2, 2)
    assert int(res["status"].abs().sum()) == 0
    compare(res, ref, f"sv B=3 T=131 chunk={chunk}")
    assert ref[2]["nobs"] == 131 * 2 and ref[0]["nobs"] < 131 * 2 - 80


# -- 2: (2,2), 263 chunks: the wave scans -----------------------------------------
def test_singleview_wave_scan(torch, gaps_chunk):
    from eks_amd import _lib
    st = G.members("sv", 2, 2100)
    models = [G.model_of("sv", st[b]) for b in range(2)]
    mask = np.random.default_rng(2100).random((2, 2100, 2)) < 0.2
    mask[0, 1000:1040] = True
    mask[:, 0] = True
    mask[:, -1] = True
    g = G.knock_out(st, mask)
    ref = reference(g, models)
    gaps_chunk(8)
    assert _lib.load().eks_smooth_gaps_chunk_len(2, 2100, 2) == 8
    assert -(-2100 // 8) == 263 > int(os.environ.get("EKS_WAVE_SCAN_CHUNKS", 24))
    res = run(torch, g, models, 2, 2)
    assert int(res["status"].abs().sum()) == 0
    compare(res, ref, "sv B=2 T=2100 chunk=8")


# -- 3: (3,8), four cameras: whole cameras missing, rank-deficient W_t ------------------
def multicam_gaps(B=3, T=131):
    st = G.members("mc", B, T)
    models = [G.model_of("mc", st[b]) for b in range(B)]
    mask = np.zeros((B, T, 8), dtype=bool)
    mask[0, 10:50, 0:2] = True    # camera 0 missing over a span
    mask[0, 30:70, 4:6] = True    # camera 2 too, overlapping
    mask[1, 20:60, 2:] = True     # one camera only: 2 observations for r = 3
    mask[1, 70, 1:] = True        # a single column
    mask[1, 90:100] = True        # nothing observed
    mask[2] = np.random.default_rng(38).random((T, 8)) < 0.5
    g = G.knock_out(st, mask)
    return g, models, mask


def test_multicam_missing_cameras(torch, gaps_chunk):
    g, models, mask = multicam_gaps()
    ref = reference(g, models)
    gaps_chunk(8)
    res = run(torch, g, models, 8, 3)
    assert int(res["status"].abs().sum()) == 0
    compare(res, ref, "mc (3,8) B=3 T=131 chunk=8")


# -- 4: runtime n: five cameras ------------------------------------------------------
def test_runtime_n_five_cameras(torch):
    st = G.members("mc", 2, 300, V=5)
    models = [G.model_of("mc", st[b]) for b in range(2)]
    mask = np.random.default_rng(10).random((2, 300, 10)) < 0.2
    mask[0, 100:140, :8] = True
    g = G.knock_out(st, mask)
    ref = reference(g, models)
    res = run(torch, g, models, 10, 3)
    assert int(res["status"].abs().sum()) == 0
    compare(res, ref, "mc n=10 B=2 T=300")


# -- 5: many trajectories: both lane mappings --------------------------------------------
@pytest.mark.parametrize("B,T", [(300, 64), (480, 24)])
def test_many_trajectories(torch, gaps_chunk, B, T):
    """B = 300: (chunk, trajectory) lanes in chunk-major order over several
    blocks; B = 480: whole blocks per chunk (the uniform-lane kernels), the
    second block of every chunk partly idle."""
    st = G.members("sv", B, T)
    models = [G.model_of("sv", st[b]) for b in range(B)]
    mask = np.random.default_rng(B).random((B, T, 2)) < 0.3
    mask[::7, 5:19] = True
    g = G.knock_out(st, mask)
    ref = reference(g, models)
    gaps_chunk(8)
    res = run(torch, g, models, 2, 2)
    assert int(res["status"].abs().sum()) == 0
    compare(res, ref, f"sv B={B} T={T} chunk=8")


# -- 6: T = 1 and T = 2 ------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2])
def test_shortest_trajectories(torch, T):
    st = G.members("sv", 3, 131)
    models = [G.model_of("sv", st[b]) for b in range(3)]
    for m in models:
        m["m0"] = np.array([0.75, -1.25])
    sub = np.ascontiguousarray(st[:, :, :T])
    mask = np.zeros((3, T, 2), dtype=bool)
    mask[0] = True          # trajectory 0: nothing observed
    mask[1, T - 1, 1] = True
    g = G.knock_out(sub, mask)
    ref = reference(g, models)
    res = run(torch, g, models, 2, 2)
    assert int(res["status"].abs().sum()) == 0
    compare(res, ref, f"sv T={T}")
    if T == 1:  # its only frame missing: the prior
        m = models[0]
        np.testing.assert_allclose(res["out"][0, 0].cpu().numpy(), m["C"] @ m["m0"] + m["means"],
                                   rtol=1e-14, atol=0)
        np.testing.assert_allclose(res["var"][0, 0].cpu().numpy(),
                                   np.einsum("ji,ik,jk->j", m["C"], m["S0"], m["C"]),
                                   rtol=1e-14, atol=0)
        assert float(res["nll"][0]) == 0.0 and int(res["nobs"][0]) == 0


# -- 7: a trajectory with nothing observed, beside normal ones ---------------------------
def test_nothing_observed_is_the_prior_carried_forward(torch, gaps_chunk):
    g, models, _, mask = G.case_sv131()
    models = [dict(m) for m in models]
    models[1]["m0"] = np.array([1.5, -2.0])
    models[1]["A"] = np.array([[0.99, 0.02], [0.0, 0.97]])
    mask = mask.copy()
    mask[1] = True
    g = G.knock_out(np.array(g), mask)
    ref = reference(g, models)
    gaps_chunk(8)
    res = run(torch, g, models, 2, 2)
    assert res["status"].cpu().tolist() == [0, 0, 0]
    compare(res, ref, "sv B=3 T=131, trajectory 1 without observations")
    assert int(res["nobs"][1]) == 0 and float(res["nll"][1]) == 0.0
    ms = res["ms"][1].cpu().numpy()
    m = models[1]["m0"]
    for t in range(131):
        if t > 0:
            m = models[1]["A"] @ m
        np.testing.assert_allclose(ms[t], m, rtol=1e-12, atol=0)


# -- 8: complete data: the existing entry points ---------------------------------------------
@pytest.mark.parametrize("kind,n,r", [("sv", 2, 2), ("mc", 8, 3)])
def test_complete_data_equals_smooth(torch, gaps_chunk, kind, n, r):
    from eks_amd import batch
    st = G.members(kind, 3, 131)
    models = [G.model_of(kind, st[b]) for b in range(3)]
    gaps_chunk(8)
    d = batch.make_time_major(st, dtype=np.float32)
    params = pack(models)
    a = batch.smooth(d, params, n=n, r=r, want_var=True, check=True)
    nll = batch.nll(d, params, n=n, r=r)
    res = batch.smooth_gaps(d, params, n=n, r=r, want_var=True, want_nll=True, check=True)
    d_out = float((res["out"] - a["out"]).abs().max())
    d_var = float(((res["var"] - a["var"]).abs() / a["var"].abs()).max())
    d_nll = float(((res["nll"] - nll).abs() / nll.abs()).max())
    print(f"[gaps] {kind} complete data vs smooth: out {d_out:.3e} px, var rel {d_var:.3e}, "
          f"nll rel {d_nll:.3e}")
    assert torch.isfinite(a["out"]).all() and torch.isfinite(a["var"]).all()
    assert d_out <= OUT_TOL and d_var <= RTOL and d_nll <= NLL_RTOL
    assert res["nobs"].cpu().tolist() == [131 * n] * 3
    compare(run(torch, st, models, n, r), reference(st, models), f"{kind} complete data")


# -- 9: the missing rule -------------------------------------------------------------------
def test_missing_rule_members(torch, gaps_chunk):
    g, models, ref, mask = G.case_sv131()
    gaps_chunk(8)
    base = run(torch, g, models, 2, 2)
    compare(base, ref, "sv, member 0 NaN")
    variants = {}
    v = np.array(g)
    v[:, 0][mask] = g[:, 1][mask]        # member 0 restored to a finite value ...
    v[:, 3][mask] = np.nan               # ... one other NaN member of five
    variants["member 3 NaN"] = v
    v = np.array(g)
    v[:, 0][mask] = g[:, 1][mask]
    v[:, 2][mask] = np.inf               # one +inf member: a NaN variance
    variants["member 2 +inf"] = v
    v = np.array(g)
    for e in range(5):
        v[:, e][mask] = np.nan           # all members NaN
    variants["all members NaN"] = v
    for name, v in variants.items():
        res = run(torch, v, models, 2, 2)
        for k in ("out", "var", "ms", "Vs", "nll", "nobs", "status"):
            assert torch.equal(res[k], base[k]), (name, k)
    # float64 members; the mean
    compare(run(torch, g, models, 2, 2, dtype=np.float64), ref, "sv, float64 members")
    compare(run(torch, g, models, 2, 2, mode="mean"), reference(g, models, "mean"), "sv, mean")


def test_missing_rule_yev_handoff_is_bit_identical(torch, gaps_chunk):
    from eks_amd import batch, core
    g, models, ref, _ = G.case_sv131()
    gaps_chunk(8)
    yev, preds, ev = core.ensemble_handoff(np.array(g[0]))
    assert np.isnan(preds).any() and np.isnan(ev).any()
    params = pack(models[:1])
    kw = dict(n=2, r=2, want_var=True, want_Vs=True, want_ms=True, want_nll=True)
    a = batch.smooth_gaps(yev, params, **kw)
    d = batch.make_time_major(g[:1], dtype=np.float64)
    b = batch.smooth_gaps(d, params, **kw)
    for k in ("out", "var", "ms", "Vs", "nll", "nobs", "status"):
        assert torch.equal(a[k], b[k]), k
    compare(a, ref[:1], "sv Yev")


# -- 10: identical members on an observed column ----------------------------------------------
def test_exact_observation_is_flagged(torch, gaps_chunk):
    from eks_amd import _lib
    g, models, ref, mask = G.case_sv131()
    assert not mask[1, 60].any()
    ex = np.array(g)
    ex[1, :, 60, 0] = ex[1, 0, 60, 0]  # trajectory 1, frame 60, x: all members equal
    gaps_chunk(8)
    res = run(torch, ex, models, 2, 2)
    assert res["status"].cpu().tolist() == [0, _lib.EKS_STATUS_SCAN, 0]
    for k in ("out", "var", "ms", "Vs"):
        assert torch.isnan(res[k][1]).all(), k
    assert torch.isnan(res["nll"][1])
    compare(res, ref, "sv exact observation: the other trajectories", rows=[0, 2])
    with pytest.raises(ValueError, match="zero ensemble variance"):
        run(torch, ex, models, 2, 2, check=True)
    ex[1, 0, 60, 0] = np.nan  # the same column marked missing
    res = run(torch, ex, models, 2, 2, check=True)
    assert res["status"].cpu().tolist() == [0, 0, 0]
    compare(res, reference(ex, models), "sv exact observation marked missing")


# -- 11: reproducible; the operator -------------------------------------------------------------
@pytest.mark.parametrize("T,chunk", [(131, 8), (2100, 8)])
def test_two_calls_bit_identical_and_operator(torch, gaps_chunk, T, chunk):
    from eks_amd import batch
    import eks_amd.ops  # noqa: F401
    B = 3 if T == 131 else 2
    st = G.members("mc", B, T)
    models = [G.model_of("mc", st[b]) for b in range(B)]
    mask = np.random.default_rng(T).random((B, T, 8)) < 0.3
    g = G.knock_out(st, mask)
    gaps_chunk(chunk)
    a = run(torch, g, models, 8, 3)
    b = run(torch, g, models, 8, 3)
    for k in ("out", "var", "ms", "Vs", "nll", "nobs", "status"):
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a["out"]).all() and int(a["status"].abs().sum()) == 0
    d = batch.make_time_major(g, dtype=np.float32)
    out, var, nll, nobs, status = torch.ops.eks.smooth_gaps(d, pack(models), 8, 3, "median")
    assert torch.equal(out, a["out"].contiguous()) and torch.equal(var, a["var"].contiguous())
    assert torch.equal(nll, a["nll"]) and torch.equal(nobs, a["nobs"])
    assert torch.equal(status, a["status"])
    assert nobs.cpu().tolist() == [int((~mask[b]).sum()) for b in range(B)]


# -- 12: the wrappers ----------------------------------------------------------------------------
def _oracle_model(kind, preds, ev, s, q):
    from oracle import eks_oracle as O
    ok = np.isfinite(preds).all(axis=1) & np.isfinite(ev).all(axis=1)
    p = (O.singleview_params if kind == "sv" else O.multicam_params)(preds[ok], ev[ok], s, q)
    return {k: p[k] for k in ("m0", "S0", "A", "Q", "C", "means")}


def test_wrapper_single_view(torch):
    from eks_amd.singleview_smoother import ensemble_kalman_smoother_single_view
    st = G.members("sv", 1, 200)[0]  # (E, T, 2)
    dfs = [pd.DataFrame(st[e], columns=["nose_x", "nose_y"]) for e in range(5)]
    a = ensemble_kalman_smoother_single_view(dfs, "nose", 10.0, 50.0, posterior_var=True)
    b = ensemble_kalman_smoother_single_view(dfs, "nose", 10.0, 50.0, posterior_var=True,
                                             allow_missing=True)
    assert set(b) == set(a) | {"n_missing"} and b["n_missing"] == 0
    d = float(np.abs(a["markers_df"].to_numpy()[:, :2] - b["markers_df"].to_numpy()[:, :2]).max())
    print(f"[gaps] single-view wrapper, gap-free: {d:.3e} px")
    assert np.isfinite(a["markers_df"].to_numpy()[:, :2]).all() and d <= OUT_TOL
    assert abs(a["nll"] - b["nll"]) <= NLL_RTOL * abs(a["nll"])
    gap = st.copy()
    gap[:, 80:110, :] = np.nan  # the keypoint NaN over 30 frames, every member
    gap[2, 150, 1] = np.nan     # and one member's y at one frame
    dfs = [pd.DataFrame(gap[e], columns=["nose_x", "nose_y"]) for e in range(5)]
    res = ensemble_kalman_smoother_single_view(dfs, "nose", 10.0, 50.0, posterior_var=True,
                                               allow_missing=True)
    assert res["n_missing"] == 61
    y, ev = G.ensemble(gap)
    ref = G.dense(y, ev, _oracle_model("sv", y, ev, 10.0, 50.0))
    got = res["markers_df"].to_numpy()
    var = res["posterior_var_df"].to_numpy()
    assert np.isfinite(ref["out"]).all() and np.isfinite(got[:, :2]).all()
    d_out = float(np.abs(got[:, :2] - ref["out"]).max())
    d_var = float((np.abs(var[:, :2] - ref["var"]) / ref["var"]).max())
    d_nll = abs(res["nll"] - ref["nll"]) / abs(ref["nll"])
    print(f"[gaps] single-view wrapper with a 30-frame gap: out {d_out:.3e} px, "
          f"var rel {d_var:.3e}, nll rel {d_nll:.3e}")
    assert d_out <= OUT_TOL and d_var <= RTOL and d_nll <= NLL_RTOL
    assert np.isnan(got[:, 2]).all()
    with pytest.raises(ValueError, match="smooth_param"):
        ensemble_kalman_smoother_single_view(dfs, "nose", None, 50.0, allow_missing=True)


def test_wrapper_multi_cam(torch):
    from eks_amd.multiview_pca_smoother import ensemble_kalman_smoother_multi_cam
    V, T = 4, 200
    cams = [f"cam{c}" for c in range(V)]
    st = G.members("mc", 1, T)[0]  # (E, T, 8)

    def frames(arr):
        return [[pd.DataFrame(arr[e][:, 2 * c:2 * c + 2], columns=["x", "y"]) for e in range(5)]
                for c in range(V)]

    a = ensemble_kalman_smoother_multi_cam(frames(st), "paw", 10.0, 25.0, cams)
    b = ensemble_kalman_smoother_multi_cam(frames(st), "paw", 10.0, 25.0, cams,
                                           allow_missing=True)
    assert set(b) == set(a) | {"n_missing"} and b["n_missing"] == 0
    d = max(float(np.abs(a[c + "_df"].to_numpy()[:, :2] - b[c + "_df"].to_numpy()[:, :2]).max())
            for c in cams)
    print(f"[gaps] multi-camera wrapper, gap-free: {d:.3e} px")
    assert d <= OUT_TOL
    gap = st.copy()
    gap[:, 60:110, 2:4] = np.nan  # camera 1's columns NaN over 50 frames
    res = ensemble_kalman_smoother_multi_cam(frames(gap), "paw", 10.0, 25.0, cams,
                                             posterior_var=True, allow_missing=True)
    assert res["n_missing"] == 100
    y, ev = G.ensemble(gap)
    ref = G.dense(y, ev, _oracle_model("mc", y, ev, 10.0, 25.0))
    assert np.isfinite(ref["out"]).all() and np.isfinite(ref["var"]).all()
    got = np.concatenate([res[c + "_df"].to_numpy()[:, :2] for c in cams], axis=1)
    var = np.concatenate([res["posterior_var_df"][c + "_df"].to_numpy()[:, :2] for c in cams], 1)
    assert np.isfinite(got).all() and np.isfinite(var).all()
    d_out = float(np.abs(got - ref["out"]).max())
    d_var = float((np.abs(var - ref["var"]) / ref["var"]).max())
    print(f"[gaps] multi-camera wrapper, camera 1 missing over 50 frames: out {d_out:.3e} px, "
          f"var rel {d_var:.3e}")
    assert d_out <= OUT_TOL and d_var <= RTOL
    with pytest.raises(ValueError, match="smooth_param"):
        ensemble_kalman_smoother_multi_cam(frames(gap), "paw", None, 25.0, cams,
                                           allow_missing=True)
