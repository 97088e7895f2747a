"""The likelihood sweep through missing observations (eks_nll_sweep_gaps,
batch.nll_sweep_gaps, torch.ops.eks.nll_sweep_gaps,
select_smooth_param(allow_missing=True), allow_missing=True in the pupil
wrappers) against tests/gaps_ref.py's dense reference: per step the observed
rows are selected, the innovation system is solved and the NLL is summed over
the observed entries.

Bounds (the project's own): rtol 1e-9 against the dense reference
(test_gpu_gaps / test_gpu_sweep), 2e-9 against per-candidate
batch.smooth_gaps(want_nll=True) and against batch.nll_sweep on complete data
(each is within 1e-9 of its reference), nobs exact; the wrappers 1e-8 px on
the markers and rtol 1e-8 on the variances (test_gpu_gaps).  On the shared
inputs every reference NLL is finite, |NLL| / nobs >= 1, every argmin over the
candidates is interior and best and second best differ by >= 2.6e-4 relative
(test_gaps_sweep_host.py asserts it).  Each check prints its measured maximum
before asserting; the table per case is in DESIGN.md.  Measured maxima on an
MI355X: against the dense reference 6.2e-10 at n = 10 and 2.8e-11 at (3,8),
both at the Q x 1e3 candidate (a large P against a rank-deficient W_t), at
most 1.2e-13 everywhere else; against smooth_gaps per candidate 7.9e-11;
against nll_sweep on complete data 9.2e-15; the wrappers 7.1e-15 px and 1e-14.
"""
import os

import numpy as np
import pandas as pd
import pytest

import gaps_ref as G
import gaps_sweep_data as S

pytestmark = pytest.mark.gpu

RTOL_REF, RTOL_ROUTE = 1e-9, 2e-9
OUT_TOL, VAR_RTOL = 1e-8, 1e-8
K7 = len(S.SCALES)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture
def gs_chunk():
    """eks_debug_set(EKS_DBG_GAPS_SWEEP_CHUNK, v) for one test, reset afterwards."""
    from eks_amd import _lib
    yield lambda v: _lib.debug_set(_lib.EKS_DBG_GAPS_SWEEP_CHUNK, v)
    _lib.debug_set(_lib.EKS_DBG_GAPS_SWEEP_CHUNK, 0)


def close(got, ref, what, rtol, cols=None):
    """Relative error of every entry (of the trajectories ``cols``); a
    reference of exactly 0 asks for exactly 0."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if cols is not None:
        got, ref = got[:, cols], ref[:, cols]
    assert np.isfinite(ref).all(), (what, "reference not finite")
    zero = ref == 0
    assert (got[zero] == 0).all(), what
    rel = float(np.max(np.abs(got - ref)[~zero] / np.abs(ref[~zero]))) if (~zero).any() else 0.0
    print(f"[gaps sweep] {what}: max rel err {rel:.3e} (bound {rtol:.0e})")
    assert np.isfinite(got).all(), what
    assert rel <= rtol, (what, rel)


def sweep(torch, g, cands, n, r, dtype=np.float32, mode="median", check=False):
    """batch.nll_sweep_gaps of cands[k][b] on members g (B, E, T, n) ->
    (nll (K, B) numpy, nobs (B,) numpy, status (K, B) numpy, the result dict,
    the member view, the rows)."""
    from eks_amd import batch
    d = batch.make_time_major(g, dtype=dtype)
    rows = torch.from_numpy(S.rows_of(cands)).cuda()
    res = batch.nll_sweep_gaps(d, rows, K=len(cands), n=n, r=r, mode=mode, check=check)
    torch.cuda.synchronize()
    return (res["nll"].cpu().numpy(), res["nobs"].cpu().numpy(), res["status"].cpu().numpy(), res,
            d, rows)


def per_candidate(d, rows, K, n, r, mode="median"):
    """K back-to-back batch.smooth_gaps(want_nll=True) calls: the route without the sweep."""
    from eks_amd import batch
    B = d.shape[0]
    return np.stack([batch.smooth_gaps(d, rows[k * B:(k + 1) * B].contiguous(), n=n, r=r,
                                       mode=mode, want_nll=True)["nll"].cpu().numpy()
                     for k in range(K)])


def both_bounds(torch, name, n, r, what):
    c = S.case(name)
    cands = S.scale_candidates(c["models"])
    got, nobs, status, _, d, rows = sweep(torch, c["g"], cands, n, r)
    assert not status.any(), status
    close(got, c["ref"], f"{what} vs dense", RTOL_REF)
    close(got, per_candidate(d, rows, K7, n, r), f"{what} vs smooth_gaps per candidate", RTOL_ROUTE)
    np.testing.assert_array_equal(nobs, c["nobs"])
    return got


# -- 1: (2,2), serial scan, ragged last chunk, voids across boundaries; automatic; one chunk --
@pytest.mark.parametrize("chunk", [8, 0, 136])
def test_singleview_chunked_auto_single(torch, gs_chunk, chunk):
    from eks_amd import _lib
    gs_chunk(chunk)
    L = _lib.load().eks_nll_sweep_gaps_chunk_len(3, K7, 131, 2)
    assert L == (chunk if chunk else L) and L % 8 == 0
    if chunk == 8:
        assert -(-131 // L) == 17 and 131 - 16 * 8 == 3
    if chunk == 136:
        assert L >= 131
    mask = S.case("sv131")["mask"]
    assert mask[0, 45:85].all() and mask[1, 3:43].all() and not mask[2].any()
    both_bounds(torch, "sv131", 2, 2, f"sv B=3 T=131 chunk={chunk}")


# -- 2: (2,2), 263 chunks: one wave per row ---------------------------------------------------
def test_singleview_wave_scan(torch, gs_chunk):
    from eks_amd import _lib
    gs_chunk(8)
    assert _lib.load().eks_nll_sweep_gaps_chunk_len(2, K7, 2100, 2) == 8
    assert -(-2100 // 8) == 263 > int(os.environ.get("EKS_WAVE_SCAN_CHUNKS", 24))
    both_bounds(torch, "sv2100", 2, 2, "sv B=2 T=2100 chunk=8")


# -- 3: (3,8): whole cameras missing, rank-deficient and zero W_t; runtime n ------------------
def test_multicam_missing_cameras(torch, gs_chunk):
    gs_chunk(8)
    mask = S.case("mc131")["mask"]
    assert mask[1, 20:60, 2:].all() and not mask[1, 20:60, :2].any()  # 2 observations for r = 3
    assert mask[1, 90:100].all()                                      # a 10-frame void
    both_bounds(torch, "mc131", 8, 3, "mc (3,8) B=3 T=131 chunk=8")


def test_runtime_n_five_cameras(torch):
    both_bounds(torch, "mc300", 10, 3, "mc n=10 B=2 T=300")


# -- 4: the pupil model with a blink; candidates that also differ in A --------------------------
def test_pupil_blink(torch, gs_chunk):
    gs_chunk(8)
    c = S.case("pupil131")
    assert c["mask"][0, 40:60].all()
    both_bounds(torch, "pupil131", 8, 3, "pupil B=2 T=131 chunk=8")
    grid = [(.99, .99), (.999, .99), (.9999, .999), (.99, .9999)]
    cands = S.pupil_grid_candidates(S.pupil_complete(), grid)
    assert len({m["A"][0, 0] for ms in cands for m in ms}) == 3
    ref, nobs_ref = S.dense_table(c["g"], cands)
    got, nobs, status, _, d, rows = sweep(torch, c["g"], cands, 8, 3)
    assert not status.any()
    close(got, ref, "pupil (d, c) grid vs dense", RTOL_REF)
    close(got, per_candidate(d, rows, len(grid), 8, 3), "pupil (d, c) grid vs smooth_gaps",
          RTOL_ROUTE)
    np.testing.assert_array_equal(nobs, nobs_ref)


# -- 5: T = 1 and T = 2, trajectory 0 unobserved ----------------------------------------------
@pytest.mark.parametrize("T", [1, 2])
def test_shortest_trajectories(torch, T):
    st = G.members("sv", 3, 131)
    models = [G.model_of("sv", st[b]) for b in range(3)]
    for m in models:
        m["m0"] = np.array([0.75, -1.25])
    mask = np.zeros((3, T, 2), dtype=bool)
    mask[0] = True          # trajectory 0: nothing observed
    mask[1, T - 1, 1] = True
    g = G.knock_out(np.ascontiguousarray(st[:, :, :T]), mask)
    cands = S.scale_candidates(models)
    ref, nobs_ref = S.dense_table(g, cands)
    got, nobs, status, _, d, rows = sweep(torch, g, cands, 2, 2)
    assert not status.any()
    close(got, ref, f"sv T={T} vs dense", RTOL_REF)
    close(got, per_candidate(d, rows, K7, 2, 2), f"sv T={T} vs smooth_gaps", RTOL_ROUTE)
    assert (got[:, 0] == 0.0).all() and nobs[0] == 0
    np.testing.assert_array_equal(nobs, nobs_ref)


# -- 6: the lane mappings ---------------------------------------------------------------------
@pytest.mark.parametrize("K,B", [(8, 32), (2, 480)])
def test_lane_mappings(torch, gs_chunk, K, B):
    """K = 8, B = 32: 256 rows, whole blocks per chunk in the row kernels and
    (chunk, trajectory) pairs in chunk-major order in the reduce kernel;
    K = 2, B = 480: whole blocks per chunk in both, the last block partly idle."""
    T = 24
    gs_chunk(8)
    st = G.members("sv", B, T)
    models = [G.model_of("sv", st[b]) for b in range(B)]
    mask = np.random.default_rng(B).random((B, T, 2)) < 0.3
    mask[::7, 5:19] = True
    g = G.knock_out(st, mask)
    scales = tuple(10.0 ** e for e in range(-3, 5)) if K == 8 else (0.1, 10.0)
    cands = S.scale_candidates(models, scales)
    ref, nobs_ref = S.dense_table(g, cands)
    got, nobs, status, _, d, rows = sweep(torch, g, cands, 2, 2)
    assert rows.shape[0] == K * B and not status.any()
    close(got, ref, f"sv K={K} B={B} T=24 chunk=8 vs dense", RTOL_REF)
    np.testing.assert_array_equal(nobs, nobs_ref)


# -- 7: a trajectory with nothing observed beside normal ones ----------------------------------
def test_nothing_observed_scores_exactly_zero(torch, gs_chunk):
    c = S.case("sv131")
    mask = c["mask"].copy()
    mask[1] = True
    g = G.knock_out(np.array(c["g"]), mask)
    cands = S.scale_candidates(c["models"])
    gs_chunk(8)
    got, nobs, status, _, _, _ = sweep(torch, g, cands, 2, 2, check=True)
    assert not status.any()
    assert (got[:, 1] == 0.0).all() and nobs[1] == 0
    close(got, c["ref"], "sv B=3 T=131, trajectory 1 without observations: the others", RTOL_REF,
          cols=[0, 2])
    assert nobs[0] == c["nobs"][0] and nobs[2] == c["nobs"][2]


# -- 8: complete data: eks_nll_sweep ------------------------------------------------------------
@pytest.mark.parametrize("kind,n,r", [("sv", 2, 2), ("mc", 8, 3)])
def test_complete_data_equals_nll_sweep(torch, gs_chunk, kind, n, r):
    from eks_amd import batch
    st = G.members(kind, 3, 131)
    cands = S.scale_candidates([G.model_of(kind, st[b]) for b in range(3)])
    gs_chunk(8)
    got, nobs, status, _, d, rows = sweep(torch, st, cands, n, r)
    assert not status.any()
    other = batch.nll_sweep(d, rows, K=K7, n=n, r=r).cpu().numpy()
    close(got, other, f"{kind} complete data vs nll_sweep", RTOL_ROUTE)
    assert nobs.tolist() == [131 * n] * 3


# -- 9: the missing rule --------------------------------------------------------------------------
def test_missing_rule_members(torch, gs_chunk):
    c = S.case("sv131")
    g, mask = c["g"], c["mask"]
    cands = S.scale_candidates(c["models"])
    gs_chunk(8)
    base = sweep(torch, g, cands, 2, 2)[3]
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
        res = sweep(torch, v, cands, 2, 2)[3]
        for k in ("nll", "nobs", "status"):
            assert torch.equal(res[k], base[k]), (name, k)
    # float64 members; the mean
    got, nobs, status, *_ = sweep(torch, g, cands, 2, 2, dtype=np.float64)
    assert not status.any()
    close(got, c["ref"], "sv, float64 members vs dense", RTOL_REF)
    ref_mean, nobs_mean = S.dense_table(g, cands, "mean")
    got, nobs, status, *_ = sweep(torch, g, cands, 2, 2, mode="mean")
    assert not status.any()
    close(got, ref_mean, "sv, mean vs dense", RTOL_REF)
    np.testing.assert_array_equal(nobs, nobs_mean)


def test_missing_rule_yev_handoff_is_bit_identical(torch, gs_chunk):
    from eks_amd import batch, core
    c = S.case("sv131")
    gs_chunk(8)
    yev, preds, ev = core.ensemble_handoff(np.array(c["g"][0]))
    assert np.isnan(preds).any() and np.isnan(ev).any()
    cands = [[ms[0]] for ms in S.scale_candidates(c["models"])]
    rows = torch.from_numpy(S.rows_of(cands)).cuda()
    a = batch.nll_sweep_gaps(yev, rows, K=K7, n=2, r=2)
    d = batch.make_time_major(c["g"][:1], dtype=np.float64)
    b = batch.nll_sweep_gaps(d, rows, K=K7, n=2, r=2)
    for k in ("nll", "nobs", "status"):
        assert torch.equal(a[k], b[k]), k
    close(a["nll"].cpu().numpy(), c["ref"][:, :1], "sv Yev vs dense", RTOL_REF)


# -- 10: status ---------------------------------------------------------------------------------------
def test_exact_observation_is_flagged(torch, gs_chunk):
    from eks_amd import _lib
    c = S.case("sv131")
    assert not c["mask"][1, 60].any()
    cands = S.scale_candidates(c["models"])
    ex = np.array(c["g"])
    ex[1, :, 60, 0] = ex[1, 0, 60, 0]  # trajectory 1, frame 60, x: all members equal
    gs_chunk(8)
    got, nobs, status, *_ = sweep(torch, ex, cands, 2, 2)
    assert (status == np.array([0, _lib.EKS_STATUS_SCAN, 0])[None, :]).all(), status
    assert np.isnan(got[:, 1]).all()
    close(got, c["ref"], "sv exact observation: the other trajectories", RTOL_REF, cols=[0, 2])
    with pytest.raises(ValueError, match="zero ensemble variance"):
        sweep(torch, ex, cands, 2, 2, check=True)
    ex[1, 0, 60, 0] = np.nan  # the same column marked missing
    got, nobs, status, *_ = sweep(torch, ex, cands, 2, 2, check=True)
    assert not status.any()
    ref, nobs_ref = S.dense_table(ex, cands)
    close(got, ref, "sv exact observation marked missing", RTOL_REF)
    np.testing.assert_array_equal(nobs, nobs_ref)


@pytest.mark.parametrize("chunk", [8, 136])
def test_changed_offset_is_a_bad_model_on_that_row_only(torch, gs_chunk, chunk):
    from eks_amd import _lib, batch
    c = S.case("sv131")
    cands = S.scale_candidates(c["models"])
    cands[4][1] = dict(cands[4][1], means=cands[4][1]["means"] + np.array([0.0, 1e-9]))
    gs_chunk(chunk)
    got, nobs, status, _, d, rows = sweep(torch, c["g"], cands, 2, 2)
    want = np.zeros((K7, 3), dtype=np.int32)
    want[4, 1] = _lib.EKS_STATUS_BAD_MODEL
    np.testing.assert_array_equal(status, want)
    keep = np.ones((K7, 3), dtype=bool)
    keep[4, 1] = False
    rel = float((np.abs(got - c["ref"])[keep] / np.abs(c["ref"][keep])).max())
    print(f"[gaps sweep] bad model chunk={chunk}: the other rows, max rel err {rel:.3e}")
    assert rel <= RTOL_REF
    with pytest.raises(ValueError, match="share C and offset"):
        batch.nll_sweep_gaps(d, rows, K=K7, n=2, r=2)


# -- 11: reproducible; the operator ------------------------------------------------------------------
@pytest.mark.parametrize("name,chunk", [("sv131", 8), ("sv2100", 8), ("sv131", 136)])
def test_two_calls_bit_identical_and_operator(torch, gs_chunk, name, chunk):
    import eks_amd.ops  # noqa: F401
    c = S.case(name)
    cands = S.scale_candidates(c["models"])
    gs_chunk(chunk)
    a = sweep(torch, c["g"], cands, 2, 2)
    b = sweep(torch, c["g"], cands, 2, 2)
    for k in ("nll", "nobs", "status"):
        assert torch.equal(a[3][k], b[3][k]), k
    assert torch.isfinite(a[3]["nll"]).all() and not a[2].any()
    nll, nobs, status = torch.ops.eks.nll_sweep_gaps(a[4], a[5], K7, 2, 2, "median")
    assert torch.equal(nll, a[3]["nll"]) and torch.equal(nobs, a[3]["nobs"])
    assert torch.equal(status, a[3]["status"])
    assert nobs.cpu().tolist() == c["nobs"].tolist()


# -- 12: selection -------------------------------------------------------------------------------------
def base_params(torch, models):
    return torch.from_numpy(S.rows_of([models])).cuda()


@pytest.mark.parametrize("name,n,r", [("sv131", 2, 2), ("mc131", 8, 3), ("pupil131", 8, 3),
                                      ("sv2100", 2, 2)])
def test_refine_zero_returns_the_references_argmin(torch, name, n, r):
    from eks_amd import batch
    c = S.case(name)
    d = batch.make_time_major(c["g"], dtype=np.float32)
    res = batch.select_smooth_param(d, base_params(torch, c["models"]), n=n, r=r, grid=S.SCALES,
                                    refine=0, allow_missing=True)
    want = np.array(S.SCALES)[np.argmin(c["ref"], axis=0)]
    print(f"[gaps sweep] {name}: reference argmin {want}, chosen "
          f"{res['smooth_param'].cpu().numpy()}")
    np.testing.assert_array_equal(res["smooth_param"].cpu().numpy(), want)
    close(res["nll"].cpu().numpy()[None], np.min(c["ref"], axis=0)[None],
          f"{name} NLL at the argmin", RTOL_REF)
    assert not bool(res["at_edge"].any())
    np.testing.assert_array_equal(res["nobs"].cpu().numpy(), c["nobs"])


@pytest.mark.parametrize("name,n,r", [("sv131", 2, 2), ("mc131", 8, 3)])
def test_refinement_never_raises_the_nll(torch, gs_chunk, name, n, r):
    from eks_amd import batch
    gs_chunk(8)
    c = S.case(name)
    d = batch.make_time_major(c["g"], dtype=np.float32)
    base = base_params(torch, c["models"])
    kw = dict(n=n, r=r, grid=S.SCALES, allow_missing=True)
    coarse = batch.select_smooth_param(d, base, refine=0, **kw)
    fine = batch.select_smooth_param(d, base, refine=2, **kw)
    s = fine["smooth_param"]
    print(f"[gaps sweep] {name}: coarse {coarse['smooth_param'].cpu().numpy()} nll "
          f"{coarse['nll'].cpu().numpy()}, refined {s.cpu().numpy()} nll "
          f"{fine['nll'].cpu().numpy()}")
    again = batch.nll_sweep_gaps(d, fine["params"], K=1, n=n, r=r)["nll"][0]
    assert torch.equal(again, fine["nll"])
    assert bool((fine["nll"] <= coarse["nll"]).all())
    want = base.clone()
    q0 = r + 2 * r * r
    want[:, q0:q0 + r * r] *= s.unsqueeze(1)
    assert torch.equal(fine["params"], want)


def test_default_selection_is_todays_route(torch):
    """allow_missing=False on complete data: the choice and its NLL are
    nll_sweep's, bit for bit."""
    from eks_amd import batch
    st = G.members("sv", 3, 131)
    models = [G.model_of("sv", st[b]) for b in range(3)]
    d = batch.make_time_major(st, dtype=np.float32)
    base = base_params(torch, models)
    res = batch.select_smooth_param(d, base, n=2, r=2, grid=S.SCALES, refine=0)
    assert "nobs" not in res
    rows = torch.from_numpy(S.rows_of(S.scale_candidates(models))).cuda()
    scores = batch.nll_sweep(d, rows, K=K7, n=2, r=2)
    idx = torch.argmin(scores, dim=0)
    assert torch.equal(res["nll"], scores.gather(0, idx[None])[0])
    assert torch.equal(res["smooth_param"],
                       torch.tensor(S.SCALES, dtype=torch.float64, device="cuda")[idx])


# -- 13: the pupil wrappers ----------------------------------------------------------------------------
KPS = ['pupil_top_r', 'pupil_right_r', 'pupil_bottom_r', 'pupil_left_r']


def _pupil_frames(st):
    from eks_amd import fit
    return [pd.DataFrame(st[e], columns=list(fit.PUPIL_KEYS)) for e in range(st.shape[0])]


def _pupil_ref(st, A):
    """gaps_ref.dense on the oracle's pupil model of the complete frames, in
    the markers_df column order."""
    from eks_amd import fit
    from oracle import eks_oracle as O
    y, ev = G.ensemble(st)
    ok = np.isfinite(y).all(axis=1) & np.isfinite(ev).all(axis=1)
    p = O.pupil_params(y[ok], np.asarray(A))
    ref = G.dense(y, ev, {k: p[k] for k in S.KEYS})
    order = [fit.PUPIL_KEYS.index(f"{kp}_{c}") for kp in KPS for c in "xy"]
    return ref, order, y, ev, ok


def test_pupil_wrapper(torch):
    from eks_amd import synthetic
    from eks_amd.pupil_smoother import ensemble_kalman_smoother_pupil
    T = 200
    st = synthetic.pupil_obs(np.random.default_rng(5), 5, T).astype(np.float64)
    A = np.diag([.9999, .999, .999])
    a = ensemble_kalman_smoother_pupil(_pupil_frames(st), KPS, "tracker", A, posterior_var=True)
    b = ensemble_kalman_smoother_pupil(_pupil_frames(st), KPS, "tracker", A, posterior_var=True,
                                       allow_missing=True)
    assert set(b) == set(a) | {"n_missing"} and b["n_missing"] == 0
    xy = np.arange(12) % 3 != 2
    d = float(np.abs(a["markers_df"].to_numpy()[:, xy] - b["markers_df"].to_numpy()[:, xy]).max())
    print(f"[gaps sweep] pupil wrapper, gap-free: {d:.3e} px")
    assert np.isfinite(a["markers_df"].to_numpy()[:, xy]).all() and d <= OUT_TOL
    gap = st.copy()
    gap[:, 80:110, :] = np.nan  # a blink: every keypoint NaN over 30 frames, every member
    gap[2, 150, 1] = np.nan     # and one member's single NaN
    res = ensemble_kalman_smoother_pupil(_pupil_frames(gap), KPS, "tracker", A,
                                         posterior_var=True, allow_missing=True)
    assert res["n_missing"] == 30 * 8 + 1
    ref, order, *_ = _pupil_ref(gap, A)
    got = res["markers_df"].to_numpy()
    var = res["posterior_var_df"].to_numpy()
    lat = res["latents_df"].to_numpy()
    lvar = res["latents_posterior_var_df"].to_numpy()
    assert np.isfinite(ref["out"]).all() and np.isfinite(ref["var"]).all()
    for arr in (got[:, xy], var[:, xy], lat, lvar):
        assert np.isfinite(arr).all()
    assert np.isnan(got[:, ~xy]).all()
    d_out = float(np.abs(got[:, xy] - ref["out"][:, order]).max())
    d_var = float((np.abs(var[:, xy] - ref["var"][:, order]) / ref["var"][:, order]).max())
    d_lvar = float((np.abs(lvar - np.einsum("tii->ti", ref["Vs"]))
                    / np.einsum("tii->ti", ref["Vs"])).max())
    print(f"[gaps sweep] pupil wrapper with a 30-frame blink: out {d_out:.3e} px, "
          f"var rel {d_var:.3e}, latent var rel {d_lvar:.3e}")
    assert d_out <= OUT_TOL and d_var <= VAR_RTOL and d_lvar <= VAR_RTOL


def test_pupil_smoothing_sweep_through_a_blink(torch):
    from eks_amd import synthetic
    from eks_amd.pupil_smoother import ensemble_kalman_smoother_pupil, pupil_smoothing_sweep
    from oracle import eks_oracle as O
    T = 200
    gap = synthetic.pupil_obs(np.random.default_rng(5), 5, T).astype(np.float64)
    gap[:, 80:110, :] = np.nan
    gap[2, 150, 1] = np.nan
    ds, cs = [0.99, 0.9999], [0.99, 0.999]
    res = pupil_smoothing_sweep(_pupil_frames(gap), KPS, "tracker", ds, cs, allow_missing=True)
    _, _, y, ev, ok = _pupil_ref(gap, np.eye(3))
    ref = np.array([[G.dense(y, ev, {k: O.pupil_params(y[ok], np.diag([d, c, c]))[k]
                                     for k in S.KEYS})["nll"] for c in cs] for d in ds])
    assert res["nll"].shape == (2, 2)
    close(res["nll"], ref, "pupil_smoothing_sweep(allow_missing=True) vs dense", RTOL_REF)
    i, j = np.unravel_index(np.argmin(ref), ref.shape)
    assert res["best"] == (ds[i], cs[j])
    one = ensemble_kalman_smoother_pupil(_pupil_frames(gap), KPS, "tracker",
                                         np.diag([ds[i], cs[j], cs[j]]), allow_missing=True)
    pd.testing.assert_frame_equal(res["markers_df"], one["markers_df"], check_exact=True)
    pd.testing.assert_frame_equal(res["latents_df"], one["latents_df"], check_exact=True)
    assert res["n_missing"] == one["n_missing"] == 30 * 8 + 1
    assert np.isfinite(res["latents_df"].to_numpy()).all()
