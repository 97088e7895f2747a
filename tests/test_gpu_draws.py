"""Joint posterior trajectory draws on the device (eks_draws_gaps,
eks_draws_noise, batch.draws_gaps / draws_noise, torch.ops.eks.draws_gaps,
posterior_draws in the wrappers) against tests/draws_ref.py.

The sampler is pinned exactly, without statistics: fed the T r one-hot noise
vectors, the responses M = latent - ms satisfy M M^T = Sigma, the dense joint
posterior covariance of draws_ref.joint, every block of it -- the marginals
Vs_t on the diagonal and the cross-covariances between any two frames off it.

Members come from eks_amd.synthetic as float32 unless stated; the models are
the oracle's on the complete data.  Every case prints its measured maxima
before asserting.

Tolerances (the project's own, test_gpu_gaps.py): draws, latent and out 1e-8
px; M M^T norm-wise rtol 1e-8 relative to max |Sigma| (the Vs tolerance).
The generator: the 53-bit integers behind the uniforms exact; the normals
1e-12 absolute against the numpy model, about 100 x the few-ulp difference of
log / cos / sin at |z| <= 8.6.
Measured on an MI355X: M M^T 6.6e-16 / 7.5e-16 (T = 24) and 3.5e-15 (T = 211);
out vs the joint mean 5.7e-14 px; random noise 1.2e-13 px; zero noise, the
input forms and seeded vs draws_noise's tensor 0 (the same bits); draws_noise
vs the numpy model 4.4e-16 with the integers exact.
"""
import functools
import os

import numpy as np
import pandas as pd
import pytest

import draws_ref as D
import gaps_ref as G

pytestmark = pytest.mark.gpu

OUT_TOL, RTOL, Z_TOL = 1e-8, 1e-8, 1e-12


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


def noise_tensor(torch, z):
    """(B, S, T, r) numpy noise as the (B, S, T, r) view of a (T, B, S, r) buffer."""
    tm = np.ascontiguousarray(np.transpose(np.asarray(z, dtype=np.float64), (2, 0, 1, 3)))
    return torch.from_numpy(tm).to("cuda").permute(1, 2, 0, 3)


def run(torch, st, models, n, r, z=None, dtype=np.float32, **kw):
    from eks_amd import batch
    d = batch.make_time_major(st, dtype=dtype)
    if z is not None:
        kw["noise"] = noise_tensor(torch, z)
    res = batch.draws_gaps(d, pack(models), n=n, r=r, want_latent=True, **kw)
    torch.cuda.synchronize()
    return res


def smooth(torch, st, models, n, r, dtype=np.float32):
    from eks_amd import batch
    d = batch.make_time_major(st, dtype=dtype)
    res = batch.smooth_gaps(d, pack(models), n=n, r=r, want_ms=True)
    torch.cuda.synchronize()
    return res


def covariance_identity(torch, kind, T, what):
    """One-hot noise through the device sampler against draws_ref.joint."""
    g, model, y, ev, mask = D.case(kind, T, True)
    n, r = y.shape[1], model["m0"].shape[0]
    assert mask[0, 9:14].all() and mask[0, 0].all() and mask[0, -1].all()
    Sigma, mean = D.joint(y, ev, model)
    assert np.isfinite(Sigma).all() and np.isfinite(mean).all()
    res = run(torch, g, [model], n, r, z=D.one_hot(T, r)[None])
    assert res["status"].cpu().tolist() == [0]
    ms = smooth(torch, g, [model], n, r)["ms"][0].cpu().numpy()
    latent = res["latent"][0].cpu().numpy()
    assert latent.shape == (T * r, T, r) and np.isfinite(latent).all()
    M = D.responses(latent, ms)
    err = float(np.abs(M @ M.T - Sigma).max() / np.abs(Sigma).max())
    e_out = float(np.abs(res["out"][0].cpu().numpy()
                         - (mean @ model["C"].T + model["means"])).max())
    # the projected draws are the latent draws through C
    e_proj = float(np.abs(res["draws"][0].cpu().numpy()
                          - (latent @ model["C"].T + model["means"])).max())
    print(f"[draws] {what}: M M^T vs Sigma {err:.3e} (cond {np.linalg.cond(Sigma):.2e}), "
          f"out vs joint mean {e_out:.3e} px, draws vs C latent {e_proj:.3e} px")
    assert err <= RTOL, (what, err)
    assert e_out <= OUT_TOL and e_proj <= OUT_TOL, (what, e_out, e_proj)


# -- 1: the exact covariance, three chunks, the serial scans ---------------------------------
@pytest.mark.parametrize("kind", ["sv", "mc"])
def test_exact_covariance_serial_scans(torch, gaps_chunk, kind):
    from eks_amd import _lib
    gaps_chunk(8)
    assert _lib.load().eks_draws_gaps_chunk_len(1, 24, 2 if kind == "sv" else 3) == 8
    covariance_identity(torch, kind, 24, f"{kind} T=24 chunk=8")


# -- 2: 27 chunks (the wave scans), the last one of 3 frames ------------------------------------
def test_exact_covariance_wave_scans_ragged_chunk(torch, gaps_chunk):
    from eks_amd import _lib
    gaps_chunk(8)
    assert _lib.load().eks_draws_gaps_chunk_len(1, 211, 2) == 8
    assert -(-211 // 8) == 27 > int(os.environ.get("EKS_WAVE_SCAN_CHUNKS", 24)) and 211 % 8 == 3
    covariance_identity(torch, "sv", 211, "sv T=211 chunk=8 (wave scans)")


# -- 3: random noise against the sequential reference ----------------------------------------
@functools.lru_cache(maxsize=None)
def sv131_reference():
    """case_sv131 with S = 5 random draws: (z (3, 5, 131, 2), [draws_ref.draws])."""
    g, models, _, _ = G.case_sv131()
    z = np.random.default_rng(5131).standard_normal((3, 5, 131, 2))
    z.setflags(write=False)
    refs = []
    for b in range(3):
        y, ev = G.ensemble(g[b])
        refs.append(D.draws(y, ev, models[b], z[b]))
    return z, refs


def compare(res, refs, what, rows=None, draws=slice(None)):
    rows = range(len(refs)) if rows is None else rows
    worst = dict(draws=0.0, latent=0.0)
    for b in rows:
        for k in ("draws", "latent"):
            ref = refs[b][k][draws]
            got = res[k][b].cpu().numpy()
            assert np.isfinite(ref).all(), (what, b, k, "reference not finite")
            assert got.shape == ref.shape and np.isfinite(got).all(), (what, b, k)
            worst[k] = max(worst[k], float(np.abs(got - ref).max()))
    print(f"[draws] {what}: draws {worst['draws']:.3e} px, latent {worst['latent']:.3e}")
    assert worst["draws"] <= OUT_TOL and worst["latent"] <= OUT_TOL, (what, worst)


@pytest.mark.parametrize("chunk", [8, 0, 136])
def test_parity_random_noise(torch, gaps_chunk, chunk):
    g, models, _, mask = G.case_sv131()
    z, refs = sv131_reference()
    assert mask[0, 45:85].all()
    gaps_chunk(chunk)
    res = run(torch, g, models, 2, 2, z=z)  # S = 5: a tile of 4 and a remainder of 1
    assert res["draws"].shape == (3, 5, 131, 2) and res["latent"].shape == (3, 5, 131, 2)
    assert int(res["status"].abs().sum()) == 0
    compare(res, refs, f"sv131 S=5 chunk={chunk}")
    one = run(torch, g, models, 2, 2, z=z[:, :1])
    compare(one, refs, f"sv131 S=1 chunk={chunk}", draws=slice(0, 1))


# -- 4: zero noise is the smoothed mean -------------------------------------------------------
def test_zero_noise_is_out(torch, gaps_chunk):
    g, models, _, _ = G.case_sv131()
    gaps_chunk(8)
    res = run(torch, g, models, 2, 2, z=np.zeros((3, 3, 131, 2)), want_var=True)
    sm = smooth(torch, g, models, 2, 2)
    d0 = float((res["draws"] - res["out"][:, None]).abs().max())
    d1 = float((res["out"] - sm["out"]).abs().max())
    bits0 = bool(torch.equal(res["draws"], res["out"][:, None].expand_as(res["draws"])))
    bits1 = bool(torch.equal(res["out"], sm["out"]))
    print(f"[draws] zero noise: draws vs out {d0:.3e} px (same bits: {bits0}), out vs "
          f"smooth_gaps {d1:.3e} px (same bits: {bits1})")
    assert torch.isfinite(res["draws"]).all() and d0 <= OUT_TOL and d1 <= OUT_TOL
    from eks_amd import batch
    var = batch.smooth_gaps(batch.make_time_major(g, dtype=np.float32), pack(models), n=2, r=2,
                            want_var=True)["var"]
    assert float((res["var"] - var).abs().max()) <= 1e-12


# -- 5: input forms; a draw does not depend on the others; reproducible -------------------------
def test_input_forms_and_independence(torch, gaps_chunk):
    from eks_amd import batch
    g, models, _, _ = G.case_sv131()
    z, refs = sv131_reference()
    gaps_chunk(8)
    a = run(torch, g, models, 2, 2, z=z, dtype=np.float32)
    b = run(torch, g, models, 2, 2, z=z, dtype=np.float64)
    yev = batch.ensemble_gaps(batch.make_time_major(g, dtype=np.float64), n=2, min_members=5)["yev"]
    c = batch.draws_gaps(yev, pack(models), n=2, r=2, noise=noise_tensor(torch, z),
                         want_latent=True)
    d_ab = float((a["draws"] - b["draws"]).abs().max())
    d_ac = float((a["draws"] - c["draws"]).abs().max())
    print(f"[draws] float32 vs float64 members {d_ab:.3e} px, members vs Yev planes {d_ac:.3e} px")
    assert d_ab <= OUT_TOL and d_ac <= OUT_TOL
    compare(c, refs, "sv131 Yev planes")
    for s in (0, 3, 4):  # tile slots 0 and 3, and the remainder tile
        one = run(torch, g, models, 2, 2, z=z[:, s:s + 1])
        assert torch.equal(one["draws"][:, 0], a["draws"][:, s]), s
        assert torch.equal(one["latent"][:, 0], a["latent"][:, s]), s
    again = run(torch, g, models, 2, 2, z=z, dtype=np.float32)
    for k in ("draws", "latent", "out", "status"):
        assert torch.equal(a[k], again[k]), k


# -- 6: seeded noise ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,r", [("sv", 2, 2), ("mc", 8, 3)])
def test_seeded_equals_explicit_noise(torch, gaps_chunk, kind, n, r):
    from eks_amd import batch
    B, T, S, seed = 2, 131, 5, 2026
    st = G.members(kind, B, T)
    models = [G.model_of(kind, st[b]) for b in range(B)]
    g = G.knock_out(st, np.random.default_rng(T + n).random((B, T, n)) < 0.2)
    gaps_chunk(8)
    d = batch.make_time_major(g, dtype=np.float32)
    a = batch.draws_gaps(d, pack(models), n=n, r=r, S=S, seed=seed, want_latent=True)
    zs = batch.draws_noise(B, S, T, r, seed)
    b = batch.draws_gaps(d, pack(models), n=n, r=r, noise=zs, want_latent=True)
    diff = float((a["draws"] - b["draws"]).abs().max())
    bits = bool(torch.equal(a["draws"], b["draws"]) and torch.equal(a["latent"], b["latent"]))
    print(f"[draws] {kind} seeded vs draws_noise: {diff:.3e} px (same bits: {bits})")
    assert torch.isfinite(a["draws"]).all() and int(a["status"].abs().sum()) == 0
    assert diff <= OUT_TOL
    other = batch.draws_gaps(d, pack(models), n=n, r=r, S=S, seed=seed + 1)
    assert float((other["draws"] - a["draws"]).abs().max()) > 1e-3
    # against the sequential reference on the numpy model's noise
    zm = D.normals(seed, B, S, T, r)
    refs = [D.draws(*G.ensemble(g[k]), models[k], zm[k]) for k in range(B)]
    compare(a, refs, f"{kind} seeded vs the reference on the model's noise")


@pytest.mark.parametrize("r", [2, 3])
def test_draws_noise_is_the_numpy_model(torch, r):
    from eks_amd import _lib, batch
    B, S, T, seed = 3, 5, 300, 20261021
    z = batch.draws_noise(B, S, T, r, seed)
    assert z.shape == (B, S, T, r) and z.stride(3) == 1
    prev = _lib.debug_set(_lib.EKS_DBG_DRAWS_RAW, 1)
    try:
        k = batch.draws_noise(B, S, T, r, seed).cpu().numpy()
    finally:
        _lib.debug_set(_lib.EKS_DBG_DRAWS_RAW, prev)
    assert np.array_equal(k, D.raw(seed, B, S, T, r).astype(np.float64)), "uniform bits differ"
    err = float(np.abs(z.cpu().numpy() - D.normals(seed, B, S, T, r)).max())
    print(f"[draws] draws_noise r={r} vs the numpy model: {err:.3e} (integer bits exact)")
    assert err <= Z_TOL
    sub = batch.draws_noise(2, 3, 50, r, seed)
    assert torch.equal(sub, z[:2, :3, :50])
    big_seed = batch.draws_noise(1, 1, 4, r, 2 ** 63 + 12345).cpu().numpy()
    assert np.abs(big_seed - D.normals(2 ** 63 + 12345, 1, 1, 4, r)).max() <= Z_TOL
    import eks_amd.ops  # noqa: F401
    assert torch.equal(torch.ops.eks.draws_noise(z, B, S, T, r, seed), z.contiguous())


# -- 7: status -----------------------------------------------------------------------------------
def test_status_bits(torch, gaps_chunk):
    from eks_amd import _lib, batch
    g, models, _, mask = G.case_sv131()
    z, refs = sv131_reference()
    gaps_chunk(8)
    bad = dict(models[1], A=np.eye(2), S0=np.eye(2), Q=-0.5 * np.eye(2))
    blind = np.array(g)
    blind[1] = np.nan  # nothing observed: D_0 = P_0 - J_0 S_0 J_0^T = I - 2 (0.5 I) 2 = -I
    res = run(torch, blind, [models[0], bad, models[2]], 2, 2, z=z)
    st = res["status"].cpu().tolist()
    print(f"[draws] status with an indefinite model on trajectory 1: {st}")
    assert st[0] == 0 and st[2] == 0 and st[1] & _lib.EKS_STATUS_SINGULAR
    assert torch.isnan(res["draws"][1]).all() and torch.isnan(res["latent"][1]).all()
    compare(res, refs, "indefinite model: the other trajectories", rows=[0, 2])
    with pytest.raises(np.linalg.LinAlgError):
        run(torch, blind, [models[0], bad, models[2]], 2, 2, z=z, check=True)
    # an exact observation: an observed column with ev == 0
    assert not mask[1, 60].any()
    ex = np.array(g)
    ex[1, :, 60, 0] = ex[1, 0, 60, 0]
    res = run(torch, ex, models, 2, 2, z=z)
    st = res["status"].cpu().tolist()
    print(f"[draws] status with an exact observation on trajectory 1: {st}")
    # (its P_t are NaN, and a NaN pivot is not > 0: EKS_STATUS_SINGULAR may be set as well)
    assert st[0] == 0 and st[2] == 0 and st[1] & _lib.EKS_STATUS_SCAN
    assert st[1] & ~(_lib.EKS_STATUS_SCAN | _lib.EKS_STATUS_SINGULAR) == 0
    assert torch.isnan(res["draws"][1]).all()
    compare(res, refs, "exact observation: the other trajectories", rows=[0, 2])
    # S = 0: the draws buffer is not touched
    lib = _lib.load()
    d = batch.make_time_major(g, dtype=np.float32)
    params = pack(models)
    poison = torch.full((3 * 131 * 2 * 4,), -7.25, dtype=torch.float64, device="cuda")
    status = torch.full((3,), 99, dtype=torch.int32, device="cuda")
    ws = batch.workspace(lib.eks_draws_gaps_workspace_bytes(3, 0, 131, 2, 2), "cuda", slot="t")
    sb, stt, se, sj = d.stride()
    _lib.check(lib.eks_draws_gaps(d.data_ptr(), _lib.EKS_F32, 3, 131, 5, 2, 2, sb, stt, se, sj,
                                  _lib.EKS_MEDIAN, params.data_ptr(), 0, None, 0, 0, 0, 1,
                                  poison.data_ptr(), 0, 0, 0, 0, None, None, 0, 0, 0, None,
                                  ws.data_ptr(), ws.numel(), status.data_ptr(),
                                  _lib.stream_ptr()), "eks_draws_gaps")
    torch.cuda.synchronize()
    assert bool((poison == -7.25).all()) and status.cpu().tolist() == [0, 0, 0]
    empty = batch.draws_gaps(d, params, n=2, r=2, S=0, seed=1)
    assert empty["draws"].shape == (3, 0, 131, 2)


# -- 8: the wrappers -----------------------------------------------------------------------------
def test_wrapper_single_view(torch):
    from eks_amd import batch, core, fit
    from eks_amd.singleview_smoother import ensemble_kalman_smoother_single_view as sv
    st = np.array(G.members("sv", 1, 200)[0])  # (E, T, 2)
    st[:, 80:110, :] = np.nan
    st[2, 150, 1] = np.nan
    dfs = [pd.DataFrame(st[e], columns=["nose_x", "nose_y"]) for e in range(5)]
    kw = dict(posterior_var=True, allow_missing=True)
    a = sv(dfs, "nose", 10.0, 50.0, **kw)
    b = sv(dfs, "nose", 10.0, 50.0, posterior_draws=3, draws_seed=11, **kw)
    assert set(b) == set(a) | {"posterior_draws"}
    for k in ("markers_df", "posterior_var_df"):
        pd.testing.assert_frame_equal(a[k], b[k], check_exact=True)
    assert a["nll"] == b["nll"] and a["n_missing"] == b["n_missing"] == 61
    dr = b["posterior_draws"]
    assert dr.shape == (3, 200, 2) and dr.dtype == np.float64 and np.isfinite(dr).all()
    yev, preds, ev = core.ensemble_handoff(st, "median")
    ok = np.isfinite(preds).all(axis=1) & np.isfinite(ev).all(axis=1)
    m = fit.singleview_model(preds[ok], ev[ok], 10.0, 50.0)
    params = batch.pack_params(m["m0"], m["S0"], m["A"], m["Q"], m["C"], m["offset"])
    ref = batch.draws_gaps(yev, params, n=2, r=2, S=3, seed=11)["draws"][0].cpu().numpy()
    assert np.array_equal(dr, ref)
    # the draws spread where nothing is observed, by about the posterior sd
    sd = np.sqrt(b["posterior_var_df"].to_numpy()[:, :2])
    dev = np.abs(dr - b["markers_df"].to_numpy()[None, :, :2]) / sd[None]
    print(f"[draws] single-view wrapper: largest |draw - mean| / sd {dev.max():.2f}")
    assert 0.5 < dev.max() < 6.0


def test_wrapper_multi_cam(torch):
    from eks_amd import batch, core, fit
    from eks_amd.multiview_pca_smoother import ensemble_kalman_smoother_multi_cam as mc
    V, T = 4, 200
    cams = [f"cam{c}" for c in range(V)]
    st = G.members("mc", 1, T)[0]  # (E, T, 8)
    frames = [[pd.DataFrame(st[e][:, 2 * c:2 * c + 2], columns=["x", "y"]) for e in range(5)]
              for c in range(V)]
    a = mc(frames, "paw", 10.0, 25.0, cams)
    b = mc(frames, "paw", 10.0, 25.0, cams, posterior_draws=3)
    assert set(b) == set(a) | {"posterior_draws"}
    for c in cams:
        pd.testing.assert_frame_equal(a[c + "_df"], b[c + "_df"], check_exact=True)
    dr = b["posterior_draws"]
    assert dr.shape == (3, T, 8) and np.isfinite(dr).all()
    yev, preds, ev = core.ensemble_handoff(np.asarray(st))
    m = fit.multicam_model(preds, ev, 10.0, 25.0)
    params = batch.pack_params(m["m0"], m["S0"], m["A"], m["Q"], m["C"], m["offset"])
    ref = batch.draws_gaps(yev, params, n=8, r=3, S=3, seed=0)["draws"][0].cpu().numpy()
    assert np.array_equal(dr, ref)


@pytest.mark.parametrize("fit_on_device", [False, True])
def test_wrapper_pupil(torch, fit_on_device):
    from eks_amd import fit, synthetic
    from eks_amd.pupil_smoother import ensemble_kalman_smoother_pupil as pupil
    T = 300
    st = synthetic.pupil_obs(np.random.default_rng(300), 5, T).astype(np.float32).astype(np.float64)
    st[:, 100:120] = np.nan  # a blink
    frames = [pd.DataFrame(st[e], columns=list(fit.PUPIL_KEYS)) for e in range(5)]
    kps = ['pupil_top_r', 'pupil_right_r', 'pupil_bottom_r', 'pupil_left_r']
    A = np.diag([.9999, .999, .999])
    kw = dict(allow_missing=True, fit_on_device=fit_on_device)
    a = pupil(frames, kps, "tracker", A, **kw)
    b = pupil(frames, kps, "tracker", A, posterior_draws=3, draws_seed=5, **kw)
    assert set(b) == set(a) | {"posterior_draws", "latents_posterior_draws"}
    for k in ("markers_df", "latents_df"):
        pd.testing.assert_frame_equal(a[k], b[k], check_exact=True)
    dr, lat = b["posterior_draws"], b["latents_posterior_draws"]
    assert dr.shape == (3, T, 8) and lat.shape == (3, T, 3)
    assert np.isfinite(dr).all() and np.isfinite(lat).all()
    # the latent draws are in latents_df's columns: they scatter around it
    gap = np.abs(lat - b["latents_df"].to_numpy()[None]).max()
    scale = np.abs(b["latents_df"].to_numpy()).max()
    print(f"[draws] pupil wrapper fit_on_device={fit_on_device}: largest |latent draw - mean| "
          f"{gap:.3e} (latents up to {scale:.3e})")
    assert 0 < gap < scale


# -- 9: the operator -----------------------------------------------------------------------------
def test_operator_equals_batch(torch, gaps_chunk):
    from eks_amd import batch
    import eks_amd.ops  # noqa: F401
    g, models, _, _ = G.case_sv131()
    z, _ = sv131_reference()
    gaps_chunk(8)
    a = run(torch, g, models, 2, 2, z=z)
    d = batch.make_time_major(g, dtype=np.float32)
    draws, latent, out, status = torch.ops.eks.draws_gaps(d, pack(models), noise_tensor(torch, z),
                                                          2, 2, "median")
    assert torch.equal(draws, a["draws"].contiguous()) and torch.equal(latent, a["latent"])
    assert torch.equal(out, a["out"].contiguous()) and torch.equal(status, a["status"])
