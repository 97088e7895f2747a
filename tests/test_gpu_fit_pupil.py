"""The pupil model fitted on the device (eks_fit_pupil, batch.fit_pupil /
pupil_params / pupil_sweep, torch.ops.eks.fit_pupil and the wrappers'
``fit_on_device``) against the host fit: fit.pupil_model(preds[ok], A) on
the oracle's ensemble, ok the frames that are finite in every column.

Data is synthetic.pupil_obs (float32 values; the float64 members hold the
same values).  Bounds: the six statistics rtol 1e-10 (the project's NLL
tolerance; a numpy model of the shifted sums + Chan merges agrees with
fit.pupil_model to 2e-15, so a miss is a bug, not noise), NLL rtol 1e-10,
out / ms 1e-8 px, posterior variances rtol 1e-8.
"""
import functools
import os
import warnings

import numpy as np
import pandas as pd
import pytest

import ensemble_gaps_ref as R

pytestmark = pytest.mark.gpu

STAT_RTOL, NLL_RTOL, OUT_TOL, VAR_RTOL = 1e-10, 1e-10, 1e-8, 1e-8
KPS = ['pupil_top_r', 'pupil_right_r', 'pupil_bottom_r', 'pupil_left_r']


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@functools.lru_cache(maxsize=None)
def members(B, T, E, seed=0):
    """(B, E, T, 8) float64 members holding float32 values; shared, read only."""
    from eks_amd import synthetic
    rng = np.random.default_rng(1000 * seed + 7 * B + T + E)
    st = np.stack([synthetic.pupil_obs(rng, E, T) for _ in range(B)]).astype(np.float64)
    st.setflags(write=False)
    return st


def host_fit(st, mode="median", A=None, planes=None):
    """fit.pupil_model on the complete frames of one trajectory's members
    (E, T, 8) -- or of given (y, ev) planes -- -> (stats (6,), count, model,
    (preds, ev))."""
    from eks_amd import fit
    from oracle import eks_oracle as O
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        preds, ev = O.ensemble_array(st, mode) if planes is None else planes
        ok = np.isfinite(preds).all(axis=1) & np.isfinite(ev).all(axis=1)
        if not ok.any():
            return np.full(6, np.nan), 0, None, (preds, ev)
        m = fit.pupil_model(preds[ok], np.eye(3) if A is None else A)
    stats = np.array([m["m0"][0], m["mx"], m["my"], *np.diag(m["S0"])])
    return stats, int(ok.sum()), m, (preds, ev)


def host_stats(st, mode="median"):
    """(stats (B, 6), counts (B,)) of members (B, E, T, 8)."""
    res = [host_fit(st[b], mode) for b in range(st.shape[0])]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res])


def layouts(st, dtype):
    """(B, T, E, 8) views: make_time_major's (T, E, n, B) buffer and a
    contiguous (B, T, E, n) tensor."""
    import torch
    from eks_amd import batch
    yield "time-major", batch.make_time_major(st, dtype=dtype)
    yield "contiguous", torch.from_numpy(
        np.ascontiguousarray(st.transpose(0, 2, 1, 3).astype(dtype))).to("cuda")


def rel_err(got, want):
    """max |got - want| / |want| over the finite entries; the NaN patterns must match."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    f = ~np.isnan(want)
    if not f.any():
        return 0.0
    return float((np.abs(got[f] - want[f]) / np.abs(want[f])).max())


def with_gaps(st, seed, frac=0.2, blink=None, kill_first=True, inf_at=None):
    """A copy of members (B, E, T, 8): one NaN member in ~frac of the frames,
    a blink (every member NaN) over frames blink = (t0, t1), frame 0
    incomplete, an inf member at frame inf_at."""
    B, E, T, n = st.shape
    g = st.copy()
    rng = np.random.default_rng(seed)
    hit = rng.random((B, T)) < frac
    e = rng.integers(0, E, size=(B, T))
    j = rng.integers(0, n, size=(B, T))
    for b, t in zip(*np.nonzero(hit)):
        g[b, e[b, t], t, j[b, t]] = np.nan
    if blink is not None:
        g[:, :, blink[0]:blink[1], :] = np.nan
    if kill_first:
        g[:, 0, 0, 3] = np.nan
    if inf_at is not None:
        g[:, E - 1, inf_at, 5] = np.inf
        g[0, 0, inf_at + 1, 2] = -np.inf
    return g


# -- 1: shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 2), (1, 97), (3, 4099), (70, 1000)])
@pytest.mark.parametrize("E", [2, 5, 8])
def test_shapes(torch, B, T, E):
    """Both lane mappings (B below and above the switch), B no multiple of 64,
    T off every segment and wave boundary, the minimum T; compiled (5, 8) and
    runtime (2) member counts, both modes, both member types, both layouts."""
    from eks_amd import batch
    st = members(B, T, E)
    worst = 0.0
    for mode in ("median", "mean"):
        want, cnt = host_stats(st, mode)
        assert (cnt == T).all()
        for dtype in (np.float32, np.float64):
            for name, obs in layouts(st, dtype):
                res = batch.fit_pupil(obs, mode=mode)
                assert res["yev"] is None
                assert (res["status"] == 0).all() and (res["ncomplete"] == T).all()
                err = rel_err(res["stats"].cpu().numpy(), want)
                worst = max(worst, err)
                assert err <= STAT_RTOL, (mode, dtype, name, err)
    print(f"[fit pupil] B={B} T={T} E={E}: stats rel {worst:.3e}")


# -- 2: gaps -----------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,blink", [(3, 4099, (500, 1100)), (20, 203, (30, 70))])
def test_gaps(torch, B, T, blink):
    """Scattered NaN members over ~20 % of the frames, a blink that wipes whole
    lane chunks and a whole block's range (its partials are empty), frame 0
    incomplete, an inf member: the counts equal the host's and the statistics
    match the host fit on preds[ok].  (3, 4099) runs frames across a wave,
    (20, 203) the trajectory-fastest lanes."""
    from eks_amd import batch
    worst = 0.0
    for E in (2, 5):
        g = with_gaps(members(B, T, E), seed=B + E, blink=blink, inf_at=T - 9)
        for mode in ("median", "mean"):
            want, cnt = host_stats(g, mode)
            assert (cnt < 0.85 * T).all() and (cnt > 0.5 * T).all()
            for dtype in (np.float32, np.float64):
                for name, obs in layouts(g, dtype):
                    res = batch.fit_pupil(obs, mode=mode)
                    assert (res["status"] == 0).all()
                    assert np.array_equal(res["ncomplete"].cpu().numpy(), cnt), (mode, name)
                    err = rel_err(res["stats"].cpu().numpy(), want)
                    worst = max(worst, err)
                    assert err <= STAT_RTOL, (E, mode, dtype, name, err)
    print(f"[fit pupil] gaps B={B} T={T}: stats rel {worst:.3e}")


# -- 3: degenerate trajectories -----------------------------------------------------------
@pytest.mark.parametrize("T", [700])
def test_degenerate_trajectories(torch, T):
    from eks_amd import _lib, batch
    E = 5
    st = members(4, T, E)
    g = with_gaps(st, seed=3, frac=0.1, kill_first=False)
    g[0] = np.nan                      # nothing observed
    g[1] = np.nan                      # exactly one complete frame
    g[1, :, 333, :] = st[1, :, 333, :]
    want, cnt = host_stats(g)
    assert cnt[0] == 0 and cnt[1] == 1 and (cnt[2:] > 0.8 * T).all()
    for name, obs in layouts(g, np.float32):
        res = batch.fit_pupil(obs, check=False)
        stats = res["stats"].cpu().numpy()
        status = res["status"].cpu().numpy()
        assert np.array_equal(res["ncomplete"].cpu().numpy(), cnt)
        assert status[0] == _lib.EKS_STATUS_SINGULAR and (status[1:] == 0).all()
        assert np.isnan(stats[0]).all()
        assert (stats[1, 3:] == 0.0).all()          # variances exactly 0
        assert np.array_equal(stats[1, :3], want[1, :3])  # means equal that frame
        assert rel_err(stats[2:], want[2:]) <= STAT_RTOL
        for b in (2, 3):  # bit-identical to the same trajectory fitted alone
            alone = batch.fit_pupil(obs[b:b + 1])
            assert np.array_equal(alone["stats"].cpu().numpy()[0], stats[b]), (name, b)
            assert int(alone["ncomplete"][0]) == cnt[b]
        with pytest.raises(ValueError, match="no complete frame"):
            batch.fit_pupil(obs, check=True)


# -- 4: planes ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(3, 1031), (20, 203)])
@pytest.mark.parametrize("E", [2, 5])
def test_planes(torch, B, T, E):
    """The planes fit_pupil writes are eks_ensemble_gaps(min_members=E)'s byte
    for byte; the fit from those planes has the bits of the fit from the
    members; the fit from min_members=3 planes matches the host fit on the
    reference's planes."""
    from eks_amd import _lib, batch
    g = with_gaps(members(B, T, E), seed=11 + E, blink=(100, 140), inf_at=T - 5)
    lib = _lib.load()
    for mode in ("median", "mean"):
        m = _lib.EKS_MEDIAN if mode == "median" else _lib.EKS_MEAN
        nbytes = lib.eks_yev_bytes(B, T, 8, _lib.EKS_F64, E, m)
        for dtype in (np.float32, np.float64):
            for name, obs in layouts(g, dtype):
                res = batch.fit_pupil(obs, mode=mode, keep_yev=True)
                ens = batch.ensemble_gaps(obs, n=8, mode=mode, min_members=E)["yev"]
                yev = res["yev"]
                assert yev.code == _lib.EKS_YEV64 and yev.shape == (B, T, E, 8)
                sz = T * 8 * B * 8
                off = (sz + 255) // 256 * 256
                for lo in (0, off):  # (the padding between the planes is not written)
                    assert torch.equal(yev.buf[lo:lo + sz], ens.buf[lo:lo + sz]), (mode, name)
                assert off + sz == nbytes
                again = batch.fit_pupil(ens)
                assert again["yev"] is ens
                assert torch.equal(again["stats"], res["stats"]), (mode, dtype, name)
                assert torch.equal(again["ncomplete"], res["ncomplete"])
                reuse = batch.fit_pupil(obs, mode=mode, keep_yev=yev)
                assert reuse["yev"].buf.data_ptr() == yev.buf.data_ptr()
        with pytest.raises(ValueError, match="keep_yev"):
            batch.fit_pupil(ens, keep_yev=True)
    if E < 3:
        return
    obs = next(layouts(g, np.float32))[1]
    res = batch.fit_pupil(batch.ensemble_gaps(obs, n=8, min_members=3)["yev"])
    y, ev, _ = R.ensemble_valid(g.transpose(1, 0, 2, 3), "median", 3)  # (B, T, 8)
    fits = [host_fit(None, planes=(y[b], ev[b])) for b in range(B)]
    all_members = host_stats(g)[1]
    cnt = np.array([f[1] for f in fits])
    assert (cnt > all_members).all()
    assert np.array_equal(res["ncomplete"].cpu().numpy(), cnt)
    assert rel_err(res["stats"].cpu().numpy(), np.stack([f[0] for f in fits])) <= STAT_RTOL


# -- 5: determinism ----------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(2, 5000), (40, 777)])
def test_bit_identical_from_run_to_run(torch, B, T):
    from eks_amd import batch
    g = with_gaps(members(B, T, 5), seed=21, blink=(64, 128))
    obs = next(layouts(g, np.float32))[1]
    a = batch.fit_pupil(obs, keep_yev=True)
    b = batch.fit_pupil(obs, keep_yev=True)
    assert torch.equal(a["stats"], b["stats"]) and torch.equal(a["ncomplete"], b["ncomplete"])
    sz = T * 8 * B * 8
    off = (sz + 255) // 256 * 256
    for lo in (0, off):  # (the padding between the planes is not written)
        assert torch.equal(a["yev"].buf[lo:lo + sz], b["yev"].buf[lo:lo + sz])
    assert torch.isfinite(a["stats"]).all()


# -- 6: pupil_sweep ----------------------------------------------------------------------
def test_pupil_sweep(torch):
    from eks_amd import batch
    B, T, E = 3, 3000, 5
    ds, cs = [0.9, 0.99, 0.999, 0.9999], [0.8, 0.95, 0.99, 0.999]
    grid = [(d, c) for d in ds for c in cs]
    K = len(grid)
    g = with_gaps(members(B, T, E, seed=6), seed=6, frac=0.1, blink=(1500, 1520))
    obs = next(layouts(g, np.float32))[1]
    sw = batch.pupil_sweep(obs, ds, cs, want_var=True)
    # host-fitted rows, row k * B + b
    fits = [[host_fit(g[b], A=np.diag([d, c, c])) for b in range(B)] for d, c in grid]
    rows = torch.cat([batch.pack_params(*(f[2][k] for k in ("m0", "S0", "A", "Q", "C", "offset")))
                      for fk in fits for f in fk])
    ref = batch.nll_sweep_gaps(obs, rows, K=K, n=8, r=3)
    host = ref["nll"].cpu().numpy()
    got = sw["nll"].cpu().numpy()
    assert got.shape == (K, B)
    d_nll = float((np.abs(got - host) / np.abs(host)).max())
    assert d_nll <= NLL_RTOL
    best = sw["best"].cpu().numpy()
    hidx = host.argmin(axis=0)
    for b in range(B):
        k = grid.index((best[b, 0], best[b, 1]))
        assert abs(host[k, b] - host[hidx[b], b]) <= NLL_RTOL * abs(host[hidx[b], b])
    hrows = rows.view(K, B, -1)[torch.as_tensor(hidx, device=rows.device),
                                torch.arange(B, device=rows.device)].contiguous()
    sm = batch.smooth_gaps(obs, hrows, n=8, r=3, want_ms=True, want_var=True)
    d_out = float((sw["out"] - sm["out"]).abs().max())
    d_ms = float((sw["ms"] - sm["ms"]).abs().max())
    d_var = float(((sw["var"] - sm["var"]).abs() / sm["var"]).max())
    assert torch.isfinite(sw["out"]).all()
    preds_ev = [fits[0][b][3] for b in range(B)]
    nobs = [int((np.isfinite(p) & np.isfinite(e)).sum()) for p, e in preds_ev]
    assert sw["nobs"].cpu().tolist() == nobs == sm["nobs"].cpu().tolist()
    assert sw["ncomplete"].cpu().tolist() == [fits[0][b][1] for b in range(B)]
    assert sw["params"].shape == (B, batch.param_len(8, 3)) and int(sw["status"].abs().sum()) == 0
    print(f"[fit pupil] sweep: nll rel {d_nll:.3e}, out {d_out:.3e} px, ms {d_ms:.3e}, "
          f"var rel {d_var:.3e}")
    assert d_out <= OUT_TOL and d_ms <= OUT_TOL and d_var <= VAR_RTOL


# -- 7: wrappers -------------------------------------------------------------------------
def frames_of(arr):
    from eks_amd import fit
    return [pd.DataFrame(arr[e], columns=list(fit.PUPIL_KEYS)) for e in range(arr.shape[0])]


@pytest.mark.parametrize("allow_missing", [True, False])
def test_wrapper_fit_on_device(torch, allow_missing):
    from eks_amd.pupil_smoother import ensemble_kalman_smoother_pupil as pupil
    T, E = 3000, 5
    st = members(1, T, E, seed=7)
    gap = with_gaps(st, seed=7, frac=0.05, blink=(700, 730))[0]
    arr = gap if allow_missing else st[0]
    A = np.diag([.9999, .999, .999])
    kw = dict(posterior_var=True, allow_missing=allow_missing)
    old = pupil(frames_of(arr), KPS, "tracker", A, **kw)
    new = pupil(frames_of(arr), KPS, "tracker", A, fit_on_device=True, **kw)
    assert set(new) == set(old)
    xy = np.arange(12) % 3 != 2
    for key in ("markers_df", "latents_df"):
        assert list(new[key].columns) == list(old[key].columns)
        a, b = new[key].to_numpy(), old[key].to_numpy()
        if key == "markers_df":
            assert np.isnan(a[:, ~xy]).all()
            a, b = a[:, xy], b[:, xy]
        assert np.isfinite(a).all()
        d = float(np.abs(a - b).max())
        print(f"[fit pupil] wrapper allow_missing={allow_missing} {key}: {d:.3e}")
        assert d <= OUT_TOL
    for key in ("posterior_var_df", "latents_posterior_var_df"):
        a, b = new[key].to_numpy(), old[key].to_numpy()
        if key == "posterior_var_df":
            a, b = a[:, xy], b[:, xy]
        d = float((np.abs(a - b) / np.abs(b)).max())
        print(f"[fit pupil] wrapper allow_missing={allow_missing} {key}: rel {d:.3e}")
        assert d <= VAR_RTOL
    if allow_missing:
        assert new["n_missing"] == old["n_missing"] > 0
    else:
        with pytest.raises(ValueError, match="allow_missing=True"):
            pupil(frames_of(gap), KPS, "tracker", A, fit_on_device=True)


@pytest.mark.parametrize("allow_missing", [True, False])
def test_wrapper_sweep_fit_on_device(torch, allow_missing):
    from eks_amd.pupil_smoother import pupil_smoothing_sweep
    T, E = 3000, 5
    st = members(1, T, E, seed=8)
    gap = with_gaps(st, seed=8, frac=0.05, blink=(700, 730))[0]
    arr = gap if allow_missing else st[0]
    ds, cs = [0.9, 0.99, 0.9999], [0.9, 0.99, 0.999]
    old = pupil_smoothing_sweep(frames_of(arr), KPS, "tracker", ds, cs,
                                allow_missing=allow_missing)
    new = pupil_smoothing_sweep(frames_of(arr), KPS, "tracker", ds, cs,
                                allow_missing=allow_missing, fit_on_device=True)
    assert set(new) == set(old)
    host = np.sort(np.asarray(old["nll"]).ravel())
    assert (host[1] - host[0]) > 1e-6 * abs(host[0])  # the choice is no near-tie
    assert new["best"] == old["best"]
    d = float((np.abs(new["nll"] - old["nll"]) / np.abs(old["nll"])).max())
    print(f"[fit pupil] sweep wrapper allow_missing={allow_missing}: nll rel {d:.3e}")
    assert new["nll"].shape == old["nll"].shape and d <= NLL_RTOL
    xy = np.arange(12) % 3 != 2
    assert np.abs(new["markers_df"].to_numpy()[:, xy]
                  - old["markers_df"].to_numpy()[:, xy]).max() <= OUT_TOL
    assert np.abs(new["latents_df"].to_numpy() - old["latents_df"].to_numpy()).max() <= OUT_TOL
    if allow_missing:
        assert new["n_missing"] == old["n_missing"]
    else:
        with pytest.raises(ValueError, match="allow_missing=True"):
            pupil_smoothing_sweep(frames_of(gap), KPS, "tracker", ds, cs, fit_on_device=True)


def test_cli_device_fit(tmp_path, torch):
    """--device-fit of the pupil script writes the files of the default run
    (1e-8), with fixed parameters and with --sweep."""
    from eks_amd.scripts import pupil_example
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csv", "ibl-pupil")
    for tag, extra in [("fixed", []), ("sweep", ["--sweep", "0.99,0.9999", "0.99,0.999"])]:
        files = {}
        for dev in (False, True):
            out = tmp_path / f"{tag}_{int(dev)}"
            out.mkdir()
            args = ["--csv-dir", src, "--save-dir", str(out), "--eks_version", "standard",
                    "--no-plot", *extra, *(["--device-fit"] if dev else [])]
            files[dev] = pupil_example.run(pupil_example.build_parser().parse_args(args))
        for a, b in zip(files[False], files[True]):
            assert os.path.basename(a) == os.path.basename(b)
            hdr = [0, 1, 2] if "traces" in a else [0, 1]
            da = pd.read_csv(a, header=hdr, index_col=0).to_numpy(dtype=float)
            db = pd.read_csv(b, header=hdr, index_col=0).to_numpy(dtype=float)
            assert da.shape == db.shape and np.array_equal(np.isnan(da), np.isnan(db))
            f = ~np.isnan(da)
            assert f.any() and np.abs(da[f] - db[f]).max() <= OUT_TOL, (tag, a)


# -- 8: torch op -------------------------------------------------------------------------
def test_torch_op(torch):
    import eks_amd.ops  # noqa: F401
    from eks_amd import batch
    for B, T in [(2, 301), (33, 120)]:
        g = with_gaps(members(B, T, 5), seed=31, blink=(40, 60))
        for name, obs in layouts(g, np.float32):
            for mode in ("median", "mean"):
                want = batch.fit_pupil(obs, mode=mode, keep_yev=True)
                stats, ncomplete, status, yev = torch.ops.eks.fit_pupil(obs, mode)
                assert torch.equal(stats, want["stats"]), (name, mode)
                assert torch.equal(ncomplete, want["ncomplete"])
                assert torch.equal(status, want["status"])
                sz = T * 8 * B * 8
                off = (sz + 255) // 256 * 256
                assert yev.numel() == off + sz
                for lo in (0, off):
                    assert torch.equal(yev[lo:lo + sz], want["yev"].buf[lo:lo + sz])
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.eks.fit_pupil(torch.zeros((2, 100, 5, 8)), "median")
