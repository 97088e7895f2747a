"""The likelihood sweep on the device (eks_nll_sweep, batch.nll_sweep,
batch.select_smooth_param, torch.ops.eks.nll_sweep, smooth_param=None in the
wrappers) against oracle.compute_nll and against batch.nll per candidate.

Bounds: rtol 1e-9 against the oracle (the project's NLL-vs-oracle bound,
test_gpu_configs.py / test_gpu_pupil.py) and 2e-9 against batch.nll (both are
within 1e-9 of the oracle).  On these inputs |oracle NLL| / T >= 4.6 for every
candidate, every argmin over the candidates is interior, and best and second
best differ by >= 5.5e-4 relative (test_sweep_host.py asserts it for the sv /
mc (3, 131) data).  Each check prints its measured maximum before asserting.
"""
import os

import numpy as np
import pandas as pd
import pytest

import sweep_data as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL_ORACLE, RTOL_NLL = 1e-9, 2e-9


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture
def sweep_chunk():
    """eks_debug_set(EKS_DBG_SWEEP_CHUNK, v) for one test, reset afterwards."""
    from eks_amd import _lib
    yield lambda v: _lib.debug_set(_lib.EKS_DBG_SWEEP_CHUNK, v)
    _lib.debug_set(_lib.EKS_DBG_SWEEP_CHUNK, 0)


def close(got, ref, what, rtol):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    rel = float(np.max(np.abs(got - ref) / np.abs(ref)))
    print(f"[sweep] {what}: max rel err {rel:.3e} (bound {rtol:.0e})")
    assert np.isfinite(got).all(), what
    assert rel <= rtol, (what, rel)


def rows_of(torch, models, scales=D.SCALES):
    return torch.from_numpy(D.candidate_rows(models, scales)).cuda()


def sweep(torch, st, rows, K, n, r, dtype=np.float32, **kw):
    """(nll (K, B) numpy, status (K, B) numpy, the member view)."""
    from eks_amd import batch
    d = batch.make_time_major(st, dtype=dtype)
    status = torch.empty((K, st.shape[0]), dtype=torch.int32, device="cuda")
    got = batch.nll_sweep(d, rows, K=K, n=n, r=r, status=status, **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy(), status.cpu().numpy(), d


def per_candidate(torch, d, rows, K, n, r, **kw):
    """K back-to-back batch.nll calls: the route without the sweep."""
    from eks_amd import batch
    B = d.shape[0]
    return np.stack([batch.nll(d, rows[k * B:(k + 1) * B].contiguous(), n=n, r=r, **kw).cpu().numpy()
                     for k in range(K)])


def both_bounds(torch, kind, B, T, n, r, what, V=4, **kw):
    st, models, ref = D.dataset(kind, B, T, V=V)
    rows = rows_of(torch, models)
    K = len(D.SCALES)
    got, status, d = sweep(torch, st, rows, K, n, r, **kw)
    assert not status.any(), status
    close(got, ref, f"{what} vs oracle", RTOL_ORACLE)
    close(got, per_candidate(torch, d, rows, K, n, r), f"{what} vs batch.nll", RTOL_NLL)
    return got


# -- 1: (2,2), serial scan, ragged last chunk, partial waves; automatic; one chunk ------
@pytest.mark.parametrize("chunk", [8, 0, 136])
def test_singleview_chunked_auto_single(torch, sweep_chunk, chunk):
    from eks_amd import _lib
    sweep_chunk(chunk)
    L = _lib.load().eks_nll_sweep_chunk_len(3, 7, 131, 2)
    assert L == (chunk if chunk else L) and L % 8 == 0
    if chunk == 8:
        assert -(-131 // L) == 17 and 131 - 16 * 8 == 3
    if chunk == 136:
        assert L >= 131
    both_bounds(torch, "sv", 3, 131, 2, 2, f"sv B=3 T=131 chunk={chunk}")


# -- 2: (2,2), 263 chunks: one wave per row --------------------------------------------
def test_singleview_wave_scan(torch, sweep_chunk):
    from eks_amd import _lib
    sweep_chunk(8)
    assert _lib.load().eks_nll_sweep_chunk_len(2, 7, 2100, 2) == 8
    assert -(-2100 // 8) == 263 > int(os.environ.get("EKS_WAVE_SCAN_CHUNKS", 24))
    both_bounds(torch, "sv", 2, 2100, 2, 2, "sv B=2 T=2100 chunk=8")


# -- 3: (3,8) dense C, four cameras; runtime n: five cameras ----------------------------
def test_multicam_four_cameras(torch, sweep_chunk):
    sweep_chunk(8)
    both_bounds(torch, "mc", 3, 131, 8, 3, "mc V=4 B=3 T=131 chunk=8")


def test_multicam_five_cameras(torch):
    both_bounds(torch, "mc", 2, 300, 10, 3, "mc V=5 n=10 B=2 T=300", V=5)


# -- 4: the pupil model; candidates that also differ in A -------------------------------
def test_pupil(torch, sweep_chunk):
    sweep_chunk(8)
    both_bounds(torch, "pupil", 2, 131, 8, 3, "pupil B=2 T=131 chunk=8")


def test_pupil_candidates_differ_in_A(torch, sweep_chunk):
    sweep_chunk(8)
    st, _, _ = D.dataset("pupil", 2, 131)
    grid = [(.99, .99), (.999, .99), (.9999, .999), (.99, .9999)]
    cands = [[D.model_of("pupil", st[b], A=(d, c, c)) for b in range(2)] for d, c in grid]
    rows = torch.cat([rows_of(torch, ms, scales=(1.0,)) for ms in cands])
    ref = np.array([[D.oracle_nll(st[b], ms[b]) for b in range(2)] for ms in cands])
    assert len({m["A"][0, 0] for ms in cands for m in ms}) == 3
    got, status, d = sweep(torch, st, rows, len(grid), 8, 3)
    assert not status.any()
    close(got, ref, "pupil (d, c) grid vs oracle", RTOL_ORACLE)
    close(got, per_candidate(torch, d, rows, len(grid), 8, 3), "pupil (d, c) grid vs batch.nll",
          RTOL_NLL)


# -- 5: T = 1 and T = 2 ------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2])
def test_shortest_trajectories(torch, T):
    st, models, _ = D.dataset("sv", 3, 131)
    sub = np.ascontiguousarray(st[:, :, :T])
    ref = np.array([[D.oracle_nll(sub[b], models[b], s) for b in range(3)] for s in D.SCALES])
    rows = rows_of(torch, models)
    got, status, d = sweep(torch, sub, rows, 7, 2, 2)
    assert not status.any()
    close(got, ref, f"sv T={T} vs oracle", RTOL_ORACLE)
    close(got, per_candidate(torch, d, rows, 7, 2, 2), f"sv T={T} vs batch.nll", RTOL_NLL)


# -- 6: whole blocks per chunk in the element kernel: K B = 256 rows ----------------------
def test_uniform_lanes(torch, sweep_chunk):
    sweep_chunk(8)
    scales = tuple(10.0 ** e for e in range(-3, 5))  # K = 8
    rng = np.random.default_rng(7 * 32 + 24)
    from eks_amd import synthetic
    st = synthetic.singleview_obs(rng, 5, 24, K=32).transpose(2, 0, 1, 3).astype(np.float64)
    models = [D.model_of("sv", st[b]) for b in range(32)]
    ref = np.array([[D.oracle_nll(st[b], models[b], s) for b in range(32)] for s in scales])
    rows = rows_of(torch, models, scales)
    assert rows.shape[0] == 256
    got, status, d = sweep(torch, st, rows, 8, 2, 2)
    assert not status.any()
    close(got, ref, "sv K B=256 T=24 chunk=8 vs oracle", RTOL_ORACLE)
    close(got, per_candidate(torch, d, rows, 8, 2, 2), "sv K B=256 T=24 chunk=8 vs batch.nll",
          RTOL_NLL)


# -- 7: float64 members, mean, the y / ev hand-off, reproducibility, the operator --------
def test_float64_members_and_mean(torch, sweep_chunk):
    sweep_chunk(8)
    st, models, ref = D.dataset("mc", 3, 131)
    rows = rows_of(torch, models)
    got64, status, _ = sweep(torch, st, rows, 7, 8, 3, dtype=np.float64)
    assert not status.any()
    close(got64, ref, "mc float64 members vs oracle", RTOL_ORACLE)
    got32, _, _ = sweep(torch, st, rows, 7, 8, 3)
    np.testing.assert_allclose(got64, got32, rtol=1e-12, atol=0)  # float32-exact members
    ref_mean = np.array([[D.oracle_nll(st[b], models[b], s, mode="mean") for b in range(3)]
                         for s in D.SCALES])
    got, status, d = sweep(torch, st, rows, 7, 8, 3, mode="mean")
    assert not status.any()
    close(got, ref_mean, "mc mode=mean vs oracle", RTOL_ORACLE)
    close(got, per_candidate(torch, d, rows, 7, 8, 3, mode="mean"), "mc mode=mean vs batch.nll",
          RTOL_NLL)
    assert not np.array_equal(got, got32)


@pytest.mark.parametrize("kind,n,r", [("sv", 2, 2), ("mc", 8, 3)])
def test_yev_handoff_input_is_bit_identical(torch, sweep_chunk, kind, n, r):
    from eks_amd import batch
    sweep_chunk(8)
    st, models, ref = D.dataset(kind, 3, 131)
    rows = rows_of(torch, models)
    d = batch.make_time_major(st, dtype=np.float32)
    _, _, yev = batch.fit(d, kind="singleview" if kind == "sv" else "multicam", n=n, r=r,
                          smooth_param=1.0, quantile_keep=50.0, keep_yev=True)
    a = batch.nll_sweep(d, rows, K=7, n=n, r=r)
    b = batch.nll_sweep(yev, rows, K=7, n=n, r=r)
    assert torch.equal(a, b)
    close(b.cpu().numpy(), ref, f"{kind} Yev vs oracle", RTOL_ORACLE)


def test_two_calls_are_bit_identical_and_operator(torch, sweep_chunk):
    from eks_amd import batch
    import eks_amd.ops  # noqa: F401
    for chunk, (B, T) in ((8, (2, 2100)), (8, (3, 131)), (136, (3, 131))):
        sweep_chunk(chunk)
        st, models, ref = D.dataset("sv", B, T)
        rows = rows_of(torch, models)
        d = batch.make_time_major(st, dtype=np.float32)
        a = batch.nll_sweep(d, rows, K=7, n=2, r=2)
        b = batch.nll_sweep(d, rows, K=7, n=2, r=2)
        assert torch.equal(a, b), (chunk, B, T)
    nll_op, st_op = torch.ops.eks.nll_sweep(d, rows, 7, 2, 2, "median")
    assert torch.equal(nll_op, a) and st_op.shape == (7, 3) and int(st_op.abs().sum()) == 0


# -- 8: status -----------------------------------------------------------------------------
def test_identical_members_are_flagged_and_recomputed(torch, sweep_chunk):
    from eks_amd import _lib
    sweep_chunk(8)
    st, models, ref = D.dataset("sv", 3, 131)
    ex = st.copy()
    ex[1, :, 5, :] = ex[1, 0, 5, :]   # all members equal: both coordinates
    ex[1, :, 40, 0] = ex[1, 0, 40, 0]  # x only
    rows = rows_of(torch, models)
    got, status, d = sweep(torch, ex, rows, 7, 2, 2, check=False)
    assert (status[:, 1] == _lib.EKS_STATUS_SCAN).all() and not status[:, [0, 2]].any()
    assert np.isnan(got[:, 1]).all()
    close(got[:, [0, 2]], ref[:, [0, 2]], "sv identical members: the other trajectories",
          RTOL_ORACLE)
    got, status, _ = sweep(torch, ex, rows, 7, 2, 2, check=True)
    assert not status.any()
    want = per_candidate(torch, d, rows, 7, 2, 2)
    np.testing.assert_array_equal(got[:, 1], want[:, 1])
    close(got, want, "sv identical members, check=True vs batch.nll", RTOL_NLL)


def test_rank_deficient_C_is_flagged_and_recomputed(torch, sweep_chunk):
    from eks_amd import _lib
    sweep_chunk(8)
    st, models, ref = D.dataset("sv", 3, 131)
    models = [dict(m) for m in models]
    models[2]["C"] = np.array([[1.0, 0.0], [1.0, 0.0]])
    rows = rows_of(torch, models)
    got, status, d = sweep(torch, st, rows, 7, 2, 2, check=False)
    assert (status[:, 2] == _lib.EKS_STATUS_SCAN).all() and not status[:, :2].any()
    assert np.isnan(got[:, 2]).all()
    close(got[:, :2], ref[:, :2], "sv rank-deficient C: the other trajectories", RTOL_ORACLE)
    got, status, _ = sweep(torch, st, rows, 7, 2, 2, check=True)
    assert not status.any()
    want = per_candidate(torch, d, rows, 7, 2, 2)
    np.testing.assert_array_equal(got[:, 2], want[:, 2])
    close(got, want, "sv rank-deficient C, check=True vs batch.nll", RTOL_NLL)


@pytest.mark.parametrize("chunk", [8, 136])
def test_changed_offset_is_a_bad_model_on_that_row_only(torch, sweep_chunk, chunk):
    from eks_amd import _lib
    sweep_chunk(chunk)
    st, models, ref = D.dataset("sv", 3, 131)
    rows = rows_of(torch, models)
    rows[4 * 3 + 1, -1] += 0.5  # candidate 4 of trajectory 1: offset_y
    got, status, _ = sweep(torch, st, rows, 7, 2, 2, check=False)
    want = np.zeros((7, 3), dtype=np.int32)
    want[4, 1] = _lib.EKS_STATUS_BAD_MODEL
    np.testing.assert_array_equal(status, want)
    keep = want == 0
    close(got[keep], ref[keep], f"sv changed offset chunk={chunk}: the other rows", RTOL_ORACLE)
    with pytest.raises(ValueError):
        sweep(torch, st, rows, 7, 2, 2, check=True)


def test_nan_member_gives_nan_and_no_bit(torch, sweep_chunk):
    st, models, ref = D.dataset("sv", 3, 131)
    bad = st.copy()
    bad[1, 2, 60, 1] = np.nan
    rows = rows_of(torch, models)
    for chunk in (8, 136):
        sweep_chunk(chunk)
        got, status, _ = sweep(torch, bad, rows, 7, 2, 2, check=False)
        assert not status.any(), (chunk, status)
        assert np.isnan(got[:, 1]).all()
        close(got[:, [0, 2]], ref[:, [0, 2]], f"sv NaN member chunk={chunk}: the other trajectories",
              RTOL_ORACLE)
    st2, models2, ref2 = D.dataset("sv", 2, 2100)
    bad = st2.copy()
    bad[0, 1, 1000, 0] = np.nan
    sweep_chunk(8)  # 263 chunks: one wave per row
    got, status, _ = sweep(torch, bad, rows_of(torch, models2), 7, 2, 2, check=False)
    assert not status.any() and np.isnan(got[:, 0]).all()
    close(got[:, 1], ref2[:, 1], "sv NaN member, wave scan: the other trajectory", RTOL_ORACLE)


# -- 9: selection ----------------------------------------------------------------------------
def base_params(torch, models):
    return rows_of(torch, models, scales=(1.0,))


@pytest.mark.parametrize("kind,B,T,n,r", [("sv", 3, 131, 2, 2), ("mc", 3, 131, 8, 3),
                                          ("pupil", 2, 131, 8, 3), ("sv", 2, 2100, 2, 2)])
def test_refine_zero_returns_the_oracles_argmin(torch, kind, B, T, n, r):
    from eks_amd import batch
    st, models, ref = D.dataset(kind, B, T)
    d = batch.make_time_major(st, dtype=np.float32)
    res = batch.select_smooth_param(d, base_params(torch, models), n=n, r=r, grid=D.SCALES,
                                    refine=0)
    want = np.array(D.SCALES)[np.argmin(ref, axis=0)]
    print(f"[sweep] {kind} B={B} T={T}: oracle argmin {want}, chosen "
          f"{res['smooth_param'].cpu().numpy()}")
    np.testing.assert_array_equal(res["smooth_param"].cpu().numpy(), want)
    close(res["nll"].cpu().numpy(), np.min(ref, axis=0), f"{kind} NLL at the argmin", RTOL_ORACLE)
    assert not bool(res["at_edge"].any())


@pytest.mark.parametrize("kind,n,r", [("sv", 2, 2), ("mc", 8, 3)])
def test_refinement_lowers_the_nll(torch, sweep_chunk, kind, n, r):
    from eks_amd import batch
    sweep_chunk(8)  # one chunk length for K = 7 and K = 1: the same association per row
    st, models, ref = D.dataset(kind, 3, 131)
    d = batch.make_time_major(st, dtype=np.float32)
    base = base_params(torch, models)
    coarse = batch.select_smooth_param(d, base, n=n, r=r, grid=D.SCALES, refine=0)
    fine = batch.select_smooth_param(d, base, n=n, r=r, grid=D.SCALES, refine=2)
    s = fine["smooth_param"]
    print(f"[sweep] {kind}: coarse {coarse['smooth_param'].cpu().numpy()} nll "
          f"{coarse['nll'].cpu().numpy()}, refined {s.cpu().numpy()} nll {fine['nll'].cpu().numpy()}")
    # the device NLL at the returned s, recomputed from the returned rows
    again = batch.nll_sweep(d, fine["params"], K=1, n=n, r=r)[0]
    assert torch.equal(again, fine["nll"])
    assert bool((fine["nll"] <= coarse["nll"]).all())
    assert not bool(fine["at_edge"].any())
    want = base.clone()
    q0 = r + 2 * r * r
    want[:, q0:q0 + r * r] *= s.unsqueeze(1)
    assert torch.equal(fine["params"], want)
    # within the refined grid's reach of the coarse best
    ratio = (s / coarse["smooth_param"]).cpu().numpy()
    assert np.all((ratio > 0.1) & (ratio < 10.0))


def test_wrappers_with_smooth_param_none(torch):
    from eks_amd.multiview_pca_smoother import ensemble_kalman_smoother_multi_cam
    from eks_amd.singleview_smoother import ensemble_kalman_smoother_single_view
    g = np.load(os.path.join(GOLDEN, "singleview_c1.npz"))
    obs = g["obs"]
    dfs = [pd.DataFrame(obs[e], columns=["nose_x", "nose_y"]) for e in range(len(obs))]
    a = ensemble_kalman_smoother_single_view(dfs, "nose", None, float(g["q"]))
    s = a["smooth_param"]
    assert isinstance(s, float) and 1e-4 <= s <= 1e4
    b = ensemble_kalman_smoother_single_view(dfs, "nose", s, float(g["q"]))
    assert set(a) == set(b) | {"smooth_param"}
    pd.testing.assert_frame_equal(a["markers_df"], b["markers_df"], check_exact=True)
    assert a["nll"] == b["nll"]
    print(f"[sweep] single-view wrapper: smooth_param {s:.6g}, nll {a['nll']:.6f}")
    # a number behaves as before: no new key
    assert "smooth_param" not in b
    st, _, _ = D.dataset("mc", 3, 131)
    cams = [f"cam{c}" for c in range(4)]
    markers = [[pd.DataFrame(st[0, e][:, 2 * c:2 * c + 2], columns=["x", "y"]) for e in range(5)]
               for c in range(4)]
    a = ensemble_kalman_smoother_multi_cam(markers, "paw", None, 25, cams)
    s = a["smooth_param"]
    b = ensemble_kalman_smoother_multi_cam(markers, "paw", s, 25, cams)
    assert set(a) == set(b) | {"smooth_param"}
    for cam in cams:
        pd.testing.assert_frame_equal(a[cam + "_df"], b[cam + "_df"], check_exact=True)
    print(f"[sweep] multi-cam wrapper: smooth_param {s:.6g}")


def test_multi_cam_batch_with_smooth_param_none(torch):
    from eks_amd.smoothers import multi_cam_batch
    st, _, _ = D.dataset("mc", 3, 131)
    out, s = multi_cam_batch(st, None, 25)
    assert out.shape == (3, 131, 8) and s.shape == (3,) and np.isfinite(out).all()
    for k in range(3):  # each keypoint equals a call with its own value
        np.testing.assert_allclose(out[k], multi_cam_batch(st[k:k + 1], float(s[k]), 25)[0],
                                   rtol=0, atol=1e-9)


def test_multicam_script_auto(tmp_path, capsys, torch):
    """--s auto of the multi-camera script: the chosen values are printed and
    the file holds the frames of a run with those values."""
    from eks_amd.scripts import multicam_example
    src = os.path.join(GOLDEN, "csv", "mirror-mouse")
    kps = ["paw1LH", "paw2LF"]
    common = ["--csv-dir", src, "--bodypart-list", *kps, "--camera-names", "top", "bot",
              "--eks_version", "standard", "--no-plot"]
    multicam_example.main([*common, "--save-dir", str(tmp_path), "--s", "auto"])
    printed = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("smooth_param")]
    assert len(printed) == 2 and all(kp in ln for kp, ln in zip(kps, printed))
    auto = pd.read_csv(tmp_path / "eks.csv", header=[0, 1, 2], index_col=0)
    for kp, ln in zip(kps, printed):
        s = float(ln.split(":")[-1])
        assert 1e-4 <= s <= 1e4
        one = tmp_path / kp
        one.mkdir()
        multicam_example.main(["--csv-dir", src, "--bodypart-list", kp, "--camera-names", "top",
                               "bot", "--eks_version", "standard", "--no-plot", "--save-dir",
                               str(one), "--s", repr(s)])
        ref = pd.read_csv(one / "eks.csv", header=[0, 1, 2], index_col=0)
        cols = [c for c in ref.columns if c[1].startswith(kp) and c[2] in ("x", "y")]
        # the printed value has six digits (5e-7 relative); an output moves by at most the
        # members' spread (< 100 px here) per unit of ln s: 100 px x 5e-7 = 5e-5 px
        err = np.abs(auto[cols].to_numpy() - ref[cols].to_numpy()).max()
        print(f"[sweep] multicam --s auto vs --s {s!r} ({kp}): max |d| {err:.3e} px")
        assert err < 1e-4


def test_singleview_script_auto(tmp_path, capsys, torch):
    """--s auto on the fixture tests/test_cli.py uses for the single-view script."""
    from eks_amd import io
    from eks_amd.scripts import singleview_example
    from eks_amd.singleview_smoother import ensemble_kalman_smoother_single_view
    src = os.path.join(GOLDEN, "csv", "mirror-mouse")
    kps = ["paw1LH_top", "paw2LF_bot"]
    singleview_example.main(["--csv-dir", src, "--bodypart-list", *kps, "--save-dir",
                             str(tmp_path), "--s", "auto"])
    printed = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("smooth_param")]
    assert len(printed) == 2 and all(kp in ln for kp, ln in zip(kps, printed))
    res = pd.read_csv(tmp_path / "eks.csv", header=[0, 1, 2], index_col=0)
    ml, _, _ = io.load_markers_dir(src)
    for kp, ln in zip(kps, printed):
        ref = ensemble_kalman_smoother_single_view(ml, kp, None, 25)
        assert abs(float(ln.split(":")[-1]) / ref["smooth_param"] - 1.0) < 1e-4, (ln, ref["smooth_param"])
        a = res.loc[:, ("ensemble-kalman_tracker", kp, ["x", "y"])].to_numpy()
        assert np.abs(a - ref["markers_df"].to_numpy()[:, :2]).max() < 1e-5
