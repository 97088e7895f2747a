"""Per-keypoint entry points, API-compatible with the reference wrappers.

    ensemble_kalman_smoother_multi_cam   eks/multiview_pca_smoother.py:611-767
    ensemble_kalman_smoother_pupil       eks/pupil_smoother.py:82-223
    ensemble_kalman_smoother_single_view build definition
    eks_opti_smoother_multi_cam          eks/multiview_pca_smoother.py:777-933
    eks_opti_smoother_pupil              eks/pupil_smoother.py:227-320

Flow for one keypoint: member DataFrames -> (E, T, n) array -> GPU ensemble
(eks_ensemble, written as the y / ev hand-off planes) -> host model fit
(eks_amd.fit, on the planes' host copies) -> GPU fused smoother from the
planes (eks_smooth: forward, backward, projection) -> DataFrames in the
reference's output format.  The members are uploaded and reduced once; no
step of the smoother runs on the CPU.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from . import _lib, batch, core, fit
from .newton_eks import kalman_newton_recursive, newton_filter_batch
from .utils import TRACKER, make_dlc_pandas_index


def _run_fused(stack: np.ndarray, model: dict, mode: str = "median", want_ms=False,
               want_nll=False, yev=None, want_var=False, want_Vs=False):
    """stack (E, T, n) float64 host array + model -> out (T, n), ms, nll
    (and, with ``want_var`` or ``want_Vs``, the posterior variances var (T, n)
    and covariances Vs (T, r, r) as a fourth and fifth value).
    With ``yev`` (core.ensemble_handoff's planes of the same stack) the
    smoother reads the planes instead of uploading and reducing the members
    again (every algorithm, the runtime-n kernels included)."""
    torch = _lib.require_gpu()
    E, T, n = stack.shape
    r = len(model["m0"])
    if yev is not None:
        obs = yev
    else:
        obs = torch.from_numpy(np.ascontiguousarray(stack, dtype=np.float64)).to("cuda")
        obs = obs.permute(1, 0, 2).unsqueeze(0)  # (1, T, E, n) view, no copy
    params = batch.pack_params(model["m0"], model["S0"], model["A"], model["Q"], model["C"],
                               model["offset"])
    res = batch.smooth(obs, params, n=n, r=r, mode=mode, want_ms=want_ms, want_nll=want_nll,
                       flags=batch.model_flags(model["A"], model["C"], model["Q"]), check=True,
                       want_var=want_var, want_Vs=want_Vs)
    out = res["out"][0].cpu().numpy()
    ms = res["ms"][0].cpu().numpy() if want_ms else None
    nll = float(res["nll"][0].item()) if want_nll else None
    if want_var or want_Vs:
        return (out, ms, nll, res["var"][0].cpu().numpy() if want_var else None,
                res["Vs"][0].cpu().numpy() if want_Vs else None)
    return out, ms, nll


def _complete_frames(preds, ev):
    """Frames whose ensemble average and variance are finite in every column."""
    return np.isfinite(preds).all(axis=1) & np.isfinite(ev).all(axis=1)


def _run_gaps(yev, model: dict, mode: str = "median", want_var=False):
    """The hand-off planes of one keypoint through batch.smooth_gaps (columns
    with a non-finite average or variance are missing) -> out (T, n), nll,
    var (T, n) or None, the number of missing entries."""
    _, T, _, n = yev.shape
    r = len(model["m0"])
    params = batch.pack_params(model["m0"], model["S0"], model["A"], model["Q"], model["C"],
                               model["offset"])
    res = batch.smooth_gaps(yev, params, n=n, r=r, mode=mode, want_var=want_var, want_nll=True,
                            check=True)
    return (res["out"][0].cpu().numpy(), float(res["nll"][0].item()),
            res["var"][0].cpu().numpy() if want_var else None,
            T * n - int(res["nobs"][0].item()))


def _posterior_draws(yev, params, *, n: int, r: int, S: int, seed: int, mode: str = "median",
                     want_latent: bool = False):
    """``S`` joint draws from the smoothing posterior of one keypoint, one
    batch.draws_gaps call on the planes and packed model the smoother read ->
    draws (S, T, n) and, if asked, the latent draws (S, T, r)."""
    res = batch.draws_gaps(yev, params, n=n, r=r, S=int(S), seed=int(seed), mode=mode,
                           want_latent=want_latent, want_out=False, check=True)
    return (res["draws"][0].cpu().numpy(),
            res["latent"][0].cpu().numpy() if want_latent else None)


def _model_draws(yev, model: dict, S: int, seed: int, mode: str = "median"):
    """_posterior_draws for a host model dict."""
    params = batch.pack_params(model["m0"], model["S0"], model["A"], model["Q"], model["C"],
                               model["offset"])
    return _posterior_draws(yev, params, n=len(model["offset"]), r=len(model["m0"]), S=S,
                            seed=seed, mode=mode)[0]


# ``posterior_draws=S`` (default 0: nothing changes) with ``draws_seed``, in the
# multi-camera, pupil and single-view wrappers below: the dict gains
# 'posterior_draws', a float64 (S, T, n) array of S joint draws from the
# smoothing posterior in the columns of the smoother's out (one extra
# batch.draws_gaps call on the same planes and model).  Unlike the posterior
# variances, the draws carry the correlation between frames.


def _auto_smooth_param(yev, model: dict, mode: str = "median") -> float:
    """The smoothing parameter chosen by likelihood (batch.select_smooth_param)
    for one keypoint: ``model`` fitted with smooth_param = 1, ``yev`` the
    hand-off planes the smoother will read."""
    n, r = len(model["offset"]), len(model["m0"])
    params = batch.pack_params(model["m0"], model["S0"], model["A"], model["Q"], model["C"],
                               model["offset"])
    sel = batch.select_smooth_param(yev, params, n=n, r=r, mode=mode)
    return float(sel["smooth_param"][0].item())


def _check_min_members(min_members, allow_missing):
    """``min_members`` (the ensemble over the valid members of each column,
    core.ensemble_handoff) changes what is missing: only with allow_missing."""
    if min_members is not None and not allow_missing:
        raise ValueError("min_members needs allow_missing=True")


# ``min_members`` (with ``allow_missing=True`` only), in every wrapper below:
# the ensemble is taken over the finite members of each column
# (batch.ensemble_gaps) and a column is missing only when fewer than
# ``min_members`` of them are finite -- one rejected member no longer discards
# its frame.  ``None``: a NaN prediction of any member makes its column missing.


def ensemble_kalman_smoother_multi_cam(markers_list_cameras, keypoint_ensemble, smooth_param,
                                       quantile_keep_pca, camera_names, posterior_var=False,
                                       allow_missing=False, min_members=None, posterior_draws=0,
                                       draws_seed=0):
    """Multi-view PCA smoother for one keypoint (eks/multiview_pca_smoother.py:611-767).

    ``smooth_param=None``: chosen by minimising the filter's NLL on the device
    (batch.select_smooth_param); the dict then gains 'smooth_param', and the
    frames equal those of a call with that value.

    ``allow_missing=True``: a column whose ensemble average or variance is not
    finite (a NaN prediction of any member) is a missing observation; the
    model is fitted on the frames that are complete in every column, the
    smoother steps over the gaps (batch.smooth_gaps) and every frame of the
    output is finite.  The dict gains 'n_missing', the number of missing
    entries.  It needs a ``smooth_param``.  With ``min_members`` a column is
    missing only when fewer than that many members are finite, and the
    ensemble is taken over the finite ones (batch.ensemble_gaps).

    markers_list_cameras[camera][model] is a DataFrame whose first two
    columns are that camera's x and y predictions.  Returns
    {f'{camera}_df': DataFrame} with (scorer, keypoint, x/y/likelihood)
    columns; likelihood is NaN as in the reference.  With ``posterior_var``
    the dict gains 'posterior_var_df': {f'{camera}_df': DataFrame} in the same
    layout, x / y holding the posterior variances of the smoothed x / y."""
    _check_min_members(min_members, allow_missing)
    V = len(camera_names)
    if V < 2:
        raise ValueError("ensemble_kalman_smoother_multi_cam needs at least two cameras "
                         "(the reference's 3-component PCA needs >= 3 columns); use "
                         "ensemble_kalman_smoother_single_view for one view")
    n_models = len(markers_list_cameras[0])
    cols = [np.stack([np.asarray(markers_list_cameras[c][e].to_numpy()[:, :2], dtype=np.float64)
                      for e in range(n_models)]) for c in range(V)]  # V x (E, T, 2)
    stack = np.concatenate(cols, axis=2)  # (E, T, 2V), camera-major columns
    if allow_missing and smooth_param is None:
        raise ValueError("allow_missing=True needs a smooth_param: the likelihood sweep does "
                         "not step over gaps")
    yev, preds, ev = core.ensemble_handoff(stack, min_members=min_members)
    auto = smooth_param is None
    dfs = {}
    if allow_missing:
        ok = _complete_frames(preds, ev)
        model = fit.multicam_model(preds[ok], ev[ok], smooth_param, quantile_keep_pca)
        out, _, var, dfs["n_missing"] = _run_gaps(yev, model, want_var=bool(posterior_var))
        pv = [var]
    else:
        if auto:
            smooth_param = _auto_smooth_param(
                yev, fit.multicam_model(preds, ev, 1.0, quantile_keep_pca))
        model = fit.multicam_model(preds, ev, smooth_param, quantile_keep_pca)
        out, _, _, *pv = _run_fused(stack, model, yev=yev, want_var=bool(posterior_var))
    pdindex = make_dlc_pandas_index([keypoint_ensemble])
    if auto:
        dfs["smooth_param"] = smooth_param
    nan = np.full(out.shape[0], np.nan)
    for c, cam in enumerate(camera_names):
        arr = np.stack([out[:, 2 * c], out[:, 2 * c + 1], nan], axis=1)
        dfs[cam + "_df"] = pd.DataFrame(arr, columns=pdindex)
    if posterior_var:
        dfs["posterior_var_df"] = _camera_dfs(pv[0], keypoint_ensemble, camera_names)
    if posterior_draws:
        dfs["posterior_draws"] = _model_draws(yev, model, posterior_draws, draws_seed)
    return dfs


def _run_gaps_pupil(yev, model: dict, pv: bool):
    """The pupil hand-off planes through batch.smooth_gaps -> out (T, 8),
    ms (T, 3), var (T, 8) and Vs (T, 3, 3) (None unless ``pv``), the number of
    missing entries."""
    _, T, _, n = yev.shape
    params = batch.pack_params(model["m0"], model["S0"], model["A"], model["Q"], model["C"],
                               model["offset"])
    res = batch.smooth_gaps(yev, params, n=n, r=3, want_ms=True, want_var=pv, want_Vs=pv,
                            check=True)
    return (res["out"][0].cpu().numpy(), res["ms"][0].cpu().numpy(),
            res["var"][0].cpu().numpy() if pv else None,
            res["Vs"][0].cpu().numpy() if pv else None, T * n - int(res["nobs"][0].item()))


def _pupil_device_obs(stack, min_members):
    """(E, T, 8) host members -> what batch.fit_pupil / batch.pupil_sweep read
    on the device: the (1, T, E, 8) member view, uploaded once, or with
    ``min_members`` the planes of batch.ensemble_gaps."""
    torch = _lib.require_gpu()
    obs = torch.from_numpy(np.ascontiguousarray(stack, dtype=np.float64)).to("cuda")
    obs = obs.permute(1, 0, 2).unsqueeze(0)  # (1, T, E, 8) view, no copy
    if min_members is not None:
        return batch.ensemble_gaps(obs, n=obs.shape[3], min_members=min_members)["yev"]
    return obs


def _check_device_complete(ncomplete, T, allow_missing):
    """allow_missing=False promises members without gaps to the device fit."""
    m = int(ncomplete[0].item())
    if not allow_missing and m < T:
        raise ValueError(f"the device fit found {T - m} of {T} frames with a missing or "
                         "non-finite prediction: pass allow_missing=True to fit on the "
                         "complete frames and smooth through the gaps")


def _pupil_dfs(out, ms, mx, my, keypoint_names, tracker_name, var=None, Vs=None):
    """The pupil wrappers' DataFrames from out (T, 8), ms (T, 3) and, for the
    posterior variances, var (T, 8) and Vs (T, 3, 3)."""
    nan = np.full(out.shape[0], np.nan)

    def markers(arr):
        by_key = {k: arr[:, j] for j, k in enumerate(fit.PUPIL_KEYS)}
        cols = []
        for kp in ('top', 'right', 'bottom', 'left'):  # output order of :199-203
            cols += [by_key[f'pupil_{kp}_r_x'], by_key[f'pupil_{kp}_r_y'], nan]
        return pd.DataFrame(np.stack(cols, 1), columns=make_dlc_pandas_index(keypoint_names))

    lat = np.stack([ms[:, 0], ms[:, 1] + mx, ms[:, 2] + my], 1)
    idx = pd.MultiIndex.from_arrays([[tracker_name] * 3, ['diameter', 'com_x', 'com_y']],
                                    names=('scorer', 'latent'))
    res = {'markers_df': markers(out), 'latents_df': pd.DataFrame(lat, columns=idx)}
    if var is not None:
        res['posterior_var_df'] = markers(var)
        res['latents_posterior_var_df'] = pd.DataFrame(
            np.diagonal(Vs, axis1=1, axis2=2).copy(), columns=idx)
    return res


def _pupil_draws(res, yev, params, mx, my, S, seed):
    """The pupil wrapper's draw keys: 'posterior_draws' (S, T, 8) in out's
    columns and 'latents_posterior_draws' (S, T, 3) in latents_df's."""
    draws, lat = _posterior_draws(yev, params, n=8, r=3, S=S, seed=seed, want_latent=True)
    res['posterior_draws'] = draws
    res['latents_posterior_draws'] = lat + np.array([0.0, mx, my])


def _pupil_on_device(stack, keypoint_names, tracker_name, state_transition_matrix, pv,
                     allow_missing, min_members, posterior_draws=0, draws_seed=0):
    """ensemble_kalman_smoother_pupil(fit_on_device=True): members -> fit ->
    smooth on the device; only the results come back."""
    A = np.asarray(state_transition_matrix, dtype=np.float64)
    if A.shape != (3, 3) or not batch._diagonal(A):
        raise ValueError("fit_on_device=True needs a diagonal 3 x 3 state_transition_matrix")
    T = stack.shape[1]
    obs = _pupil_device_obs(stack, min_members)
    f = batch.fit_pupil(obs, keep_yev=None if isinstance(obs, batch.Yev) else True)
    _check_device_complete(f["ncomplete"], T, allow_missing)
    params = batch.pupil_params(f["stats"], np.diag(A)[None])
    sm = batch.smooth_gaps(f["yev"], params, n=8, r=3, want_ms=True, want_var=pv, want_Vs=pv,
                           check=True)
    stats = f["stats"][0].cpu().numpy()
    res = _pupil_dfs(sm["out"][0].cpu().numpy(), sm["ms"][0].cpu().numpy(), stats[1], stats[2],
                     keypoint_names, tracker_name,
                     sm["var"][0].cpu().numpy() if pv else None,
                     sm["Vs"][0].cpu().numpy() if pv else None)
    if allow_missing:
        res['n_missing'] = T * 8 - int(sm["nobs"][0].item())
    if posterior_draws:
        _pupil_draws(res, f["yev"], params, stats[1], stats[2], posterior_draws, draws_seed)
    return res


def ensemble_kalman_smoother_pupil(markers_list, keypoint_names, tracker_name,
                                   state_transition_matrix, posterior_var=False,
                                   allow_missing=False, min_members=None, fit_on_device=False,
                                   posterior_draws=0, draws_seed=0):
    """IBL pupil smoother (eks/pupil_smoother.py:82-223).

    ``allow_missing=True``: a column whose ensemble average or variance is not
    finite (a NaN prediction of any member: a blink) is a missing observation;
    the model is fitted on the frames that are complete in every column, the
    smoother steps over the gaps (batch.smooth_gaps) and every frame of the
    output is finite.  The dict gains 'n_missing', the number of missing
    entries.  With ``min_members`` a column is missing only when fewer than
    that many members are finite (the ensemble over the finite ones).

    Returns {'markers_df': smoothed keypoints in the order top, right, bottom,
    left (NaN likelihood), 'latents_df': diameter, com_x, com_y}.  With
    ``posterior_var`` also 'posterior_var_df' (the markers layout, x / y holding
    the posterior variances) and 'latents_posterior_var_df' (diag(Vs)).

    ``fit_on_device=True``: the members go to the device once, the model comes
    from batch.fit_pupil + batch.pupil_params instead of the host fit, and the
    smoother reads the planes the fit wrote (batch.smooth_gaps); the dict has
    the same keys.  Without ``allow_missing`` a frame the device fit finds
    incomplete raises ValueError.

    ``posterior_draws=S``: also 'posterior_draws' (S, T, 8), joint posterior
    draws in the columns of the smoother's out (fit.PUPIL_KEYS), and
    'latents_posterior_draws' (S, T, 3) in the columns of latents_df, seeded
    by ``draws_seed``."""
    _check_min_members(min_members, allow_missing)
    stack = np.stack([np.stack([np.asarray(df[k], dtype=np.float64) for k in fit.PUPIL_KEYS], 1)
                      for df in markers_list])  # (E, T, 8)
    if fit_on_device:
        return _pupil_on_device(stack, keypoint_names, tracker_name, state_transition_matrix,
                                bool(posterior_var), allow_missing, min_members,
                                posterior_draws, draws_seed)
    yev, preds, ev = core.ensemble_handoff(stack, min_members=min_members)
    pv = bool(posterior_var)
    n_missing = None
    if allow_missing:
        model = fit.pupil_model(preds[_complete_frames(preds, ev)], state_transition_matrix)
        out, ms, *var_Vs, n_missing = _run_gaps_pupil(yev, model, pv)
    else:
        model = fit.pupil_model(preds, state_transition_matrix)
        out, ms, _, *var_Vs = _run_fused(stack, model, want_ms=True, yev=yev, want_var=pv,
                                         want_Vs=pv)
    var, Vs = var_Vs if pv else (None, None)
    res = _pupil_dfs(out, ms, model["mx"], model["my"], keypoint_names, tracker_name, var, Vs)
    if allow_missing:
        res['n_missing'] = n_missing
    if posterior_draws:
        params = batch.pack_params(model["m0"], model["S0"], model["A"], model["Q"], model["C"],
                                   model["offset"])
        _pupil_draws(res, yev, params, model["mx"], model["my"], posterior_draws, draws_seed)
    return res


def pupil_smoothing_sweep(markers_list, keypoint_names, tracker_name, diameter_s_grid,
                          com_s_grid, allow_missing=False, min_members=None,
                          fit_on_device=False):
    """The pupil smoother with its smoothing parameters chosen by likelihood.

    Every (diameter_s, com_s) pair of the grid defines a model
    (A = diag(d, c, c), Q = var (1 - A^2): eks/pupil_smoother.py:140-147);
    all candidates are scored in ONE filter-only batched call (the member
    predictions are shared, batch stride 0) by their innovation NLL, and the
    argmin is smoothed.  Returns ensemble_kalman_smoother_pupil's dict plus
    'nll' (len(diameter_s_grid), len(com_s_grid)) and 'best' (d, c).
    (The reference has no NLL loop: SURVEY.md §0; this is the build's.)

    ``allow_missing=True``: the candidates are fitted on the complete frames
    (they share C and offset and differ in A and Q), scored over the observed
    entries in one batch.nll_sweep_gaps call, and the argmin is smoothed
    through the gaps (ensemble_kalman_smoother_pupil(allow_missing=True));
    ``min_members`` as there.

    ``fit_on_device=True``: the members go to the device once and
    batch.pupil_sweep fits, scores, picks and smooths there (the gaps kernels,
    from the planes); the dict has the same keys.  Without ``allow_missing`` a
    frame the device fit finds incomplete raises ValueError."""
    _check_min_members(min_members, allow_missing)
    torch = _lib.require_gpu()
    stack = np.stack([np.stack([np.asarray(df[k], dtype=np.float64) for k in fit.PUPIL_KEYS], 1)
                      for df in markers_list])  # (E, T, 8)
    E, T, n = stack.shape
    if fit_on_device:
        sw = batch.pupil_sweep(_pupil_device_obs(stack, min_members), diameter_s_grid,
                               com_s_grid)
        _check_device_complete(sw["ncomplete"], T, allow_missing)
        stats = sw["stats"][0].cpu().numpy()
        res = _pupil_dfs(sw["out"][0].cpu().numpy(), sw["ms"][0].cpu().numpy(), stats[1],
                         stats[2], keypoint_names, tracker_name)
        if allow_missing:
            res["n_missing"] = T * n - int(sw["nobs"][0].item())
        res["nll"] = sw["nll"][:, 0].cpu().numpy().reshape(len(diameter_s_grid), len(com_s_grid))
        res["best"] = tuple(float(v) for v in sw["best"][0].cpu().numpy())
        return res
    if allow_missing:
        yev, preds, ev = core.ensemble_handoff(stack, min_members=min_members)
        ok = _complete_frames(preds, ev)
        grid = [(d, c) for d in diameter_s_grid for c in com_s_grid]
        models = [fit.pupil_model(preds[ok], np.diag([d, c, c])) for d, c in grid]
        stackp = lambda k: np.stack([m[k] for m in models])  # noqa: E731
        params = batch.pack_params(stackp("m0"), stackp("S0"), stackp("A"), stackp("Q"),
                                   stackp("C"), stackp("offset"))
        scores = batch.nll_sweep_gaps(yev, params, K=len(grid), n=n, r=3)["nll"][:, 0]
        scores = scores.cpu().numpy()
        best = grid[int(np.argmin(scores))]
        res = ensemble_kalman_smoother_pupil(markers_list, keypoint_names, tracker_name,
                                             np.diag([best[0], best[1], best[1]]),
                                             allow_missing=True, min_members=min_members)
        res["nll"] = scores.reshape(len(diameter_s_grid), len(com_s_grid))
        res["best"] = best
        return res
    preds, _ = core.ensemble_array(stack)
    grid = [(d, c) for d in diameter_s_grid for c in com_s_grid]
    models = [fit.pupil_model(preds, np.diag([d, c, c])) for d, c in grid]
    stackp = lambda k: np.stack([m[k] for m in models])  # noqa: E731
    params = batch.pack_params(stackp("m0"), stackp("S0"), stackp("A"), stackp("Q"),
                               stackp("C"), stackp("offset"))
    obs = torch.from_numpy(np.ascontiguousarray(stack)).to("cuda").permute(1, 0, 2).unsqueeze(0)
    flags = batch.model_flags(stackp("A"), stackp("C"), stackp("Q"))
    scores = batch.nll(obs.expand(len(grid), -1, -1, -1), params, n=n, r=3,
                       flags=flags).cpu().numpy()
    best = grid[int(np.argmin(scores))]
    res = ensemble_kalman_smoother_pupil(markers_list, keypoint_names, tracker_name,
                                         np.diag([best[0], best[1], best[1]]))
    res["nll"] = scores.reshape(len(diameter_s_grid), len(com_s_grid))
    res["best"] = best
    return res


def ensemble_kalman_smoother_single_view(markers_list, keypoint_ensemble, smooth_param,
                                         quantile_keep_pca=25, ensembling_mode="median",
                                         posterior_var=False, allow_missing=False,
                                         min_members=None, posterior_draws=0, draws_seed=0):
    """Single-view EKS for one keypoint (the reference
    snapshot has no single-view smoother).

    ``allow_missing=True``: a coordinate whose ensemble average or variance is
    not finite (a NaN prediction of any member) is a missing observation; the
    model is fitted on the complete frames, the smoother steps over the gaps
    (batch.smooth_gaps), 'nll' is the NLL over the observed entries and the
    dict gains 'n_missing'.  It needs a ``smooth_param``.  With
    ``min_members`` a coordinate is missing only when fewer than that many
    members are finite (the ensemble over the finite ones).

    markers_list: E DataFrames with '{keypoint}_x' / '{keypoint}_y' columns.
    Model: C = A = I2, m0 = 0, S0 = diag(var), Q = s cov(diff) over the
    low-variance frames, offset = their mean.  Returns {'markers_df',
    'nll'} with the reference's output format; with ``posterior_var`` also
    'posterior_var_df' (the same layout, x / y holding the posterior variances).
    ``smooth_param=None``: chosen by minimising the filter's NLL on the device
    (batch.select_smooth_param); the dict then gains 'smooth_param', and the
    frames equal those of a call with that value."""
    _check_min_members(min_members, allow_missing)
    keys = [f"{keypoint_ensemble}_x", f"{keypoint_ensemble}_y"]
    stack = np.stack([np.stack([np.asarray(df[k], dtype=np.float64) for k in keys], 1)
                      for df in markers_list])  # (E, T, 2)
    if allow_missing and smooth_param is None:
        raise ValueError("allow_missing=True needs a smooth_param: the likelihood sweep does "
                         "not step over gaps")
    yev, preds, ev = core.ensemble_handoff(stack, ensembling_mode, min_members=min_members)
    auto = smooth_param is None
    n_missing = None
    if allow_missing:
        ok = _complete_frames(preds, ev)
        model = fit.singleview_model(preds[ok], ev[ok], smooth_param, quantile_keep_pca)
        out, nll, var, n_missing = _run_gaps(yev, model, mode=ensembling_mode,
                                             want_var=bool(posterior_var))
        pv = [var]
    else:
        if auto:
            smooth_param = _auto_smooth_param(
                yev, fit.singleview_model(preds, ev, 1.0, quantile_keep_pca), ensembling_mode)
        model = fit.singleview_model(preds, ev, smooth_param, quantile_keep_pca)
        out, _, nll, *pv = _run_fused(stack, model, mode=ensembling_mode, want_nll=True, yev=yev,
                                      want_var=bool(posterior_var))
    nan = np.full(out.shape[0], np.nan)
    idx = make_dlc_pandas_index([keypoint_ensemble])
    df = pd.DataFrame(np.stack([out[:, 0], out[:, 1], nan], 1), columns=idx)
    res = {'markers_df': df, 'nll': nll}
    if allow_missing:
        res['n_missing'] = n_missing
    if auto:
        res['smooth_param'] = smooth_param
    if posterior_var:
        res['posterior_var_df'] = pd.DataFrame(np.stack([pv[0][:, 0], pv[0][:, 1], nan], 1),
                                               columns=idx)
    if posterior_draws:
        res['posterior_draws'] = _model_draws(yev, model, posterior_draws, draws_seed,
                                              ensembling_mode)
    return res




def _camera_dfs(out, keypoint_ensemble, camera_names):
    pdindex = make_dlc_pandas_index([keypoint_ensemble])
    nan = np.full(out.shape[0], np.nan)
    return {cam + "_df": pd.DataFrame(np.stack([out[:, 2 * c], out[:, 2 * c + 1], nan], axis=1),
                                      columns=pdindex)
            for c, cam in enumerate(camera_names)}


def eks_opti_smoother_multi_cam(markers_list_cameras, keypoint_ensemble, smooth_param,
                                quantile_keep_pca, camera_names, plot=False):
    """Multi-view PCA model + Newton forward filter, no backward pass
    (eks/multiview_pca_smoother.py:777-933): the model fit of
    ensemble_kalman_smoother_multi_cam, then kalman_newton_recursive with
    B = PCA axes, E = smooth_param * cov(diff(pcs)), output B q + means.
    ``plot`` is accepted for signature compatibility; the reference's plot
    branch reads a developer-local file, so nothing is plotted."""
    V = len(camera_names)
    if V < 2:
        raise ValueError("eks_opti_smoother_multi_cam needs at least two cameras")
    n_models = len(markers_list_cameras[0])
    cols = [np.stack([np.asarray(markers_list_cameras[c][e].to_numpy()[:, :2], dtype=np.float64)
                      for e in range(n_models)]) for c in range(V)]
    stack = np.concatenate(cols, axis=2)
    preds, ev = core.ensemble_array(stack)
    model = fit.multicam_model(preds, ev, smooth_param, quantile_keep_pca)
    q = kalman_newton_recursive(preds - model["offset"], model["m0"], model["S0"], model["A"],
                                model["C"], ev, model["Q"])
    out = q @ model["C"].T + model["offset"]
    return _camera_dfs(out, keypoint_ensemble, camera_names)


def eks_opti_smoother_pupil(markers_list, keypoint_names, tracker_name, state_transition_matrix,
                            plot=False):
    """IBL pupil model + Newton forward filter (eks/pupil_smoother.py:227-320).

    As in the reference, the transition matrix is fixed at A = 0.99 I (:260)
    and ``state_transition_matrix`` is ignored.  The reference's plot=False
    branch then uses an undefined variable; this returns what its plot=True
    branch and the committed data/misc/pupil-test/opti_eks_latents.csv hold:
    markers_df (C q + offsets, order top, right, bottom, left, NaN likelihood)
    and latents_df (diameter, com_x, com_y)."""
    stack = np.stack([np.stack([np.asarray(df[k], dtype=np.float64) for k in fit.PUPIL_KEYS], 1)
                      for df in markers_list])
    preds, ev = core.ensemble_array(stack)
    model = fit.pupil_model(preds, np.diag([0.99, 0.99, 0.99]))
    q = kalman_newton_recursive(preds - model["offset"], model["m0"], model["S0"], model["A"],
                                model["C"], ev, model["Q"])
    out = q @ model["C"].T + model["offset"]
    by_key = {k: out[:, j] for j, k in enumerate(fit.PUPIL_KEYS)}
    nan = np.full(out.shape[0], np.nan)
    cols = []
    for kp in ('top', 'right', 'bottom', 'left'):
        cols += [by_key[f'pupil_{kp}_r_x'], by_key[f'pupil_{kp}_r_y'], nan]
    markers_df = pd.DataFrame(np.stack(cols, 1), columns=make_dlc_pandas_index(keypoint_names))
    lat = np.stack([q[:, 0], q[:, 1] + model["mx"], q[:, 2] + model["my"]], 1)
    idx = pd.MultiIndex.from_arrays([[tracker_name] * 3, ['diameter', 'com_x', 'com_y']],
                                    names=('scorer', 'latent'))
    return {'markers_df': markers_df, 'latents_df': pd.DataFrame(lat, columns=idx)}


def ensemble_stacks(stacks, mode: str = "median"):
    """(K, E, T, n) member array (numpy or CUDA tensor) of K trajectories ->
    (members on the device, preds, vars (K, T, n)) CUDA float64, one
    eks_ensemble launch."""
    torch = _lib.require_gpu()
    if mode not in ("median", "mean"):
        raise ValueError(f"{mode} averaging not supported")
    K, E, T, n = stacks.shape
    if torch.is_tensor(stacks):
        d = stacks.to(device="cuda", dtype=torch.float64).contiguous()
    else:
        d = torch.from_numpy(np.ascontiguousarray(stacks, dtype=np.float64)).to("cuda")
    preds = torch.empty((K, T, n), dtype=torch.float64, device="cuda")
    var = torch.empty_like(preds)
    lib = _lib.load()
    _lib.check(lib.eks_ensemble(d.data_ptr(), _lib.EKS_F64, K, T, E, n, E * T * n, n, T * n, 1,
                                _lib.EKS_MEDIAN if mode == "median" else _lib.EKS_MEAN,
                                preds.data_ptr(), var.data_ptr(), _lib.stream_ptr()),
               "eks_ensemble")
    return d, preds, var


def multi_cam_batch(stacks, smooth_param, quantile_keep_pca, version: str = "standard"):
    """All keypoints of a multi-camera dataset in one launch each for the
    ensemble and the smoother (the reference loops keypoints one call at a
    time: scripts/multicam_example.py:106-150).

    stacks (K, E, T, 2V) camera-major (x, y) columns per keypoint.  The
    per-keypoint model fit is ensemble_kalman_smoother_multi_cam's
    (eks/multiview_pca_smoother.py:684-731); version "standard" fits every
    keypoint's model on the device (eks_fit, 1-8 cameras) and runs the fused
    RTS smoother (eks_smooth) on the fit's ensemble hand-off planes, "opti"
    fits on the host and runs the Newton filter (eks_newton_filter,
    :777-933).  Returns out (K, T, 2V) float64 numpy.

    ``smooth_param=None`` ("standard", up to 8 cameras): every keypoint's
    smoothing parameter is chosen by likelihood on the device
    (batch.select_smooth_param) from the fit's hand-off planes; returns
    (out, smooth_param (K,) float64 numpy)."""
    torch = _lib.require_gpu()
    stacks = np.asarray(stacks, dtype=np.float64)
    K, E, T, n = stacks.shape
    if n < 4:
        raise ValueError("multi-camera smoothing needs at least two cameras")
    auto = smooth_param is None
    if auto and (version == "opti" or n % 2 or n > 16):
        raise ValueError("smooth_param=None needs version 'standard' and at most 8 cameras")
    if version != "opti" and n % 2 == 0 and n <= 16:
        obs = torch.from_numpy(np.ascontiguousarray(stacks)).to("cuda").permute(0, 2, 1, 3)
        params, _, yev = batch.fit(obs, kind="multicam", n=n, r=3,
                                   smooth_param=1.0 if auto else smooth_param,
                                   quantile_keep=quantile_keep_pca, keep_yev=True)
        if auto:
            sel = batch.select_smooth_param(yev, params, n=n, r=3)
            params = sel["params"]
        res = batch.smooth(yev, params, n=n, r=3, flags=_lib.EKS_MODEL_A_IDENTITY, check=True)
        if auto:
            return res["out"].cpu().numpy(), sel["smooth_param"].cpu().numpy()
        return res["out"].cpu().numpy()
    d, preds_d, ev_d = ensemble_stacks(stacks)
    preds, ev = preds_d.cpu().numpy(), ev_d.cpu().numpy()
    models = [fit.multicam_model(preds[k], ev[k], smooth_param, quantile_keep_pca)
              for k in range(K)]
    st = lambda key: np.stack([m[key] for m in models])  # noqa: E731
    if version == "opti":
        y = preds_d - torch.from_numpy(st("offset")).to("cuda")[:, None, :]
        q, status = newton_filter_batch(y, ev_d, st("m0"), st("S0"), st("A"), st("C"), st("Q"))
        if bool((status != 0).any()):
            raise np.linalg.LinAlgError("Singular matrix (kalman_newton_recursive)")
        q = q.cpu().numpy()
        return np.einsum("ktr,knr->ktn", q, st("C")) + st("offset")[:, None, :]
    params = batch.pack_params(st("m0"), st("S0"), st("A"), st("Q"), st("C"), st("offset"))
    obs = d.permute(0, 2, 1, 3)  # (K, T, E, n) view
    res = batch.smooth(obs, params, n=n, r=3, flags=batch.model_flags(st("A"), st("C")),
                       check=True)
    return res["out"].cpu().numpy()


__all__ = ["ensemble_kalman_smoother_multi_cam", "ensemble_kalman_smoother_pupil",
           "ensemble_kalman_smoother_single_view", "pupil_smoothing_sweep",
           "eks_opti_smoother_multi_cam", "eks_opti_smoother_pupil", "multi_cam_batch",
           "ensemble_stacks", "TRACKER"]


# --------------------------------------------------------------------------
# F4: asynchronous two-camera paw smoother
# --------------------------------------------------------------------------
PAW_IMG_WIDTH = 128


def interp1d_linear(x, y, xq):
    """np.interp / interp1d(kind='linear') of every column of y (n, C) at xq,
    on the GPU (eks_interp1d); bit-identical to numpy.  CUDA tensors in and
    out (float64)."""
    torch = _lib.require_gpu()
    x = torch.as_tensor(x, dtype=torch.float64, device="cuda").contiguous()
    xq = torch.as_tensor(xq, dtype=torch.float64, device="cuda").contiguous()
    y = torch.as_tensor(y, dtype=torch.float64, device="cuda")
    n, C = y.shape
    out = torch.empty((len(xq), C), dtype=torch.float64, device="cuda")
    status = torch.zeros(len(xq), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().eks_interp1d(x.data_ptr(), n, y.data_ptr(), C, y.stride(0),
                                        y.stride(1), xq.data_ptr(), len(xq), out.data_ptr(),
                                        out.stride(0), out.stride(1), status.data_ptr(),
                                        _lib.stream_ptr()), "eks_interp1d")
    if bool((status != 0).any()):
        raise ValueError("A value in x_new is outside the interpolation range.")
    return out


def _paw_async(markers_list_left_cam, markers_list_right_cam, timestamps_left_cam,
               timestamps_right_cam, keypoint_names, smooth_param, quantile_keep_pca, opti):
    torch = _lib.require_gpu()
    tl = np.asarray(timestamps_left_cam, dtype=np.float64)
    tr = np.asarray(timestamps_right_cam, dtype=np.float64)
    # left-camera frames inside the right camera's time span, in the
    # reference's loop order (:86-90): skip early frames, stop at the first late one
    late = np.flatnonzero(tl > tr[-1])
    stop = late[0] if len(late) else len(tl)
    sel = np.flatnonzero(tl[:stop] >= tr[0])
    cols = [0, 1, 3, 4]  # (x, y) of paw 1 and paw 2, likelihoods skipped
    E = len(markers_list_left_cam)
    left = np.stack([m.to_numpy()[sel][:, cols] for m in markers_list_left_cam])   # (E, T, 4)
    right_raw = np.stack([m.to_numpy()[:, cols] for m in markers_list_right_cam])  # (E, Tr, 4)
    T = len(sel)
    # right camera resampled at the kept left timestamps, x flipped (:92-94)
    rr = torch.from_numpy(np.ascontiguousarray(right_raw.transpose(1, 0, 2).reshape(len(tr), -1)))
    right = interp1d_linear(tr, rr.cuda(), tl[sel]).reshape(T, E, 4).permute(1, 0, 2).contiguous()
    right[:, :, 0] = PAW_IMG_WIDTH - right[:, :, 0]
    right[:, :, 2] = PAW_IMG_WIDTH - right[:, :, 2]
    cams = torch.stack([torch.from_numpy(left).cuda(), right])                    # (2, E, T, 4)
    _, preds_d, ev_d = ensemble_stacks(cams)
    preds, ev = preds_d.cpu().numpy(), ev_d.cpu().numpy()
    models, paw_stacks = fit.paw_async_models(preds, ev, smooth_param, quantile_keep_pca)
    st = lambda key: np.stack([m[key] for m in models])  # noqa: E731
    n = 4
    if opti:
        y = np.stack([models[k]["y"] for k in range(2)])
        v = np.stack([models[k]["ev"] for k in range(2)])
        q, status = newton_filter_batch(y, v, st("m0"), st("S0"), st("A"), st("C"), st("Q"))
        if bool((status != 0).any()):
            raise np.linalg.LinAlgError("Singular matrix (kalman_newton_recursive)")
        out = np.einsum("ktr,knr->ktn", q.cpu().numpy(), st("C")) + st("offset")[:, None, :]
    else:
        # per-paw member stacks (left view x, y | right view x, y): the fused
        # smoother ensembles them again, bit-identically
        obs = torch.stack([torch.cat([cams[0][:, :, 2 * k:2 * k + 2], cams[1][:, :, 2 * k:2 * k + 2]],
                                     dim=2) for k in range(2)])                   # (2, E, T, 4)
        params = batch.pack_params(st("m0"), st("S0"), st("A"), st("Q"), st("C"), st("offset"))
        res = batch.smooth(obs.permute(0, 2, 1, 3), params, n=n, r=3,
                           flags=_lib.EKS_MODEL_A_IDENTITY, check=True)
        out = res["out"].cpu().numpy()
    lp, rp = out[0], out[1]  # paw 1 / paw 2: (left x, y, right x, y)
    nan = np.full(T, np.nan)
    idx = make_dlc_pandas_index(keypoint_names)
    df_left = pd.DataFrame(np.stack([lp[:, 0], lp[:, 1], nan, rp[:, 0], rp[:, 1], nan], 1),
                           columns=idx)
    # right view: paws swapped back and x flipped to the LP convention (:309-320)
    df_right = pd.DataFrame(np.stack([PAW_IMG_WIDTH - rp[:, 2], rp[:, 3], nan,
                                      PAW_IMG_WIDTH - lp[:, 2], lp[:, 3], nan], 1), columns=idx)
    return {'left_df': df_left, 'right_df': df_right}


def ensemble_kalman_smoother_paw_asynchronous(
        markers_list_left_cam, markers_list_right_cam, timestamps_left_cam,
        timestamps_right_cam, keypoint_names, smooth_param, quantile_keep_pca):
    """Two asynchronous cameras, two paws (eks/multiview_pca_smoother.py:34-322):
    the right camera is resampled at the left camera's timestamps (GPU linear
    interpolation, eks_interp1d), one 3-D PCA subspace is fitted on both paws'
    good frames, and both paws are smoothed in one batched eks_smooth call.
    Returns {'left_df', 'right_df'} in the reference's layout."""
    return _paw_async(markers_list_left_cam, markers_list_right_cam, timestamps_left_cam,
                      timestamps_right_cam, keypoint_names, smooth_param, quantile_keep_pca,
                      opti=False)


def eks_opti_smoother_paw_asynchronous(
        markers_list_left_cam, markers_list_right_cam, timestamps_left_cam,
        timestamps_right_cam, keypoint_names, smooth_param, quantile_keep_pca):
    """The same model with the Newton forward filter instead of the RTS
    smoother (eks/multiview_pca_smoother.py:325-574)."""
    return _paw_async(markers_list_left_cam, markers_list_right_cam, timestamps_left_cam,
                      timestamps_right_cam, keypoint_names, smooth_param, quantile_keep_pca,
                      opti=True)


__all__ += ["ensemble_kalman_smoother_paw_asynchronous", "eks_opti_smoother_paw_asynchronous",
            "interp1d_linear"]
