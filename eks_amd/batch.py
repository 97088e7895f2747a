"""Batched, device-resident API of the fused smoother (the throughput path).

    out = smooth(obs, params, n=..., r=...)

``obs`` is a CUDA tensor viewed as (B, T, E, n) -- B trajectories (video x
keypoint), T frames, E ensemble members, n observed coordinates -- float32 or
float64, ANY strides (the kernel reads obs[b*sb + t*st + e*se + j*sj]).
For coalesced loads give it a layout whose trajectory axis is innermost, e.g.
a contiguous (T, E, n, B) buffer viewed with ``.permute(3, 0, 1, 2)``:
that is what ``bench.py`` and ``make_time_major`` use.

``params`` is the (B, P) float64 tensor from ``pack_params``.  Nothing is
copied to the host; everything is stream-ordered on the current stream.
"""
from __future__ import annotations

import collections

import numpy as np

from . import _lib

_WS = {}


class Yev:
    """Ensemble hand-off planes (y, ev) written by ``fit(..., keep_yev=True)``
    and accepted by ``smooth`` in place of the member predictions (the
    members are then read once for fit + smooth; include/eks_hip.h
    eks_yev_bytes).  ``buf`` is a uint8 CUDA tensor; ``code`` the EKS_YEV32 /
    EKS_YEV64 input code."""

    def __init__(self, buf, B: int, T: int, E: int, n: int, code: int, mode: str):
        self.buf, self.B, self.T, self.E, self.n, self.code, self.mode = buf, B, T, E, n, code, mode
        self.shape = (B, T, E, n)
        self.device = buf.device

    @staticmethod
    def layout(B: int, T: int, n: int, code: int):
        """(bytes of the y planes, byte offset of the ev planes, bytes in all)
        of the planes of B trajectories: T * n planes of B values of y (float32
        for EKS_YEV32, else float64), then from the next 256-byte boundary as
        many of ev (float64) -- include/eks_hip.h eks_yev_bytes."""
        ybytes = T * n * B * (4 if code == _lib.EKS_YEV32 else 8)
        ev_off = (ybytes + 255) // 256 * 256
        return ybytes, ev_off, ev_off + T * n * B * 8

    def planes(self):
        """The y and ev planes as (T, n, B) views of ``buf``."""
        import torch
        ybytes, ev_off, end = Yev.layout(self.B, self.T, self.n, self.code)
        ydt = torch.float32 if self.code == _lib.EKS_YEV32 else torch.float64
        shape = (self.T, self.n, self.B)
        return (self.buf[:ybytes].view(ydt).reshape(shape),
                self.buf[ev_off:end].view(torch.float64).reshape(shape))


def param_len(n: int, r: int) -> int:
    return r + 3 * r * r + n * r + n


def pack_params(m0, S0, A, Q, C, offset, device="cuda"):  # noqa: C901
    """Pack per-trajectory models into the (B, P) layout of eks_param_len:
    [m0 (r) | S0 (r*r) | A (r*r) | Q (r*r) | C (n*r) | offset (n)].
    Inputs are arrays/tensors with a leading B axis (or none, = shared)."""
    import torch

    def t(x):
        x = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x,
                            dtype=torch.float64)
        return x

    m0, S0, A, Q, C, offset = map(t, (m0, S0, A, Q, C, offset))
    r = m0.shape[-1]
    n = offset.shape[-1]
    parts = [m0, S0, A, Q, C, offset]
    B = max(p.shape[0] if p.dim() == d else 1 for p, d in zip(parts, (2, 3, 3, 3, 3, 2)))
    flat = []
    for p, d in zip(parts, (2, 3, 3, 3, 3, 2)):
        if p.dim() == d - 1:
            p = p.unsqueeze(0).expand(B, *p.shape)
        flat.append(p.reshape(B, -1))
    out = torch.cat(flat, dim=1).contiguous().to(device)
    assert out.shape[1] == param_len(n, r)
    return out


def workspace(nbytes: int, device=None, slot: str = "smooth"):
    """Cached device scratch buffer per (device, slot); reused by later calls
    on the same stream (the kernels are stream-ordered)."""
    import torch
    dev = torch.device("cuda") if device is None else torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), slot)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _WS[key] = buf
    return buf


# the pupil measurement matrix (eks/pupil_smoother.py:150-153; fit.PUPIL_C)
_PUPIL_C = np.array([[0, 1, 0], [-.5, 0, 1], [0, 1, 0], [.5, 0, 1],
                     [.5, 1, 0], [0, 0, 1], [-.5, 1, 0], [0, 0, 1]], dtype=np.float64)


def _diagonal(M) -> bool:
    off = ~np.eye(M.shape[-1], dtype=bool)
    return bool(np.all(M[..., off] == 0))


def model_flags(A, C, Q=None) -> int:
    """EKS_MODEL_* promise bits for host-side model arrays (A (.., r, r),
    C (.., n, r), Q (.., r, r)): A / C identity for every trajectory, or
    (with Q) the pupil structure -- C the pupil matrix, A and Q diagonal."""
    A = np.asarray(A)
    C = np.asarray(C)
    f = 0
    if A.shape[-1] == A.shape[-2] and np.all(A == np.eye(A.shape[-1])):
        f |= _lib.EKS_MODEL_A_IDENTITY
    if C.shape[-1] == C.shape[-2] and np.all(C == np.eye(C.shape[-1])):
        f |= _lib.EKS_MODEL_C_IDENTITY
    if (Q is not None and C.shape[-2:] == (8, 3) and np.all(C == _PUPIL_C)
            and _diagonal(A) and _diagonal(np.asarray(Q))):
        f |= _lib.EKS_MODEL_PUPIL
    return f


_FIT_KINDS = {"singleview": _lib.EKS_FIT_SINGLEVIEW, "multicam": _lib.EKS_FIT_MULTICAM}


def _mode_code(mode: str) -> int:
    if mode not in ("median", "mean"):
        raise ValueError(f"{mode} averaging not supported")
    return _lib.EKS_MEDIAN if mode == "median" else _lib.EKS_MEAN


# what an entry point passes for its input: eks_x(ptr, code, B, T, E, n, [r,] *strides, mode, ..)
_MemberIn = collections.namedtuple("_MemberIn", "ptr code B T E strides mode")


def _member_input(obs, n: int, mode, members_only: bool = False):
    """The input arguments of an entry point for a (B, T, E, n) member view of
    any strides or, unless ``members_only``, a ``Yev`` made in ``mode``: the
    pointer, the input code, B, T, E, the four strides (0 for planes) and the
    code of ``mode`` (None, unchecked, for an entry point without one).
    ``ptr`` is a bare address: the caller keeps ``obs`` (a temporary such as
    ``obs[rows]`` too) alive until the call that reads it has been launched.
    Needs no device: the checks are the same for CPU tensors."""
    import torch
    yev = isinstance(obs, Yev)
    if yev and members_only:
        raise TypeError("obs must be a member view: this entry point reads no hand-off planes")
    if not yev and obs.dim() != 4:
        raise ValueError("obs must be viewed as (B, T, E, n)")
    B, T, E, nn = obs.shape
    if nn != n:
        raise ValueError(f"obs has {nn} coordinates, expected n={n}")
    m = None if mode is None else _mode_code(mode)
    if yev:
        if mode is not None and mode != obs.mode:
            raise ValueError("the hand-off planes were made in another averaging mode")
        return _MemberIn(obs.buf.data_ptr(), obs.code, B, T, E, (0, 0, 0, 0), m)
    if obs.dtype not in (torch.float32, torch.float64):
        raise TypeError("obs must be float32 or float64")
    code = _lib.EKS_F32 if obs.dtype == torch.float32 else _lib.EKS_F64
    return _MemberIn(obs.data_ptr(), code, B, T, E, tuple(obs.stride()), m)


def _check_params(params, rows: int, n: int, r: int, ok: bool = True):
    """``params`` holds ``rows`` packed models: B, or (``ok``: K >= 0) K * B candidates."""
    import torch
    P = param_len(n, r)
    if not ok or params.shape != (rows, P) or params.dtype != torch.float64 \
            or not params.is_contiguous():
        raise ValueError(f"params must be a contiguous ({rows}, {P}) float64 tensor")


def _status_words(status, shape: tuple, dev):
    """The caller's status tensor if it has the entry point's form, a new one if None."""
    import torch
    if status is None:
        return torch.empty(shape, dtype=torch.int32, device=dev)
    if tuple(status.shape) != shape or status.dtype != torch.int32 or not status.is_contiguous():
        raise ValueError(f"status must be a contiguous {shape} int32 tensor")
    return status


def _yev_out(keep_yev, shape: tuple, code: int, mode: str, nbytes: int, dev):
    """The ``Yev`` an entry point writes its planes to: the buffer of
    ``keep_yev`` when that is a Yev large enough, else a new one; a Yev of
    another shape, code or mode gets a new header on its buffer."""
    import torch
    if isinstance(keep_yev, Yev) and keep_yev.buf.numel() >= nbytes:
        if (keep_yev.shape, keep_yev.code, keep_yev.mode) == (shape, code, mode):
            return keep_yev
        return Yev(keep_yev.buf, *shape, code, mode)
    return Yev(torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), *shape, code, mode)


def _raise_on_status(status, fn: str, errors: int) -> int:
    """Synchronises and raises on the bits of ``status`` that ``errors`` names:
    ValueError on EKS_STATUS_BAD_MODEL (a sweep's candidates) and on
    EKS_STATUS_SCAN (``fn`` has no path for an exact observation), LinAlgError
    on EKS_STATUS_SINGULAR.  Returns the bits that are set."""
    bits = status_bits(status)
    if bits & errors & _lib.EKS_STATUS_BAD_MODEL:
        raise ValueError("the candidates of a trajectory must share C and offset")
    if bits & errors & _lib.EKS_STATUS_SCAN:
        raise ValueError(f"an observed column with zero ensemble variance: {fn} does not serve it")
    if bits & errors & _lib.EKS_STATUS_SINGULAR:
        raise np.linalg.LinAlgError("Singular matrix")
    return bits


def _ptr(x):
    return x.data_ptr() if x is not None else None


def smooth_var(obs, params, *, n: int, r: int, want_Vs: bool = False, status=None, stream=None):
    """Posterior variances of ``smooth``'s output (eks_smooth_var): the
    covariance recursions alone, time-parallel on the device.

    Returns dict(var=(B,T,n) view of a time-major buffer with
    var[b,t,j] = c_j Vs_t c_j^T, Vs=(B,T,r,r) or None, status=(B,) int32).
    A trajectory with an exact observation (zero ensemble variance) is flagged
    EKS_STATUS_SCAN and NaN; ``smooth(..., want_var=True, check=True)``
    recomputes those."""
    torch = _lib.require_gpu()
    i = _member_input(obs, n, None)
    B, T = i.B, i.T
    _check_params(params, B, n, r)
    dev = obs.device
    var = torch.empty((T, B, n), dtype=torch.float64, device=dev).permute(1, 0, 2)
    Vs = torch.empty((B, T, r, r), dtype=torch.float64, device=dev) if want_Vs else None
    status = _status_words(status, (B,), dev)
    lib = _lib.load()
    ws = workspace(lib.eks_smooth_var_workspace_bytes(B, T, n, r), dev, slot="smooth_var")
    _lib.check(lib.eks_smooth_var(
        i.ptr, i.code, B, T, i.E, n, r, *i.strides, params.data_ptr(), var.data_ptr(),
        *var.stride(), _ptr(Vs), ws.data_ptr(), ws.numel(), status.data_ptr(),
        _lib.stream_ptr(stream)), "eks_smooth_var")
    return dict(var=var, Vs=Vs, status=status)


def _var_unfused(obs, params, rows, *, n: int, r: int, mode: str):
    """(var (k,T,n), Vs (k,T,r,r), status (k,)) of the trajectories ``rows``
    through the unfused kernels eks_ensemble -> eks_forward -> eks_backward and
    a projection: the path for exact observations, which have no W_t."""
    import torch
    lib = _lib.load()
    dev = obs.device
    k = int(rows.numel())
    T = obs.shape[1]
    f64 = dict(dtype=torch.float64, device=dev)
    if isinstance(obs, Yev):
        ev = obs.planes()[1][:, :, rows].permute(2, 0, 1).contiguous()
        y = torch.zeros_like(ev)  # the covariances do not depend on y
    else:
        sub = obs[rows]  # a gathered copy: it must outlive the launch that reads i.ptr
        i = _member_input(sub, n, mode)
        y = torch.empty((k, T, n), **f64)
        ev = torch.empty((k, T, n), **f64)
        _lib.check(lib.eks_ensemble(i.ptr, i.code, k, T, i.E, n, *i.strides, i.mode,
                                    y.data_ptr(), ev.data_ptr(), _lib.stream_ptr()), "eks_ensemble")
    p = params[rows]
    rr = r * r
    m0 = p[:, :r].contiguous()
    S0, A, Q = (p[:, r + i * rr:r + (i + 1) * rr].contiguous() for i in range(3))
    C = p[:, r + 3 * rr:r + 3 * rr + n * r].contiguous()
    mf = torch.empty((k, T, r), **f64)
    Vf = torch.empty((k, T, r, r), **f64)
    S = torch.empty((k, T, r, r), **f64)
    Vs = torch.empty((k, T, r, r), **f64)
    st1 = torch.empty((k,), dtype=torch.int32, device=dev)
    st2 = torch.empty((k,), dtype=torch.int32, device=dev)
    _lib.check(lib.eks_forward(k, T, n, r, y.data_ptr(), ev.data_ptr(), m0.data_ptr(),
                               S0.data_ptr(), A.data_ptr(), Q.data_ptr(), C.data_ptr(), None, 0,
                               mf.data_ptr(), Vf.data_ptr(), S.data_ptr(), None, st1.data_ptr(),
                               _lib.stream_ptr()), "eks_forward")
    _lib.check(lib.eks_backward(k, T, r, mf.data_ptr(), Vf.data_ptr(), S.data_ptr(), A.data_ptr(),
                                0, None, Vs.data_ptr(), None, st2.data_ptr(), _lib.stream_ptr()),
               "eks_backward")
    Cm = C.reshape(k, n, r)
    var = torch.einsum("bji,btik,bjk->btj", Cm, Vs, Cm)
    return var, Vs, st1 | st2


def smooth(obs, params, *, n: int, r: int, mode: str = "median", out=None, want_ms=False,
           want_nll=False, status=None, algo: int = 0, flags: int = 0, stream=None,
           check: bool = False, want_out: bool = True, want_var: bool = False,
           want_Vs: bool = False):
    """Fused ensemble -> forward -> backward -> projection for B trajectories.

    ``want_var`` / ``want_Vs``: the posterior variances of the output,
    ``var`` (B,T,n) with var[b,t,j] = c_j Vs_t c_j^T, and the smoothed
    covariances ``Vs`` (B,T,r,r), from the variance pass (``smooth_var``) run
    after the smoother on the same stream; its status is OR-ed into
    ``status``.  With ``check=True`` trajectories it flags EKS_STATUS_SCAN
    (exact observations) are recomputed through the unfused kernels.

    Returns dict(out=(B,T,n) view, ms=(B,T,r) or None, nll=(B,) or None,
    status=(B,) int32 bit mask, var, Vs (None unless asked for)).  ``out`` (if given) must be a (B, T, n)
    float64 CUDA tensor/view; by default a time-major buffer is allocated so
    that the kernel's stores are coalesced.  ``flags`` are EKS_MODEL_* promises
    (see ``model_flags``); ``algo`` 0 = automatic, 1 = sequential, 2 =
    time-parallel (three passes), 3 = time-parallel in two passes over the
    members, 4 = the runtime-n sequential kernel that every (r, n) without
    compiled kernels runs (include/eks_hip.h).  With ``check=True`` the call synchronises, raises on
    singular / mis-flagged trajectories and transparently re-runs with the
    sequential algorithm if the time-parallel scan reported a breakdown.
    """
    torch = _lib.require_gpu()
    i = _member_input(obs, n, mode)
    B, T = i.B, i.T
    _check_params(params, B, n, r)
    dev = obs.device
    if not want_out:  # filter only: NLL per trajectory, no backward pass
        want_nll, want_ms, out = True, False, None
    elif out is None:
        out = torch.empty((T, B, n), dtype=torch.float64, device=dev).permute(1, 0, 2)
    ms = torch.empty((B, T, r), dtype=torch.float64, device=dev) if want_ms else None
    nll = torch.empty((B,), dtype=torch.float64, device=dev) if want_nll else None
    status = _status_words(status, (B,), dev)
    lib = _lib.load()
    ws = workspace(lib.eks_smooth_workspace_bytes(B, T, n, r, i.E, algo), dev)
    ob, ot, oj = out.stride() if out is not None else (0, 0, 0)
    _lib.check(lib.eks_smooth(
        i.ptr, i.code, B, T, i.E, n, r, *i.strides, i.mode, params.data_ptr(), _ptr(out), ob, ot,
        oj, _ptr(ms), _ptr(nll), ws.data_ptr(), ws.numel(), flags, algo, status.data_ptr(),
        _lib.stream_ptr(stream)), "eks_smooth")
    res = dict(out=out, ms=ms, nll=nll, status=status, var=None, Vs=None)
    pv = None
    if want_var or want_Vs:  # the variance pass: own workspace slot, own status until checked
        pv = smooth_var(obs, params, n=n, r=r, want_Vs=want_Vs, stream=stream)
        res["var"] = pv["var"] if want_var else None
        res["Vs"] = pv["Vs"]
    if check:
        st_all = status_bits(status)
        if st_all & _lib.EKS_STATUS_BAD_MODEL:
            raise ValueError("a model_flags promise (A = I / C = I / pupil structure) does not hold")
        if st_all & _lib.EKS_STATUS_SCAN and algo != 1:
            return smooth(obs, params, n=n, r=r, mode=mode, out=out, want_ms=want_ms,
                          want_nll=want_nll, status=status, algo=1, flags=flags,
                          stream=stream, check=True, want_out=want_out, want_var=want_var,
                          want_Vs=want_Vs)
        if st_all & _lib.EKS_STATUS_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")
        if pv is not None and status_bits(pv["status"]) & _lib.EKS_STATUS_SCAN:
            # exact observations: only the flagged rows, through the unfused kernels
            rows = torch.nonzero(pv["status"] & _lib.EKS_STATUS_SCAN).flatten()
            var_r, Vs_r, st_r = _var_unfused(obs, params, rows, n=n, r=r, mode=mode)
            pv["var"][rows] = var_r
            if pv["Vs"] is not None:
                pv["Vs"][rows] = Vs_r
            pv["status"][rows] = st_r
        if pv is not None and status_bits(pv["status"]) & _lib.EKS_STATUS_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")
    if pv is not None:
        status |= pv["status"]
    return res


def fit(obs, *, kind: str, n: int, r: int, smooth_param: float, quantile_keep: float,
        mode: str = "median", check: bool = True, params=None, status=None, keep_yev=False):
    """Batched model fit on the device (eks_fit, F2): (B, T, E, n) member view
    -> (B, eks_param_len(n, r)) float64 parameter rows for ``smooth``.

    kind "singleview" (r == n) or "multicam" (PCA with r
    axes; eks/multiview_pca_smoother.py:684-731)."""
    torch = _lib.require_gpu()
    i = _member_input(obs, n, mode, members_only=True)
    B, T, E = i.B, i.T, i.E
    k = _FIT_KINDS[kind]
    lib = _lib.load()
    if params is None:
        params = torch.empty((B, param_len(n, r)), dtype=torch.float64, device=obs.device)
    else:
        _check_params(params, B, n, r)
    status = _status_words(status, (B,), obs.device)
    ws = workspace(lib.eks_fit_workspace_bytes(B, T, n), obs.device, slot="fit")
    yev = None
    if keep_yev:
        # a Yev object (reused when passed in) receives the ensemble planes
        yev = _yev_out(keep_yev, (B, T, E, n), lib.eks_yev_dtype(i.code, E, i.mode), mode,
                       lib.eks_yev_bytes(B, T, n, i.code, E, i.mode), obs.device)
    _lib.check(lib.eks_fit(i.ptr, i.code, B, T, E, n, r, *i.strides, i.mode, k,
                           float(smooth_param), float(quantile_keep), params.data_ptr(),
                           ws.data_ptr(), ws.numel(), status.data_ptr(),
                           yev.buf.data_ptr() if yev is not None else None, _lib.stream_ptr()),
               "eks_fit")
    if check and bool((status != 0).any()):
        raise ValueError("eks_fit: no frame passed the variance threshold (NaN ensemble "
                         "variances?)")
    if keep_yev:
        return params, status, yev
    return params, status


def fit_gaps(obs, *, kind: str, n: int, r: int, smooth_param: float, quantile_keep: float,
             mode: str = "median", check: bool = True, params=None, status=None, keep_yev=None):
    """``fit`` through missing observations (eks_fit_gaps).  A frame of a
    trajectory is complete iff the ensemble average and variance of all n
    columns are finite (``smooth_gaps``'s missing rule, per frame); the
    percentile is taken over the complete frames, the kept frames are the
    complete ones at or below it, and the model is ``fit``'s over the kept
    frames in frame order -- the host fit on ``preds[ok], ev[ok]``.

    Returns dict(params (B, P) float64, status (B,) int32, yev: the ``Yev``
    hand-off planes ``smooth_gaps`` / ``nll_sweep_gaps`` read in place of the
    members (the one passed as ``keep_yev`` when it is large enough),
    ncomplete (B,) int32 complete frames, nkept (B,) int32 kept frames).
    With ``check=True`` the call synchronises and raises ValueError when a
    trajectory has no complete frame (EKS_STATUS_SINGULAR in ``status``);
    ``check=False`` leaves ``status`` to the caller.

    ``obs`` may also be a ``Yev`` (from ``ensemble_gaps``, ``fit_gaps`` or
    ``fit``): the fit then reads its planes instead of members, ``mode`` is
    ignored, nothing is written to the planes and the returned ``yev`` is the
    one passed in (``keep_yev`` must be left unset)."""
    torch = _lib.require_gpu()
    from_yev = isinstance(obs, Yev)
    if from_yev:
        if keep_yev is not None:
            raise ValueError("keep_yev cannot be combined with a Yev input: the planes are read, "
                             "not written")
        mode = obs.mode
    i = _member_input(obs, n, mode)
    B, T, E = i.B, i.T, i.E
    k = _FIT_KINDS[kind]
    lib = _lib.load()
    dev = obs.device
    if params is None:
        params = torch.empty((B, param_len(n, r)), dtype=torch.float64, device=dev)
    else:
        _check_params(params, B, n, r)
    status = _status_words(status, (B,), dev)
    ncomplete = torch.empty((B,), dtype=torch.int32, device=dev)
    nkept = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = workspace(lib.eks_fit_gaps_workspace_bytes(B, T, n), dev, slot="fit_gaps")
    if from_yev:  # the planes are read: none are written
        yev, yptr = obs, None
    else:
        yev = _yev_out(keep_yev, (B, T, E, n), lib.eks_yev_dtype(i.code, E, i.mode), mode,
                       lib.eks_yev_bytes(B, T, n, i.code, E, i.mode), dev)
        yptr = yev.buf.data_ptr()
    _lib.check(lib.eks_fit_gaps(i.ptr, i.code, B, T, E, n, r, *i.strides, i.mode, k,
                                float(smooth_param), float(quantile_keep), params.data_ptr(),
                                ws.data_ptr(), ws.numel(), status.data_ptr(), yptr,
                                ncomplete.data_ptr(), nkept.data_ptr(), _lib.stream_ptr()),
               "eks_fit_gaps")
    if check and B > 0:
        bad = int((ncomplete == 0).sum().item())
        if bad:
            raise ValueError(f"eks_fit_gaps: {bad} of {B} trajectories have no complete frame")
        if bool((status != 0).any()):
            raise ValueError("eks_fit_gaps: no frame was kept")
    return dict(params=params, status=status, yev=yev, ncomplete=ncomplete, nkept=nkept)


def ensemble_gaps(obs, *, n: int, mode: str = "median", min_members: int,
                  want_nvalid: bool = False, keep_yev=None):
    """The ensemble over the valid (finite) members of every column
    (eks_ensemble_gaps): (B, T, E, n) member view, float32 or float64, any
    strides -> dict(yev, nvalid).  A column is missing (NaN planes) only when
    fewer than ``min_members`` of its E members are finite; otherwise y is the
    nanmedian / nanmean and ev the nanvar / m of the m valid ones.

    ``yev`` is a ``Yev`` (code EKS_YEV64) that ``smooth_gaps``,
    ``nll_sweep_gaps`` and ``fit_gaps`` read in place of the members (the
    buffer of ``keep_yev`` is reused when it is large enough); ``nvalid`` the
    uint8 (T, n, B) counts m with ``want_nvalid``, else None.  A single valid
    member has ev = 0, an exact observation to ``smooth_gaps``
    (EKS_STATUS_SCAN): use ``min_members >= 2``."""
    torch = _lib.require_gpu()
    i = _member_input(obs, n, mode, members_only=True)
    B, T, E = i.B, i.T, i.E
    min_members = int(min_members)
    if not 1 <= min_members <= E:
        raise ValueError(f"min_members={min_members} outside 1..E={E}")
    lib = _lib.load()
    dev = obs.device
    yev = _yev_out(keep_yev, (B, T, E, n), _lib.EKS_YEV64, mode,
                   lib.eks_yev_bytes(B, T, n, _lib.EKS_F64, E, i.mode), dev)
    nvalid = torch.empty((T, n, B), dtype=torch.uint8, device=dev) if want_nvalid else None
    _lib.check(lib.eks_ensemble_gaps(i.ptr, i.code, B, T, E, n, *i.strides, i.mode, min_members,
                                     yev.buf.data_ptr(), _ptr(nvalid) if B > 0 else None,
                                     _lib.stream_ptr()),
               "eks_ensemble_gaps")
    return dict(yev=yev, nvalid=nvalid)


def fit_pupil(obs, *, mode: str = "median", check: bool = True, keep_yev=None):
    """The statistics of the pupil model on the device (eks_fit_pupil): the
    mean and population variance of the pupil diameter and centre over the
    complete frames of every trajectory -- what ``fit.pupil_model`` derives
    from ``preds[ok]`` with ok the frames whose ensemble average and variance
    are finite in all 8 columns (``fit_gaps``'s rule; the reference's
    nanmedian rescue of partly observed frames is not reproduced).

    ``obs`` is a (B, T, E, 8) member view, float32 or float64, any strides,
    columns in ``fit.PUPIL_KEYS`` order (a column is missing under the
    all-members rule), or a ``Yev`` -- e.g. ``ensemble_gaps``'s, which is how a
    ``min_members`` rule comes in: the fit then reads its planes, ``mode`` is
    ignored, the returned ``yev`` is the one passed in and ``keep_yev`` must
    be left unset.

    ``keep_yev`` (member input): True, or a ``Yev`` whose buffer is reused
    when it is large enough, also writes the ensemble planes (EKS_YEV64,
    bit-identical to ``ensemble_gaps(min_members=E)``) that ``nll_sweep_gaps``
    and ``smooth_gaps`` read in place of the members; unset: none are written.

    Returns dict(stats (B, 6) float64 [mean diameter, mx, my, var diameter,
    var com_x, var com_y], ncomplete (B,) int32, status (B,) int32, yev).
    With ``check=True`` the call synchronises and raises ValueError when a
    trajectory has no complete frame (EKS_STATUS_SINGULAR, NaN stats)."""
    torch = _lib.require_gpu()
    n = 8
    from_yev = isinstance(obs, Yev)
    if from_yev:
        if keep_yev is not None:
            raise ValueError("keep_yev cannot be combined with a Yev input: the planes are read, "
                             "not written")
        mode = obs.mode
    i = _member_input(obs, n, mode)
    B, T, E = i.B, i.T, i.E
    lib = _lib.load()
    dev = obs.device
    stats = torch.empty((B, 6), dtype=torch.float64, device=dev)
    ncomplete = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = workspace(lib.eks_fit_pupil_workspace_bytes(B, T), dev, slot="fit_pupil")
    yev = obs if from_yev else None  # the planes are read: none are written
    if not from_yev and keep_yev is not None and keep_yev is not False:
        yev = _yev_out(keep_yev, (B, T, E, n), _lib.EKS_YEV64, mode,
                       lib.eks_yev_bytes(B, T, n, _lib.EKS_F64, E, i.mode), dev)
    yptr = None if from_yev or yev is None else yev.buf.data_ptr()
    if B > 0:
        _lib.check(lib.eks_fit_pupil(i.ptr, i.code, B, T, E, n, *i.strides, i.mode, stats.data_ptr(),
                                     ncomplete.data_ptr(), ws.data_ptr(), ws.numel(),
                                     status.data_ptr(), yptr, _lib.stream_ptr()),
                   "eks_fit_pupil")
        if check:
            bad = int((ncomplete == 0).sum().item())
            if bad:
                raise ValueError(f"eks_fit_pupil: {bad} of {B} trajectories have no complete "
                                 "frame")
    return dict(stats=stats, ncomplete=ncomplete, status=status, yev=yev)


def pupil_params(stats, a_diag):
    """``fit_pupil``'s statistics -> packed parameter rows of the pupil model
    (n = 8, r = 3; eks/pupil_smoother.py:140-153), a pure function of torch
    tensors on the device of ``stats`` like ``scale_q``.

    ``stats`` is (B, 6); ``a_diag`` the diagonals of K candidate transition
    matrices, (K, 3) shared by all trajectories or (K, B, 3).  Returns
    (K * B, P) float64 rows, row k * B + b candidate k of trajectory b (the
    ``nll_sweep_gaps`` convention): m0 = [mean d, 0, 0], S0 = diag(var),
    A = diag(a), Q = diag(var (1 - a^2)), C the pupil matrix,
    offset = [mx, my] x 4."""
    import torch
    stats = torch.as_tensor(stats, dtype=torch.float64)
    if stats.dim() != 2 or stats.shape[1] != 6:
        raise ValueError("stats must be (B, 6)")
    B = stats.shape[0]
    if not isinstance(a_diag, torch.Tensor):
        a_diag = np.array(a_diag, dtype=np.float64)  # (a copy: views may be read-only)
    a = torch.as_tensor(a_diag, dtype=torch.float64).to(stats.device)
    if a.dim() == 2:
        a = a.unsqueeze(1).expand(-1, B, -1)
    if a.dim() != 3 or a.shape[1:] != (B, 3):
        raise ValueError(f"a_diag must be (K, 3) or (K, {B}, 3)")
    K = a.shape[0]
    r, n = 3, 8
    var = stats[:, 3:6].unsqueeze(0).expand(K, B, 3)
    q = var * (1 - a ** 2)
    rows = torch.zeros((K, B, param_len(n, r)), dtype=torch.float64, device=stats.device)
    rows[:, :, 0] = stats[:, 0]
    s0, a0, q0, c0 = r, r + r * r, r + 2 * r * r, r + 3 * r * r
    for i in range(r):
        rows[:, :, s0 + i * (r + 1)] = var[:, :, i]
        rows[:, :, a0 + i * (r + 1)] = a[:, :, i]
        rows[:, :, q0 + i * (r + 1)] = q[:, :, i]
    rows[:, :, c0:c0 + n * r] = torch.as_tensor(_PUPIL_C.reshape(-1), device=stats.device)
    rows[:, :, c0 + n * r:] = stats[:, 1:3].repeat(1, 4)
    return rows.view(K * B, -1)


def pupil_sweep(obs, diameter_s_grid, com_s_grid, *, mode: str = "median", min_members=None,
                want_var: bool = False):
    """The pupil smoother with its two smoothing parameters chosen by
    likelihood, members -> fit -> sweep -> smooth without a member or a plane
    leaving the device.

    ``obs`` is a (B, T, E, 8) member view (or a ``Yev``).  With
    ``min_members`` the ensemble is ``ensemble_gaps``'s over the finite members
    of each column.  ``fit_pupil`` gives the statistics, ``pupil_params`` the
    K = len(diameter_s_grid) * len(com_s_grid) candidate rows per trajectory
    (A = diag(d, c, c), diameter-major), ``nll_sweep_gaps`` scores them over
    the observed entries, each trajectory takes its first minimum in grid
    order and ``smooth_gaps`` runs with the chosen rows.

    Returns dict(best (B, 2) the chosen (d, c), nll (K, B), params (B, P),
    stats, ncomplete, nobs (B,) observed entries, out (B, T, 8), ms (B, T, 3),
    var (B, T, 8) with ``want_var`` else None, status (B,) int32: the fit's,
    the sweep's (over the candidates) and the smoother's bits)."""
    torch = _lib.require_gpu()
    n, r = 8, 3
    if min_members is not None:
        if isinstance(obs, Yev):
            raise ValueError("min_members needs the members, not their planes")
        obs = ensemble_gaps(obs, n=n, mode=mode, min_members=min_members)["yev"]
    f = fit_pupil(obs, mode=mode, check=True, keep_yev=None if isinstance(obs, Yev) else True)
    yev = f["yev"]
    dev = yev.device
    B = yev.B
    d = torch.as_tensor(np.asarray(diameter_s_grid, dtype=np.float64), device=dev).flatten()
    c = torch.as_tensor(np.asarray(com_s_grid, dtype=np.float64), device=dev).flatten()
    if d.numel() < 1 or c.numel() < 1:
        raise ValueError("the grids must not be empty")
    grid = torch.cartesian_prod(d, c).reshape(-1, 2)  # diameter-major
    K = grid.shape[0]
    rows = pupil_params(f["stats"], torch.stack([grid[:, 0], grid[:, 1], grid[:, 1]], 1))
    sw = nll_sweep_gaps(yev, rows, K=K, n=n, r=r, mode=yev.mode)
    idx = torch.argmin(sw["nll"], dim=0)  # the first minimum in grid order
    params = rows.view(K, B, -1)[idx, torch.arange(B, device=dev)].contiguous()
    sm = smooth_gaps(yev, params, n=n, r=r, mode=yev.mode, want_ms=True, want_var=want_var,
                     check=True)
    status = f["status"] | sm["status"]
    for bit in (_lib.EKS_STATUS_SINGULAR, _lib.EKS_STATUS_BAD_MODEL, _lib.EKS_STATUS_SCAN):
        status = status | ((sw["status"] & bit) != 0).any(dim=0).to(torch.int32) * bit
    return dict(best=grid[idx], nll=sw["nll"], params=params, stats=f["stats"],
                ncomplete=f["ncomplete"], nobs=sm["nobs"], out=sm["out"], ms=sm["ms"],
                var=sm["var"], status=status)


def nll(obs, params, *, n: int, r: int, mode: str = "median", flags: int = 0, algo: int = 0,
        check: bool = True, status=None):
    """Filter-only pass: the innovation NLL of every
    trajectory / candidate model, no backward pass.  To score C candidate
    models of ONE trajectory, pass ``obs.expand(C, -1, -1, -1)`` (batch
    stride 0: the members are read once per candidate from the same memory)
    and C rows of params.  ``status`` (B,) int32 receives the per-trajectory
    status bits (check=False callers read it themselves)."""
    return smooth(obs, params, n=n, r=r, mode=mode, flags=flags, algo=algo, check=check,
                  want_out=False, status=status)["nll"]


def _yev_rows(obs: Yev, rows):
    """The hand-off planes of the trajectories ``rows`` as a Yev of their own."""
    import torch
    _, T, E, n = obs.shape
    k = int(rows.numel())
    nbytes = Yev.layout(k, T, n, obs.code)[2]
    sub = Yev(torch.zeros(nbytes, dtype=torch.uint8, device=obs.device), k, T, E, n, obs.code,
              obs.mode)
    for dst, src in zip(sub.planes(), obs.planes()):
        dst.copy_(src[:, :, rows])
    return sub


def nll_sweep(obs, params, *, K: int, n: int, r: int, mode: str = "median", check: bool = True,
              status=None, stream=None):
    """The innovation NLL of K candidate models for each of B trajectories in
    one call (eks_nll_sweep): the members (or the hand-off planes) are read
    and reduced once for all candidates, and a candidate costs r scalar
    updates per step whatever n is.

    ``params`` is (K * B, P): row k * B + b is candidate k of trajectory b.
    The candidates of a trajectory may differ in m0, S0, A and Q; C and
    offset must be equal.  Returns the (K, B) float64 NLLs; ``status`` (K, B)
    int32 receives the status bits.  With ``check=True`` the call
    synchronises: trajectories flagged EKS_STATUS_SCAN (an exact observation,
    a C without full column rank: NaN here) are recomputed with ``nll``, one
    call per candidate on the flagged trajectories; EKS_STATUS_BAD_MODEL (C or
    offset differ between candidates) raises ValueError, EKS_STATUS_SINGULAR
    LinAlgError."""
    torch = _lib.require_gpu()
    i = _member_input(obs, n, mode)
    B, T = i.B, i.T
    _check_params(params, K * B, n, r, ok=K >= 0)
    dev = obs.device
    out = torch.empty((K, B), dtype=torch.float64, device=dev)
    status = _status_words(status, (K, B), dev)
    lib = _lib.load()
    ws = workspace(lib.eks_nll_sweep_workspace_bytes(B, K, T, n, r), dev, slot="nll_sweep")
    _lib.check(lib.eks_nll_sweep(
        i.ptr, i.code, B, T, i.E, n, r, *i.strides, i.mode, params.data_ptr(), K, out.data_ptr(),
        ws.data_ptr(), ws.numel(), status.data_ptr(), _lib.stream_ptr(stream)), "eks_nll_sweep")
    if check and K * B > 0:
        bits = _raise_on_status(status, "eks_nll_sweep", _lib.EKS_STATUS_BAD_MODEL)
        if bits & _lib.EKS_STATUS_SCAN:
            rows = torch.nonzero(((status & _lib.EKS_STATUS_SCAN) != 0).any(dim=0)).flatten()
            sub = _yev_rows(obs, rows) if isinstance(obs, Yev) else obs[rows]
            cand = params.view(K, B, -1)
            for k in range(K):
                out[k, rows] = nll(sub, cand[k, rows].contiguous(), n=n, r=r, mode=mode,
                                   check=True)
            status[:, rows] &= ~_lib.EKS_STATUS_SCAN
        _raise_on_status(status, "eks_nll_sweep", _lib.EKS_STATUS_SINGULAR)
    return out


def smooth_gaps(obs, params, *, n: int, r: int, mode: str = "median", want_var: bool = False,
                want_Vs: bool = False, want_ms: bool = False, want_nll: bool = False,
                check: bool = False, status=None, stream=None):
    """Smoothing through missing observations (eks_smooth_gaps).  Column
    (t, j) of a trajectory is missing iff its ensemble average or variance is
    not finite (any NaN or +-inf member; a non-finite y or ev of a ``Yev``):
    it is left out of the update, and ``out`` / ``var`` are written for every
    (t, j), missing or not.  A caller who rejects a prediction writes NaN
    into it; there is no mask argument.

    Returns dict(out=(B,T,n) view of a time-major buffer, var (the same, or
    None), Vs=(B,T,r,r) or None, ms=(B,T,r) or None, nll=(B,) the innovation
    NLL over the observed entries or None, nobs=(B,) int32 observed entries,
    status=(B,) int32).  With ``check=True`` the call synchronises and raises
    LinAlgError on EKS_STATUS_SINGULAR and ValueError on EKS_STATUS_SCAN (an
    observed column with zero ensemble variance); there is no fallback path."""
    torch = _lib.require_gpu()
    i = _member_input(obs, n, mode)
    B, T = i.B, i.T
    _check_params(params, B, n, r)
    dev = obs.device
    f64 = dict(dtype=torch.float64, device=dev)
    out = torch.empty((T, B, n), **f64).permute(1, 0, 2)
    var = torch.empty((T, B, n), **f64).permute(1, 0, 2) if want_var else None
    Vs = torch.empty((B, T, r, r), **f64) if want_Vs else None
    ms = torch.empty((B, T, r), **f64) if want_ms else None
    nll_ = torch.empty((B,), **f64) if want_nll else None
    nobs = torch.empty((B,), dtype=torch.int32, device=dev)
    status = _status_words(status, (B,), dev)
    lib = _lib.load()
    ws = workspace(lib.eks_smooth_gaps_workspace_bytes(B, T, n, r), dev, slot="smooth_gaps")
    _lib.check(lib.eks_smooth_gaps(
        i.ptr, i.code, B, T, i.E, n, r, *i.strides, i.mode, params.data_ptr(), out.data_ptr(),
        *out.stride(), _ptr(var), _ptr(ms), _ptr(Vs), _ptr(nll_), nobs.data_ptr(), ws.data_ptr(),
        ws.numel(), status.data_ptr(), _lib.stream_ptr(stream)), "eks_smooth_gaps")
    if check and B > 0:
        _raise_on_status(status, "eks_smooth_gaps",
                         _lib.EKS_STATUS_SCAN | _lib.EKS_STATUS_SINGULAR)
    return dict(out=out, var=var, Vs=Vs, ms=ms, nll=nll_, nobs=nobs, status=status)


def draws_noise(B: int, S: int, T: int, r: int, seed: int, device="cuda", stream=None):
    """The noise z(b, s, t, i) that ``draws_gaps(seed=seed)`` generates in its
    kernels (eks_draws_noise; the generator's layout is in include/eks_hip.h):
    a (B, S, T, r) float64 view of a time-major (T, B, S, r) buffer."""
    torch = _lib.require_gpu()
    z = torch.empty((T, B, S, r), dtype=torch.float64, device=device).permute(1, 2, 0, 3)
    zb, zs, zt, _ = z.stride()
    _lib.check(_lib.load().eks_draws_noise(B, S, T, r, int(seed) & (2 ** 64 - 1), z.data_ptr(),
                                           zb, zs, zt, _lib.stream_ptr(stream)),
               "eks_draws_noise")
    return z


def _dummy_buffer(torch, dev):
    """A one-element device buffer for a required pointer that is never used."""
    return workspace(8, dev, slot="dummy")


def draws_gaps(obs, params, *, n: int, r: int, S=None, noise=None, seed=None,
               mode: str = "median", want_latent: bool = False, want_out: bool = True,
               want_var: bool = False, check: bool = False, status=None, stream=None):
    """S joint draws per trajectory from the smoothing posterior of
    ``smooth_gaps`` (eks_draws_gaps), same inputs and missing rule: consecutive
    frames of a draw are correlated as the posterior is, so a statistic that
    spans frames (speed, path length, time above a threshold) gets its error
    bar from the draws.

    Exactly one of ``noise`` -- a (B, S, T, r) float64 tensor of standard
    normals with a contiguous last axis, ``draws_noise``'s layout for coalesced
    loads -- and ``seed`` (with ``S``; the kernels generate the noise, none is
    allocated) is given.

    Returns dict(draws=(B,S,T,n) view of a (T,B,S,n) buffer, latent=(B,S,T,r)
    or None, out and var as ``smooth_gaps`` (None unless asked), status=(B,)
    int32).  A trajectory with a non-positive Cholesky pivot has
    EKS_STATUS_SINGULAR and NaN draws.  ``check=True`` as in ``smooth_gaps``."""
    if (noise is None) == (seed is None):
        raise ValueError("draws_gaps needs exactly one of noise and seed")
    torch = _lib.require_gpu()
    i = _member_input(obs, n, mode)
    B, T = i.B, i.T
    _check_params(params, B, n, r)
    if noise is not None:
        if noise.dim() != 4 or noise.shape[0] != B or noise.shape[2:] != (T, r) \
                or noise.dtype != torch.float64 or (r > 1 and noise.stride(3) != 1):
            raise ValueError(f"noise must be a ({B}, S, {T}, {r}) float64 tensor with a "
                             "contiguous last axis")
        if S is not None and S != noise.shape[1]:
            raise ValueError(f"S={S} but noise holds {noise.shape[1]} draws")
        S = noise.shape[1]
        zb, zs, zt, _ = noise.stride()
    else:
        if S is None or S < 0:
            raise ValueError("draws_gaps(seed=...) needs S >= 0")
        zb = zs = zt = 0
    dev = obs.device
    f64 = dict(dtype=torch.float64, device=dev)
    draws = torch.empty((T, B, S, n), **f64).permute(1, 2, 0, 3)
    # (S = 0: an empty tensor has no storage; the entry point wants a pointer it never touches)
    draws_ptr = draws.data_ptr() or _dummy_buffer(torch, dev).data_ptr()
    latent = torch.empty((B, S, T, r), **f64) if want_latent else None
    out = torch.empty((T, B, n), **f64).permute(1, 0, 2) if want_out or want_var else None
    var = torch.empty((T, B, n), **f64).permute(1, 0, 2) if want_var else None
    status = _status_words(status, (B,), dev)
    lib = _lib.load()
    ws = workspace(lib.eks_draws_gaps_workspace_bytes(B, S, T, n, r), dev, slot="draws_gaps")
    ob, ot, oj = out.stride() if out is not None else (0, 0, 0)
    _lib.check(lib.eks_draws_gaps(
        i.ptr, i.code, B, T, i.E, n, r, *i.strides, i.mode, params.data_ptr(),
        S, _ptr(noise), zb, zs, zt, (int(seed) & (2 ** 64 - 1)) if seed is not None else 0,
        draws_ptr, *draws.stride(), _ptr(latent), _ptr(out), ob, ot, oj, _ptr(var),
        ws.data_ptr(), ws.numel(), status.data_ptr(), _lib.stream_ptr(stream)), "eks_draws_gaps")
    if check and B > 0:
        _raise_on_status(status, "eks_draws_gaps",
                         _lib.EKS_STATUS_SCAN | _lib.EKS_STATUS_SINGULAR)
    return dict(draws=draws, latent=latent, out=out if want_out else None, var=var, status=status)


def nll_sweep_gaps(obs, params, *, K: int, n: int, r: int, mode: str = "median",
                   check: bool = True, status=None, stream=None):
    """``nll_sweep`` through missing observations (eks_nll_sweep_gaps): the
    innovation NLL over the observed entries of K candidate models for each of
    B trajectories in one call, with ``smooth_gaps``'s missing rule (column
    (t, j) is missing iff its ensemble average or variance is not finite).
    The members (or the hand-off planes) are read and reduced once for all
    candidates; a step with a camera out or nothing observed at all needs no
    special case.

    ``params`` is (K * B, P): row k * B + b is candidate k of trajectory b.
    The candidates of a trajectory may differ in m0, S0, A and Q; C and
    offset must be equal.  Returns dict(nll=(K, B) float64, nobs=(B,) int32
    observed entries, status=(K, B) int32).  A trajectory with nothing
    observed has NLL exactly 0.0 for every candidate.  With ``check=True``
    the call synchronises and raises ValueError on EKS_STATUS_BAD_MODEL (C or
    offset differ between candidates) and on EKS_STATUS_SCAN (an observed
    column with zero ensemble variance; there is no fallback path), and
    LinAlgError on EKS_STATUS_SINGULAR."""
    torch = _lib.require_gpu()
    i = _member_input(obs, n, mode)
    B, T = i.B, i.T
    _check_params(params, K * B, n, r, ok=K >= 0)
    dev = obs.device
    out = torch.empty((K, B), dtype=torch.float64, device=dev)
    nobs = torch.zeros((B,), dtype=torch.int32, device=dev)
    status = _status_words(status, (K, B), dev)
    lib = _lib.load()
    ws = workspace(lib.eks_nll_sweep_gaps_workspace_bytes(B, K, T, n, r), dev,
                   slot="nll_sweep_gaps")
    _lib.check(lib.eks_nll_sweep_gaps(
        i.ptr, i.code, B, T, i.E, n, r, *i.strides, i.mode, params.data_ptr(), K, out.data_ptr(),
        nobs.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(), _lib.stream_ptr(stream)),
        "eks_nll_sweep_gaps")
    if check and K * B > 0:
        _raise_on_status(status, "eks_nll_sweep_gaps", _lib.EKS_STATUS_BAD_MODEL
                         | _lib.EKS_STATUS_SCAN | _lib.EKS_STATUS_SINGULAR)
    return dict(nll=out, nobs=nobs, status=status)


DEFAULT_SWEEP_GRID = tuple(10.0 ** e for e in range(-4, 5))


def sweep_bracket(grid, best):
    """The next round's grid of a likelihood sweep (a pure function of torch
    tensors on any device): ``grid`` (B, K) ascending per row, ``best`` (B,)
    the index of each row's minimum -> (B, K): K log-spaced points from the
    best point's lower neighbour to its upper neighbour, both included,
    clipped at the row's ends (a best point at an end keeps that end)."""
    import torch
    K = grid.shape[1]
    lo = torch.gather(grid, 1, (best - 1).clamp(min=0).unsqueeze(1))
    hi = torch.gather(grid, 1, (best + 1).clamp(max=K - 1).unsqueeze(1))
    if K == 1:
        return lo.clone()
    frac = torch.arange(K, dtype=grid.dtype, device=grid.device) / (K - 1)
    new = lo * (hi / lo) ** frac
    new[:, 0] = lo[:, 0]
    new[:, -1] = hi[:, 0]
    return new


def scale_q(params, s, *, r: int):
    """params (B, P) rows -> (K, B, P) rows with Q scaled by s (K, B), on the
    device of ``params``."""
    K, B = s.shape
    rows = params.unsqueeze(0).repeat(K, 1, 1)
    q0 = r + 2 * r * r
    rows[:, :, q0:q0 + r * r] *= s.unsqueeze(2)
    return rows


def select_smooth_param(obs, params, *, n: int, r: int, mode: str = "median", grid=None,
                        refine: int = 2, allow_missing: bool = False):
    """The smoothing parameter of every trajectory chosen by likelihood on the
    device, as the reference's later versions do for ``smooth_param=None``.

    ``params`` holds B rows fitted with ``smooth_param = 1`` (Q = Q0).  Every
    round scores K candidates Q = s Q0 per trajectory in one ``nll_sweep``
    call (the K * B rows are built on the device by scaling the Q slice) and
    takes the per-trajectory argmin, ties to the smallest s; the next round
    lays K log-spaced points between the best point's two neighbours
    (``sweep_bracket``).  The default grid is 10 ** arange(-4, 5); after
    ``refine`` = 2 rounds its spacing is 10 ** (1 / 16).  A later round
    replaces the choice only where it lowers the NLL.

    ``allow_missing=True`` scores through ``nll_sweep_gaps``: the NLL over the
    observed entries, with ``smooth_gaps``'s missing rule.  A trajectory
    without any observation scores exactly 0 at every candidate: the tie goes
    to the grid's smallest s, and ``at_edge`` reports it.

    Returns dict(smooth_param (B,), nll (B,), at_edge (B,) bool: the choice is
    the grid's first or last point, params (B, P): the rows with Q scaled;
    with ``allow_missing=True`` also nobs (B,) int32, the observed entries)."""
    torch = _lib.require_gpu()
    B = params.shape[0]
    dev = params.device
    g0 = torch.as_tensor(DEFAULT_SWEEP_GRID if grid is None else np.asarray(grid, dtype=np.float64),
                         dtype=torch.float64, device=dev)
    if g0.dim() != 1 or g0.numel() < 1 or bool((g0[1:] <= g0[:-1]).any()) or bool((g0 <= 0).any()):
        raise ValueError("grid must be a positive, strictly ascending 1-D sequence")
    K = int(g0.numel())
    g = g0.unsqueeze(0).repeat(B, 1)  # (B, K)
    best_s = best_nll = nobs = None
    for rnd in range(int(refine) + 1):
        rows = scale_q(params, g.t().contiguous(), r=r).view(K * B, -1)
        if allow_missing:
            res = nll_sweep_gaps(obs, rows, K=K, n=n, r=r, mode=mode)
            scores, nobs = res["nll"].t(), res["nobs"]  # (B, K)
        else:
            scores = nll_sweep(obs, rows, K=K, n=n, r=r, mode=mode).t()  # (B, K)
        idx = torch.argmin(scores, dim=1)  # the first minimum: the smallest s
        s = torch.gather(g, 1, idx.unsqueeze(1))[:, 0]
        v = torch.gather(scores, 1, idx.unsqueeze(1))[:, 0]
        if best_s is None:
            best_s, best_nll = s, v
        else:
            better = v < best_nll
            best_s = torch.where(better, s, best_s)
            best_nll = torch.where(better, v, best_nll)
        g = sweep_bracket(g, idx)
    at_edge = (best_s == g0[0]) | (best_s == g0[-1])
    res = dict(smooth_param=best_s, nll=best_nll, at_edge=at_edge,
               params=scale_q(params, best_s.unsqueeze(0), r=r)[0])
    if allow_missing:
        res["nobs"] = nobs
    return res


def status_bits(status) -> int:
    """OR of all per-trajectory status words (synchronises)."""
    v = 0
    for bit in (_lib.EKS_STATUS_SINGULAR, _lib.EKS_STATUS_BAD_MODEL, _lib.EKS_STATUS_SCAN):
        if bool(((status & bit) != 0).any().item()):
            v |= bit
    return v


def make_time_major(stack_np, device="cuda", dtype=None):
    """(B, E, T, n) numpy array -> CUDA tensor stored (T, E, n, B), returned as
    the (B, T, E, n) view the kernels read with coalesced per-lane loads."""
    import torch
    a = np.asarray(stack_np)
    if dtype is not None:
        a = a.astype(dtype)
    tm = np.ascontiguousarray(np.transpose(a, (2, 1, 3, 0)))  # (T, E, n, B)
    d = torch.from_numpy(tm).to(device)
    return d.permute(3, 0, 1, 2)
