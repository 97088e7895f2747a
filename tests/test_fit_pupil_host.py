"""CPU-side checks of the pupil model fitted on the device (eks_fit_pupil):
symbols, the workspace query, argument errors before any launch, the torch
operator's registration and shapes, and batch.pupil_params against
pack_params of fit.pupil_model -- no kernel is launched here."""
import ctypes
import inspect

import numpy as np
import pytest

from eks_amd import _lib, batch, fit


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for name in ("eks_fit_pupil", "eks_fit_pupil_workspace_bytes"):
        assert name in _lib.header_symbols(), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.eks_version() >= 107


def test_workspace_query():
    lib = _lib.load()
    assert lib.eks_fit_pupil_workspace_bytes(1, 1_000_000) > 0
    assert lib.eks_fit_pupil_workspace_bytes(70, 97) > 0
    assert lib.eks_fit_pupil_workspace_bytes(0, 1000) == 0
    assert lib.eks_fit_pupil_workspace_bytes(-1, 1000) == 0
    assert lib.eks_fit_pupil_workspace_bytes(3, 1) == 0


def _call(lib, obs=8, dtype=_lib.EKS_F32, B=3, T=100, E=5, n=8, mode=_lib.EKS_MEDIAN, stats=8,
          ncomplete=8, ws=8, ws_bytes=None, status=8, yev=None):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    if ws_bytes is None:
        ws_bytes = lib.eks_fit_pupil_workspace_bytes(B, T)
    return lib.eks_fit_pupil(p(obs), dtype, B, T, E, n, 0, 0, 0, 0, mode, p(stats), p(ncomplete),
                             p(ws), ws_bytes, p(status), p(yev), None)


def test_argument_errors_do_not_launch():
    lib = _lib.load()
    # (the pointers are never dereferenced: every call below fails validation)
    for name in ("obs", "stats", "ncomplete", "ws", "status"):
        assert _call(lib, **{name: None}) == _lib.EKS_ERR_ARG, name
        msg = lib.eks_last_error()
        assert b"eks_fit_pupil" in msg and b"NULL" in msg, name
    assert _call(lib, n=2) == _lib.EKS_ERR_UNSUPPORTED and b"eks_fit_pupil" in lib.eks_last_error()
    assert _call(lib, T=1, ws_bytes=1 << 20) == _lib.EKS_ERR_ARG
    assert b"eks_fit_pupil" in lib.eks_last_error()
    assert _call(lib, E=0) == _lib.EKS_ERR_ARG and b"eks_fit_pupil" in lib.eks_last_error()
    big = lib.eks_max_members() + 1
    assert _call(lib, E=big) == _lib.EKS_ERR_UNSUPPORTED
    assert b"eks_fit_pupil" in lib.eks_last_error()
    assert _call(lib, dtype=9) == _lib.EKS_ERR_ARG
    assert b"eks_fit_pupil" in lib.eks_last_error() and b"dtype" in lib.eks_last_error()
    assert _call(lib, mode=7) == _lib.EKS_ERR_ARG and b"eks_fit_pupil" in lib.eks_last_error()
    for B, T in [(3, 100), (1, 1_000_000), (70, 97)]:
        need = lib.eks_fit_pupil_workspace_bytes(B, T)
        assert _call(lib, B=B, T=T, ws_bytes=need - 1) == _lib.EKS_ERR_ARG, (B, T)
        msg = lib.eks_last_error()
        assert b"eks_fit_pupil" in msg and b"workspace" in msg
    for dtype in (_lib.EKS_YEV32, _lib.EKS_YEV64):
        assert _call(lib, dtype=dtype, yev=16) == _lib.EKS_ERR_ARG
        assert b"eks_fit_pupil" in lib.eks_last_error() and b"yev" in lib.eks_last_error()
        # the other checks still come first; E and mode are ignored with planes
        assert _call(lib, dtype=dtype, n=2) == _lib.EKS_ERR_UNSUPPORTED
        assert _call(lib, dtype=dtype, B=0, E=0, mode=7) == _lib.EKS_OK
    with pytest.raises(_lib.EksError, match="eks_fit_pupil"):
        _lib.check(_call(lib, obs=None), "eks_fit_pupil")
    # no trajectories: nothing to do, nothing launched
    assert _call(lib, B=0) == _lib.EKS_OK
    assert _call(lib, B=0, yev=8) == _lib.EKS_OK


def test_fit_pupil_op_registered_with_fake_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eks_amd.ops as ops
    assert "fit_pupil" in ops.OPS and hasattr(torch.ops.eks, "fit_pupil")
    dump = torch._C._dispatch_dump("eks::fit_pupil")
    assert "CUDA: registered at" in dump and "Meta: registered at" in dump and "CPU:" not in dump
    assert "torch_ops.cpp" in dump and ".py" not in dump
    lib = _lib.load()
    with FakeTensorMode():
        for dt, B, T, E, mode in [(torch.float32, 3, 100, 5, "median"),
                                  (torch.float64, 1, 4099, 2, "mean"),
                                  (torch.float32, 70, 97, 8, "median")]:
            obs = torch.empty((B, T, E, 8), dtype=dt)
            stats, ncomplete, status, yev = torch.ops.eks.fit_pupil(obs, mode)
            m = _lib.EKS_MEDIAN if mode == "median" else _lib.EKS_MEAN
            assert stats.shape == (B, 6) and stats.dtype == torch.float64
            assert ncomplete.shape == (B,) and ncomplete.dtype == torch.int32
            assert status.shape == (B,) and status.dtype == torch.int32
            assert yev.dtype == torch.uint8
            assert yev.shape == (lib.eks_yev_bytes(B, T, 8, _lib.EKS_F64, E, m),)
            assert yev.numel() >= 2 * B * T * 8 * 8
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.eks.fit_pupil(torch.zeros((3, 100, 5, 8)), "median")


def test_python_interfaces():
    from eks_amd import smoothers
    sig = inspect.signature(batch.fit_pupil)
    assert list(sig.parameters) == ["obs", "mode", "check", "keep_yev"]
    assert sig.parameters["mode"].default == "median" and sig.parameters["check"].default is True
    assert list(inspect.signature(batch.pupil_params).parameters) == ["stats", "a_diag"]
    sig = inspect.signature(batch.pupil_sweep)
    assert list(sig.parameters) == ["obs", "diameter_s_grid", "com_s_grid", "mode", "min_members",
                                    "want_var"]
    for f in (smoothers.ensemble_kalman_smoother_pupil, smoothers.pupil_smoothing_sweep):
        assert inspect.signature(f).parameters["fit_on_device"].default is False, f.__name__


def _models(B, seed=0):
    """B host-fitted pupil models' statistics (B, 6) and the (T, 8) data."""
    from eks_amd import synthetic
    rng = np.random.default_rng(seed)
    preds = [np.median(synthetic.pupil_obs(rng, 5, 300).astype(np.float64), axis=0)
             for _ in range(B)]
    stats = []
    for p in preds:
        m = fit.pupil_model(p, np.eye(3))
        stats.append([m["m0"][0], m["mx"], m["my"], *np.diag(m["S0"])])
    return np.array(stats), preds


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("per_trajectory", [False, True])
def test_pupil_params_equals_pack_params_of_the_host_model(K, per_trajectory):
    import torch
    B = 3
    stats, preds = _models(B)
    rng = np.random.default_rng(K)
    a = rng.uniform(0.9, 0.9999, size=(K, B, 3) if per_trajectory else (K, 3))
    rows = batch.pupil_params(torch.from_numpy(stats), torch.from_numpy(a))
    assert rows.shape == (K * B, batch.param_len(8, 3)) and rows.dtype == torch.float64
    assert rows.device.type == "cpu"
    for k in range(K):
        for b in range(B):
            ab = a[k, b] if per_trajectory else a[k]
            m = fit.pupil_model(preds[b], np.diag(ab))
            want = batch.pack_params(m["m0"], m["S0"], m["A"], m["Q"], m["C"], m["offset"],
                                     device="cpu")
            assert want.shape == (1, rows.shape[1])
            np.testing.assert_array_equal(rows[k * B + b].numpy(), want[0].numpy())
    with pytest.raises(ValueError):
        batch.pupil_params(torch.from_numpy(stats), torch.zeros((K, B + 1, 3)))
    with pytest.raises(ValueError):
        batch.pupil_params(torch.zeros((B, 5)), torch.zeros((K, 3)))
