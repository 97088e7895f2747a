"""CPU-side checks of the ensemble over the valid members (eks_ensemble_gaps)
and of the fit from planes (eks_fit_gaps with EKS_YEV32 / EKS_YEV64 input):
symbols, argument errors before any launch, the torch operator's registration
and shapes -- no kernel is launched here -- and the numpy reference of
tests/ensemble_gaps_ref.py pinned against gaps_ref.ensemble on gap-free
members (equal: np.nanvar / np.nanmedian run np.var's / np.median's
arithmetic when nothing is NaN)."""
import ctypes
import inspect

import numpy as np
import pytest

import ensemble_gaps_ref as R
import gaps_ref as G
from eks_amd import _lib


def test_symbol_exported_and_bound():
    lib = _lib.load()
    assert "eks_ensemble_gaps" in _lib.header_symbols()
    assert "eks_ensemble_gaps" in _lib.SIGNATURES
    assert hasattr(lib, "eks_ensemble_gaps")
    assert lib.eks_version() >= 106


def _call(lib, obs=8, dtype=_lib.EKS_F32, B=3, T=100, E=5, n=2, mode=_lib.EKS_MEDIAN,
          min_members=3, yev=8, nvalid=None):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return lib.eks_ensemble_gaps(p(obs), dtype, B, T, E, n, 0, 0, 0, 0, mode, min_members, p(yev),
                                 p(nvalid), None)


def test_argument_errors_do_not_launch():
    lib = _lib.load()
    # (the pointers are never dereferenced: every call below fails validation)
    assert _call(lib, obs=None) == _lib.EKS_ERR_ARG and b"NULL" in lib.eks_last_error()
    assert _call(lib, yev=None) == _lib.EKS_ERR_ARG and b"NULL" in lib.eks_last_error()
    assert _call(lib, T=0) == _lib.EKS_ERR_ARG and lib.eks_last_error()
    assert _call(lib, E=0) == _lib.EKS_ERR_ARG and lib.eks_last_error()
    for dtype in (9, _lib.EKS_YEV32, _lib.EKS_YEV64):
        assert _call(lib, dtype=dtype) == _lib.EKS_ERR_ARG and b"dtype" in lib.eks_last_error()
    assert _call(lib, mode=7) == _lib.EKS_ERR_ARG and lib.eks_last_error()
    for mm in (0, -1, 6):
        assert _call(lib, min_members=mm) == _lib.EKS_ERR_ARG, mm
        assert b"min_members" in lib.eks_last_error()
    for n in (0, 65):
        assert _call(lib, n=n) == _lib.EKS_ERR_UNSUPPORTED, n
    big = lib.eks_max_members() + 1
    assert _call(lib, E=big, min_members=2) == _lib.EKS_ERR_UNSUPPORTED
    with pytest.raises(_lib.EksError):
        _lib.check(_call(lib, yev=None), "eks_ensemble_gaps")
    # no trajectories: nothing to do, nothing launched
    assert _call(lib, B=0) == _lib.EKS_OK
    assert _call(lib, B=0, n=64, E=lib.eks_max_members(), min_members=1) == _lib.EKS_OK


def _fit(lib, obs=8, dtype=_lib.EKS_YEV64, B=3, T=100, E=5, n=2, r=2, yev=None, status=8,
         ws_bytes=1 << 30):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return lib.eks_fit_gaps(p(obs), dtype, B, T, E, n, r, 0, 0, 0, 0, _lib.EKS_MEDIAN,
                            _lib.EKS_FIT_SINGLEVIEW, 0.01, 25.0, p(8), p(8), ws_bytes, p(status),
                            p(yev), None, None, None)


def test_fit_from_planes_argument_errors_do_not_launch():
    lib = _lib.load()
    for dtype in (_lib.EKS_YEV32, _lib.EKS_YEV64):
        # yev neither NULL nor obs
        assert _fit(lib, dtype=dtype, yev=16) == _lib.EKS_ERR_ARG
        assert b"yev" in lib.eks_last_error()
        # the other checks still come before any launch
        assert _fit(lib, dtype=dtype, obs=None) == _lib.EKS_ERR_ARG
        assert _fit(lib, dtype=dtype, status=None) == _lib.EKS_ERR_ARG
        assert _fit(lib, dtype=dtype, T=1) == _lib.EKS_ERR_ARG
        assert _fit(lib, dtype=dtype, n=3, r=3) == _lib.EKS_ERR_UNSUPPORTED
        assert _fit(lib, dtype=dtype, ws_bytes=8) == _lib.EKS_ERR_ARG
        assert b"workspace" in lib.eks_last_error()
        # yev NULL or obs, E and mode ignored: valid (no trajectories: no launch)
        assert _fit(lib, dtype=dtype, B=0) == _lib.EKS_OK
        assert _fit(lib, dtype=dtype, B=0, yev=8, E=0) == _lib.EKS_OK
    # members still need their own planes, and eks_fit takes no planes as input
    assert _fit(lib, dtype=_lib.EKS_F32, yev=None) == _lib.EKS_ERR_ARG
    p = ctypes.c_void_p
    assert lib.eks_fit(p(8), _lib.EKS_YEV64, 3, 100, 5, 2, 2, 0, 0, 0, 0, _lib.EKS_MEDIAN,
                       _lib.EKS_FIT_SINGLEVIEW, 0.01, 25.0, p(8), p(8), 1 << 30, p(8), None,
                       None) == _lib.EKS_ERR_ARG


def test_ensemble_gaps_op_registered_with_fake_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eks_amd.ops as ops
    assert "ensemble_gaps" in ops.OPS and hasattr(torch.ops.eks, "ensemble_gaps")
    dump = torch._C._dispatch_dump("eks::ensemble_gaps")
    assert "CUDA: registered at" in dump and "Meta: registered at" in dump and "CPU:" not in dump
    assert "torch_ops.cpp" in dump and ".py" not in dump
    lib = _lib.load()
    with FakeTensorMode():
        for dt, E, n, mode in [(torch.float32, 5, 8, "median"), (torch.float64, 4, 2, "mean"),
                               (torch.float32, 17, 12, "median")]:
            obs = torch.empty((3, 100, E, n), dtype=dt)
            yev, nvalid = torch.ops.eks.ensemble_gaps(obs, mode, 2)
            m = _lib.EKS_MEDIAN if mode == "median" else _lib.EKS_MEAN
            assert yev.dtype == torch.uint8
            assert yev.shape == (lib.eks_yev_bytes(3, 100, n, _lib.EKS_F64, E, m),)
            assert yev.numel() >= 2 * 3 * 100 * n * 8
            assert nvalid.shape == (100, n, 3) and nvalid.dtype == torch.uint8
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.eks.ensemble_gaps(torch.zeros((3, 100, 5, 2)), "median", 2)


def test_python_interfaces_take_the_option():
    from eks_amd import batch, core, smoothers
    sig = inspect.signature(batch.ensemble_gaps)
    assert list(sig.parameters) == ["obs", "n", "mode", "min_members", "want_nvalid", "keep_yev"]
    assert sig.parameters["min_members"].default is inspect.Parameter.empty
    assert inspect.signature(core.ensemble_handoff).parameters["min_members"].default is None
    for f in (smoothers.ensemble_kalman_smoother_single_view,
              smoothers.ensemble_kalman_smoother_multi_cam,
              smoothers.ensemble_kalman_smoother_pupil, smoothers.pupil_smoothing_sweep):
        assert inspect.signature(f).parameters["min_members"].default is None, f.__name__
    # the keyword is refused before anything touches the device
    with pytest.raises(ValueError, match="allow_missing"):
        smoothers.ensemble_kalman_smoother_single_view([], "kp", 1.0, min_members=3)
    with pytest.raises(ValueError, match="allow_missing"):
        smoothers.ensemble_kalman_smoother_multi_cam([], "kp", 1.0, 25, ["a", "b"], min_members=3)
    with pytest.raises(ValueError, match="allow_missing"):
        smoothers.ensemble_kalman_smoother_pupil([], [], "t", np.eye(3), min_members=3)
    with pytest.raises(ValueError, match="allow_missing"):
        smoothers.pupil_smoothing_sweep([], [], "t", [0.9], [0.9], min_members=3)


@pytest.mark.parametrize("mode", ["median", "mean"])
@pytest.mark.parametrize("E", [3, 4, 5, 8])
def test_reference_equals_the_all_members_ensemble_without_gaps(mode, E):
    st = G.members("mc", 2, 60, V=2, E=E, seed=E)
    for b in range(2):
        y0, e0 = G.ensemble(st[b], mode)
        y, ev, m = R.ensemble_valid(st[b], mode, E)
        assert (m == E).all()
        np.testing.assert_array_equal(y, y0)
        np.testing.assert_array_equal(ev, e0)


def test_reference_on_a_small_column():
    st = np.array([1.0, np.nan, 4.0, np.inf, 2.0, -np.inf]).reshape(6, 1)
    y, ev, m = R.ensemble_valid(st, "median", 3)
    assert m[0] == 3 and y[0] == 2.0
    np.testing.assert_allclose(ev[0], np.var([1.0, 4.0, 2.0]) / 3, rtol=1e-15)
    y, ev, m = R.ensemble_valid(st, "mean", 4)
    assert np.isnan(y[0]) and np.isnan(ev[0])
    y, ev, m = R.ensemble_valid(st[:4], "median", 1)   # two valid: the mean of both
    assert m[0] == 2 and y[0] == 2.5
