"""CPU-side checks of the model fit through missing observations
(eks_fit_gaps): symbols, the workspace query, argument errors before any
launch, the torch operator's registration and shapes.  No kernel is launched
here."""
import ctypes

import pytest

from eks_amd import _lib

NEW = ("eks_fit_gaps", "eks_fit_gaps_workspace_bytes")


def test_symbols_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/eks_hip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert lib.eks_version() >= 105


def test_workspace_query():
    lib = _lib.load()
    # at least the worst plane (one double per frame) and the frame mask
    assert lib.eks_fit_gaps_workspace_bytes(17, 1000, 2) >= 17 * 1000 * 8 + 17 * 16 * 8
    assert lib.eks_fit_gaps_workspace_bytes(3, 700, 16) >= 3 * 700 * 8 + 3 * 11 * 8
    for B, T, n in [(17, 1000, 3), (17, 1000, 1), (17, 1000, 18), (0, 1000, 2), (17, 0, 2)]:
        assert lib.eks_fit_gaps_workspace_bytes(B, T, n) == 0, (B, T, n)


def _call(lib, obs=8, dtype=_lib.EKS_F32, B=3, T=100, E=5, n=2, r=2, mode=_lib.EKS_MEDIAN,
          kind=_lib.EKS_FIT_SINGLEVIEW, q=25.0, params=8, ws=8, ws_bytes=1 << 30, status=8, yev=8):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return lib.eks_fit_gaps(p(obs), dtype, B, T, E, n, r, 0, 0, 0, 0, mode, kind, 0.01, q,
                            p(params), p(ws), ws_bytes, p(status), p(yev), None, None, None)


def test_argument_errors_do_not_launch():
    lib = _lib.load()
    MC = _lib.EKS_FIT_MULTICAM
    # (the pointers are never dereferenced: every call below fails validation)
    for missing in ("obs", "params", "ws", "status", "yev"):
        assert _call(lib, **{missing: None}) == _lib.EKS_ERR_ARG, missing
        assert b"eks_fit_gaps" in lib.eks_last_error() and b"NULL" in lib.eks_last_error()
    assert _call(lib, T=1) == _lib.EKS_ERR_ARG
    assert _call(lib, E=0) == _lib.EKS_ERR_ARG
    assert _call(lib, dtype=9) == _lib.EKS_ERR_ARG
    assert _call(lib, mode=7) == _lib.EKS_ERR_ARG
    assert _call(lib, kind=5) == _lib.EKS_ERR_ARG
    assert _call(lib, n=4, r=2) == _lib.EKS_ERR_ARG               # single view: r == n
    assert _call(lib, n=4, r=5, kind=MC) == _lib.EKS_ERR_ARG      # PCA: r <= n
    assert _call(lib, n=10, r=2, kind=MC) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, n=10, r=10) == _lib.EKS_ERR_UNSUPPORTED     # wide: the PCA model only
    assert _call(lib, n=3, r=3) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, n=18, r=3, kind=MC) == _lib.EKS_ERR_UNSUPPORTED
    for q in (-0.5, 100.5, float("nan")):
        assert _call(lib, q=q) == _lib.EKS_ERR_ARG, q
    assert _call(lib, E=lib.eks_max_members() + 1) == _lib.EKS_ERR_UNSUPPORTED
    need = lib.eks_fit_gaps_workspace_bytes(3, 100, 2)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == _lib.EKS_ERR_ARG
    assert b"workspace" in lib.eks_last_error()
    need = lib.eks_fit_gaps_workspace_bytes(3, 100, 12)
    assert _call(lib, n=12, r=3, kind=MC, ws_bytes=need - 1) == _lib.EKS_ERR_ARG
    with pytest.raises(_lib.EksError):
        _lib.check(_call(lib, status=None), "eks_fit_gaps")
    # no trajectories: nothing to do, nothing launched
    assert _call(lib, B=0) == _lib.EKS_OK


def test_fit_gaps_op_registered_with_fake_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eks_amd.ops as ops
    lib = _lib.load()
    assert "fit_gaps" in ops.OPS and hasattr(torch.ops.eks, "fit_gaps")
    dump = torch._C._dispatch_dump("eks::fit_gaps")
    assert "CUDA: registered at" in dump and "Meta: registered at" in dump and "CPU:" not in dump
    schema = str(torch.ops.eks.fit_gaps.default._schema)
    assert "str kind, int n, int r, float smooth_param, float quantile_keep, str mode" in schema
    with FakeTensorMode():
        for dtype, code, E, mode, n, r, kind in [
                (torch.float32, _lib.EKS_F32, 5, "median", 2, 2, "singleview"),
                (torch.float64, _lib.EKS_F64, 4, "mean", 12, 3, "multicam")]:
            obs = torch.empty((3, 100, E, n), dtype=dtype)
            params, st, yev, nc, nk = torch.ops.eks.fit_gaps(obs, kind, n, r, 0.01, 25.0, mode)
            assert params.shape == (3, lib.eks_param_len(n, r)) and params.dtype == torch.float64
            assert st.shape == (3,) and st.dtype == torch.int32
            m = _lib.EKS_MEDIAN if mode == "median" else _lib.EKS_MEAN
            assert yev.shape == (lib.eks_yev_bytes(3, 100, n, code, E, m),)
            assert yev.dtype == torch.uint8
            assert nc.shape == (3,) and nc.dtype == torch.int32
            assert nk.shape == (3,) and nk.dtype == torch.int32
    with pytest.raises((RuntimeError, NotImplementedError)):  # no CPU kernel
        torch.ops.eks.fit_gaps(torch.zeros((1, 4, 3, 2)), "singleview", 2, 2, 0.01, 25.0, "median")


def test_fit_gaps_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from eks_amd import batch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch.fit_gaps(torch.zeros((1, 4, 3, 2)), kind="singleview", n=2, r=2, smooth_param=0.01,
                       quantile_keep=25.0)
