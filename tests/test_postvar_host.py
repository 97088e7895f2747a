"""CPU-side checks of the posterior-variance pass (eks_smooth_var): symbols,
workspace and chunk-length queries, argument errors before any launch, the
debug key, the torch operator's registration and shapes.  No kernel is
launched here."""
import ctypes

import pytest

from eks_amd import _lib

NEW = ("eks_smooth_var", "eks_smooth_var_workspace_bytes", "eks_smooth_var_chunk_len")


@pytest.fixture
def pvar_chunk():
    """eks_debug_set(EKS_DBG_PVAR_CHUNK, v) for one test, reset afterwards."""
    yield lambda v: _lib.debug_set(_lib.EKS_DBG_PVAR_CHUNK, v)
    _lib.debug_set(_lib.EKS_DBG_PVAR_CHUNK, 0)


def test_symbols_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/eks_hip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert _lib.EKS_DBG_PVAR_CHUNK == 7
    assert lib.eks_version() >= 101


def test_workspace_and_limits():
    lib = _lib.load()
    # W_t and P_t planes for every step (6 doubles each at r = 3) and the chunk arrays
    assert lib.eks_smooth_var_workspace_bytes(17, 1000, 8, 3) > 17 * 1000 * 6 * 8
    assert lib.eks_smooth_var_workspace_bytes(17, 1000, 2, 2) >= 2 * 17 * 1000 * 3 * 8
    # n does not enter once W_t is formed
    assert lib.eks_smooth_var_workspace_bytes(17, 1000, 64, 3) == \
        lib.eks_smooth_var_workspace_bytes(17, 1000, 8, 3)
    for n, r in [(8, 4), (65, 3), (2, 1), (0, 2)]:
        assert lib.eks_smooth_var_workspace_bytes(17, 1000, n, r) == 0, (n, r)
    assert lib.eks_smooth_var_workspace_bytes(0, 1000, 2, 2) == 0
    assert lib.eks_smooth_var_workspace_bytes(17, 0, 2, 2) == 0


def _call(lib, obs=8, dtype=_lib.EKS_F32, B=3, T=100, E=5, n=2, r=2, params=8, pvar=8, Vs=None,
          ws=8, ws_bytes=1 << 30, status=8):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return lib.eks_smooth_var(p(obs), dtype, B, T, E, n, r, 0, 0, 0, 0, p(params), p(pvar), 0, 0,
                              0, p(Vs), p(ws), ws_bytes, p(status), None)


def test_argument_errors_do_not_launch():
    lib = _lib.load()
    # (the pointers are never dereferenced: every call below fails validation)
    assert _call(lib, status=None) == _lib.EKS_ERR_ARG and b"NULL" in lib.eks_last_error()
    assert _call(lib, pvar=None) == _lib.EKS_ERR_ARG and b"NULL" in lib.eks_last_error()
    assert _call(lib, obs=None) == _lib.EKS_ERR_ARG
    assert _call(lib, params=None) == _lib.EKS_ERR_ARG
    assert _call(lib, T=0) == _lib.EKS_ERR_ARG
    assert _call(lib, E=0) == _lib.EKS_ERR_ARG
    assert _call(lib, dtype=9) == _lib.EKS_ERR_ARG
    assert _call(lib, r=4, n=8) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, r=3, n=65) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, E=lib.eks_max_members() + 1) == _lib.EKS_ERR_UNSUPPORTED
    # a workspace that is missing or too small
    assert _call(lib, ws=None) == _lib.EKS_ERR_ARG and b"workspace" in lib.eks_last_error()
    need = lib.eks_smooth_var_workspace_bytes(3, 100, 2, 2)
    assert _call(lib, ws_bytes=need - 1) == _lib.EKS_ERR_ARG
    with pytest.raises(_lib.EksError):
        _lib.check(_call(lib, status=None), "eks_smooth_var")
    # no trajectories: nothing to do, nothing launched
    assert _call(lib, B=0) == _lib.EKS_OK


def test_debug_key_forces_the_chunk_length(pvar_chunk):
    lib = _lib.load()
    auto = lib.eks_smooth_var_chunk_len(2, 2100, 2)
    assert auto % 8 == 0 and 8 <= auto < 2100
    ws_auto = lib.eks_smooth_var_workspace_bytes(2, 2100, 2, 2)
    assert pvar_chunk(8) == 0
    assert lib.eks_smooth_var_chunk_len(2, 2100, 2) == 8
    assert lib.eks_smooth_var_workspace_bytes(2, 2100, 2, 2) != ws_auto  # more chunks
    assert pvar_chunk(13) == 8  # the previous value comes back; rounded up to a multiple of 8
    assert lib.eks_smooth_var_chunk_len(2, 2100, 2) == 16
    assert pvar_chunk(136) == 13
    assert lib.eks_smooth_var_chunk_len(3, 131, 2) == 136  # >= T: one chunk
    assert pvar_chunk(10 ** 6) == 136
    assert lib.eks_smooth_var_chunk_len(3, 131, 2) == 136
    assert pvar_chunk(0) == 10 ** 6
    assert lib.eks_smooth_var_chunk_len(2, 2100, 2) == auto
    assert lib.eks_smooth_var_workspace_bytes(2, 2100, 2, 2) == ws_auto
    # a short trajectory is a single chunk on the 8-step grid
    assert lib.eks_smooth_var_chunk_len(4, 1, 2) == 8 and lib.eks_smooth_var_chunk_len(4, 2, 3) == 8
    assert lib.eks_smooth_var_chunk_len(4, 100, 4) == 0


def test_smooth_var_op_registered_with_fake_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eks_amd.ops as ops
    assert "smooth_var" in ops.OPS and hasattr(torch.ops.eks, "smooth_var")
    dump = torch._C._dispatch_dump("eks::smooth_var")
    assert "CUDA: registered at" in dump and "Meta: registered at" in dump and "CPU:" not in dump
    with FakeTensorMode():
        obs = torch.empty((3, 100, 5, 8), dtype=torch.float32)
        params = torch.empty((3, 62), dtype=torch.float64)  # eks_param_len(8, 3)
        var, Vs, st = torch.ops.eks.smooth_var(obs, params, 8, 3)
        assert var.shape == (3, 100, 8) and var.dtype == torch.float64
        assert Vs.shape == (3, 100, 3, 3) and Vs.dtype == torch.float64
        assert st.shape == (3,) and st.dtype == torch.int32
    with pytest.raises((RuntimeError, NotImplementedError)):  # no CPU kernel
        torch.ops.eks.smooth_var(torch.zeros((1, 4, 3, 2)), torch.zeros((1, 20), dtype=torch.float64),
                                 2, 2)


def test_want_var_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from eks_amd import batch
    obs = torch.zeros((1, 4, 3, 2))
    params = torch.zeros((1, 20), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch.smooth(obs, params, n=2, r=2, want_var=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch.smooth_var(obs, params, n=2, r=2)
