"""CPU-side checks of the gap-aware likelihood sweep (eks_nll_sweep_gaps):
symbols, workspace and chunk-length queries, argument errors before any
launch, the debug key, the torch operator's registration and shapes, the
keywords of the wrappers -- no kernel is launched here -- and a numpy model of
the chunked sweep (gaps_sweep_data.chunked_sweep) pinned against
gaps_ref.dense for every candidate.

The conditions test_gpu_gaps_sweep.py relies on are asserted here on the
shared inputs: every reference NLL finite, every argmin over SCALES interior
and separated from the second best by a relative gap >= 1e-4 (five orders
above the GPU test's 1e-9), and |NLL| / nobs >= 1, so that a relative bound on
the NLL is a bound per observed entry."""
import ctypes

import numpy as np
import pytest

import gaps_ref as G
import gaps_sweep_data as S
from eks_amd import _lib

NEW = ("eks_nll_sweep_gaps", "eks_nll_sweep_gaps_workspace_bytes", "eks_nll_sweep_gaps_chunk_len")
NLL_RTOL = 1e-11
MIN_GAP = 1e-4


@pytest.fixture
def gs_chunk():
    """eks_debug_set(EKS_DBG_GAPS_SWEEP_CHUNK, v) for one test, reset afterwards."""
    yield lambda v: _lib.debug_set(_lib.EKS_DBG_GAPS_SWEEP_CHUNK, v)
    _lib.debug_set(_lib.EKS_DBG_GAPS_SWEEP_CHUNK, 0)


def test_symbols_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/eks_hip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert _lib.EKS_DBG_GAPS_SWEEP_CHUNK == 10
    assert lib.eks_version() >= 104


def test_workspace_and_limits():
    lib = _lib.load()
    ws = lib.eks_nll_sweep_gaps_workspace_bytes
    # W_t (Sym), w_t (r) and kappa_t planes for every step: 6 doubles at r = 2, 10 at r = 3
    assert ws(17, 7, 1000, 2, 2) >= 1000 * 17 * 6 * 8
    assert ws(17, 7, 1000, 8, 3) >= 1000 * 17 * 10 * 8
    # n does not enter once W_t, w_t and kappa_t are formed
    assert ws(17, 7, 1000, 64, 3) == ws(17, 7, 1000, 8, 3)
    assert ws(17, 7, 1000, 10, 2) == ws(17, 7, 1000, 2, 2)
    # the chunk arrays have K * B rows
    assert ws(17, 1, 1000, 2, 2) < ws(17, 7, 1000, 2, 2) < ws(17, 64, 1000, 2, 2)
    for n, r in [(8, 4), (65, 3), (2, 1), (0, 2)]:
        assert ws(17, 7, 1000, n, r) == 0, (n, r)
    assert ws(0, 7, 1000, 2, 2) == 0
    assert ws(17, 0, 1000, 2, 2) == 0
    assert ws(17, 7, 0, 2, 2) == 0
    assert ws(1 << 20, 1 << 9, 10, 2, 2) == 0  # K * B > 2^28 rows
    assert lib.eks_nll_sweep_gaps_chunk_len(17, 7, 1000, 4) == 0
    assert lib.eks_nll_sweep_gaps_chunk_len(1 << 20, 1 << 9, 10, 2) == 0


def _call(lib, obs=8, dtype=_lib.EKS_F32, B=3, T=100, E=5, n=2, r=2, mode=_lib.EKS_MEDIAN,
          params=8, K=7, nll=8, nobs=8, ws=8, ws_bytes=1 << 30, status=8):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return lib.eks_nll_sweep_gaps(p(obs), dtype, B, T, E, n, r, 0, 0, 0, 0, mode, p(params), K,
                                  p(nll), p(nobs), p(ws), ws_bytes, p(status), None)


def test_argument_errors_do_not_launch():
    lib = _lib.load()
    # (the pointers are never dereferenced: every call below fails validation)
    assert _call(lib, status=None) == _lib.EKS_ERR_ARG and b"NULL" in lib.eks_last_error()
    assert _call(lib, nll=None) == _lib.EKS_ERR_ARG and b"NULL" in lib.eks_last_error()
    assert _call(lib, obs=None) == _lib.EKS_ERR_ARG
    assert _call(lib, params=None) == _lib.EKS_ERR_ARG
    assert _call(lib, T=0) == _lib.EKS_ERR_ARG
    assert _call(lib, E=0) == _lib.EKS_ERR_ARG
    assert _call(lib, K=-1) == _lib.EKS_ERR_ARG
    assert _call(lib, dtype=9) == _lib.EKS_ERR_ARG
    assert _call(lib, mode=7) == _lib.EKS_ERR_ARG
    assert _call(lib, r=4, n=8) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, r=3, n=65) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, E=lib.eks_max_members() + 1) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, B=1 << 20, K=1 << 9) == _lib.EKS_ERR_UNSUPPORTED
    assert b"2^28" in lib.eks_last_error()
    # a workspace that is missing or too small
    assert _call(lib, ws=None) == _lib.EKS_ERR_ARG and b"workspace" in lib.eks_last_error()
    need = lib.eks_nll_sweep_gaps_workspace_bytes(3, 7, 100, 2, 2)
    assert _call(lib, ws_bytes=need - 1) == _lib.EKS_ERR_ARG
    with pytest.raises(_lib.EksError):
        _lib.check(_call(lib, status=None), "eks_nll_sweep_gaps")
    # no trajectories or no candidates: nothing to do, nothing launched
    assert _call(lib, B=0) == _lib.EKS_OK
    assert _call(lib, K=0) == _lib.EKS_OK


def test_debug_key_forces_the_chunk_length(gs_chunk):
    lib = _lib.load()
    cl = lib.eks_nll_sweep_gaps_chunk_len
    ws = lib.eks_nll_sweep_gaps_workspace_bytes
    auto = cl(2, 7, 2100, 2)
    assert auto % 8 == 0 and 8 <= auto < 2100
    ws_auto = ws(2, 7, 2100, 2, 2)
    others = (lib.eks_nll_sweep_chunk_len(2, 7, 2100, 2), lib.eks_smooth_gaps_chunk_len(2, 2100, 2),
              lib.eks_smooth_var_chunk_len(2, 2100, 2))
    assert gs_chunk(8) == 0
    assert cl(2, 7, 2100, 2) == 8
    assert ws(2, 7, 2100, 2, 2) != ws_auto  # more chunks
    # the other passes' lengths are their own keys'
    assert others == (lib.eks_nll_sweep_chunk_len(2, 7, 2100, 2),
                      lib.eks_smooth_gaps_chunk_len(2, 2100, 2),
                      lib.eks_smooth_var_chunk_len(2, 2100, 2))
    assert gs_chunk(13) == 8  # the previous value comes back; rounded up to a multiple of 8
    assert cl(2, 7, 2100, 2) == 16
    assert gs_chunk(136) == 13
    assert cl(3, 7, 131, 2) == 136  # >= T: one chunk
    assert gs_chunk(10 ** 6) == 136
    assert cl(3, 7, 131, 2) == 136
    assert gs_chunk(0) == 10 ** 6
    assert cl(2, 7, 2100, 2) == auto
    assert ws(2, 7, 2100, 2, 2) == ws_auto
    for key in (_lib.EKS_DBG_SWEEP_CHUNK, _lib.EKS_DBG_GAPS_CHUNK, _lib.EKS_DBG_PVAR_CHUNK):
        _lib.debug_set(key, 8)
        try:
            assert cl(2, 7, 2100, 2) == auto
        finally:
            _lib.debug_set(key, 0)
    # a short trajectory is a single chunk on the 8-step grid
    assert cl(4, 7, 1, 2) == 8
    assert cl(4, 7, 2, 3) == 8


def test_op_registered_with_fake_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eks_amd.ops as ops
    assert "nll_sweep_gaps" in ops.OPS and hasattr(torch.ops.eks, "nll_sweep_gaps")
    dump = torch._C._dispatch_dump("eks::nll_sweep_gaps")
    assert "CUDA: registered at" in dump and "Meta: registered at" in dump and "CPU:" not in dump
    with FakeTensorMode():
        obs = torch.empty((3, 100, 5, 8), dtype=torch.float32)
        params = torch.empty((21, 62), dtype=torch.float64)  # K * B rows of eks_param_len(8, 3)
        nll, nobs, st = torch.ops.eks.nll_sweep_gaps(obs, params, 7, 8, 3, "median")
        assert nll.shape == (7, 3) and nll.dtype == torch.float64
        assert nobs.shape == (3,) and nobs.dtype == torch.int32
        assert st.shape == (7, 3) and st.dtype == torch.int32
    with pytest.raises((RuntimeError, NotImplementedError)):  # no CPU kernel
        torch.ops.eks.nll_sweep_gaps(torch.zeros((1, 4, 3, 2)),
                                     torch.zeros((2, 20), dtype=torch.float64), 2, 2, 2, "median")


def test_nll_sweep_gaps_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from eks_amd import batch
    obs = torch.zeros((1, 4, 3, 2))
    params = torch.zeros((2, 20), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch.nll_sweep_gaps(obs, params, K=2, n=2, r=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch.select_smooth_param(obs, params[:1], n=2, r=2, allow_missing=True)


def test_keywords():
    import inspect
    from eks_amd import batch
    from eks_amd.pupil_smoother import ensemble_kalman_smoother_pupil, pupil_smoothing_sweep
    for f in (ensemble_kalman_smoother_pupil, pupil_smoothing_sweep, batch.select_smooth_param):
        assert inspect.signature(f).parameters["allow_missing"].default is False
    sig = inspect.signature(batch.nll_sweep_gaps).parameters
    assert [k for k in sig][:2] == ["obs", "params"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY
               for k in ("K", "n", "r", "mode", "check", "status", "stream"))
    assert sig["mode"].default == "median" and sig["check"].default is True


# ---------------------------------------------------------------------------
# the inputs of the GPU tests
# ---------------------------------------------------------------------------
# (argmin over SCALES, relative gap of the best to the second best: measured
# minima over the trajectories, float64 numpy)
CASES = {"sv131": (3, 0.13), "mc131": (3, 2.6e-4), "pupil131": (5, 0.067), "sv2100": (3, 0.15)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_conditions(name):
    c = S.case(name)
    ref, nobs = c["ref"], c["nobs"]
    K = len(S.SCALES)
    assert ref.shape == (K, c["g"].shape[0]) and np.isfinite(ref).all()
    best = ref.argmin(axis=0)
    srt = np.sort(ref, axis=0)
    gap = (srt[1] - srt[0]) / np.abs(srt[0])
    per_entry = np.abs(ref).min(axis=0) / nobs
    print(f"[gaps sweep ref] {name}: argmin {best.tolist()}, gap {gap.min():.3e}, "
          f"|nll| / nobs {per_entry.min():.3f}")
    assert ((best > 0) & (best < K - 1)).all(), best
    assert (best == CASES[name][0]).all() and gap.min() >= CASES[name][1]
    assert gap.min() >= MIN_GAP
    assert (per_entry >= 1.0).all(), per_entry
    assert (nobs == (~c["mask"]).sum(axis=(1, 2))).all()
    assert (nobs < c["mask"][0].size).any()  # there are gaps


@pytest.mark.parametrize("L", [8, 136])
@pytest.mark.parametrize("name", ["sv131", "mc131"])
def test_chunked_sweep_model_agrees_with_the_dense_reference(name, L):
    c = S.case(name)
    cands = S.scale_candidates(c["models"])
    worst = 0.0
    for b in range(c["g"].shape[0]):
        y, ev = G.ensemble(c["g"][b])
        assert (~G.observed(y, ev) == c["mask"][b]).all()
        got = S.chunked_sweep(y, ev, [ms[b] for ms in cands], L)
        worst = max(worst, float((np.abs(got - c["ref"][:, b]) / np.abs(c["ref"][:, b])).max()))
    print(f"[gaps sweep ref] {name} L={L}: chunked model vs dense, nll rel {worst:.2e}")
    assert worst <= NLL_RTOL, (name, L, worst)


def test_nothing_observed_scores_zero_for_every_candidate():
    c = S.case("sv131")
    y = np.full((20, 2), np.nan)
    cands = [S.scaled(c["models"][0], s) for s in S.SCALES]
    for L in (8, 24):
        assert (S.chunked_sweep(y, y, cands, L) == 0.0).all()
