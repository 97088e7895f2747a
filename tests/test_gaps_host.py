"""CPU-side checks of the missing-observation smoother (eks_smooth_gaps):
symbols, workspace and chunk-length queries, argument errors before any
launch, the debug key, the torch operator's registration and shapes -- no
kernel is launched here -- and the references of tests/gaps_ref.py pinned
against the oracle and against each other.

Bounds of the pinning tests: 1e-10 px on out, 1e-10 relative on var, 1e-11
relative on the NLL, about 1000 x the maxima of a float64 numpy check of the
same formulas (9e-14 px, 7e-14, 2e-14)."""
import ctypes

import numpy as np
import pytest

import gaps_ref as G
from eks_amd import _lib

NEW = ("eks_smooth_gaps", "eks_smooth_gaps_workspace_bytes", "eks_smooth_gaps_chunk_len")
OUT_TOL, VAR_RTOL, NLL_RTOL = 1e-10, 1e-10, 1e-11


@pytest.fixture
def gaps_chunk():
    """eks_debug_set(EKS_DBG_GAPS_CHUNK, v) for one test, reset afterwards."""
    yield lambda v: _lib.debug_set(_lib.EKS_DBG_GAPS_CHUNK, v)
    _lib.debug_set(_lib.EKS_DBG_GAPS_CHUNK, 0)


def test_symbols_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/eks_hip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert _lib.EKS_DBG_GAPS_CHUNK == 9
    assert lib.eks_version() >= 103


def test_workspace_and_limits():
    lib = _lib.load()
    # W_t, P_t (Sym), w_t, m_t (r) and kappa_t planes for every step: 11 doubles at r = 2,
    # 19 at r = 3, plus the chunk arrays
    assert lib.eks_smooth_gaps_workspace_bytes(17, 1000, 2, 2) >= 1000 * 17 * 11 * 8
    assert lib.eks_smooth_gaps_workspace_bytes(17, 1000, 8, 3) >= 1000 * 17 * 19 * 8
    # n does not enter once W_t, w_t and kappa_t are formed
    assert lib.eks_smooth_gaps_workspace_bytes(17, 1000, 64, 3) == \
        lib.eks_smooth_gaps_workspace_bytes(17, 1000, 8, 3)
    assert lib.eks_smooth_gaps_workspace_bytes(17, 1000, 10, 2) == \
        lib.eks_smooth_gaps_workspace_bytes(17, 1000, 2, 2)
    for n, r in [(8, 4), (65, 3), (2, 1), (0, 2)]:
        assert lib.eks_smooth_gaps_workspace_bytes(17, 1000, n, r) == 0, (n, r)
    assert lib.eks_smooth_gaps_workspace_bytes(0, 1000, 2, 2) == 0
    assert lib.eks_smooth_gaps_workspace_bytes(17, 0, 2, 2) == 0
    assert lib.eks_smooth_gaps_chunk_len(17, 1000, 4) == 0


def _call(lib, obs=8, dtype=_lib.EKS_F32, B=3, T=100, E=5, n=2, r=2, mode=_lib.EKS_MEDIAN,
          params=8, out=8, ws=8, ws_bytes=1 << 30, status=8):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return lib.eks_smooth_gaps(p(obs), dtype, B, T, E, n, r, 0, 0, 0, 0, mode, p(params), p(out),
                               0, 0, 0, None, None, None, None, None, p(ws), ws_bytes, p(status),
                               None)


def test_argument_errors_do_not_launch():
    lib = _lib.load()
    # (the pointers are never dereferenced: every call below fails validation)
    assert _call(lib, status=None) == _lib.EKS_ERR_ARG and b"NULL" in lib.eks_last_error()
    assert _call(lib, out=None) == _lib.EKS_ERR_ARG and b"NULL" in lib.eks_last_error()
    assert _call(lib, obs=None) == _lib.EKS_ERR_ARG
    assert _call(lib, params=None) == _lib.EKS_ERR_ARG
    assert _call(lib, T=0) == _lib.EKS_ERR_ARG
    assert _call(lib, E=0) == _lib.EKS_ERR_ARG
    assert _call(lib, dtype=9) == _lib.EKS_ERR_ARG
    assert _call(lib, mode=7) == _lib.EKS_ERR_ARG
    assert _call(lib, r=4, n=8) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, r=3, n=65) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, E=lib.eks_max_members() + 1) == _lib.EKS_ERR_UNSUPPORTED
    # a workspace that is missing or too small
    assert _call(lib, ws=None) == _lib.EKS_ERR_ARG and b"workspace" in lib.eks_last_error()
    need = lib.eks_smooth_gaps_workspace_bytes(3, 100, 2, 2)
    assert _call(lib, ws_bytes=need - 1) == _lib.EKS_ERR_ARG
    with pytest.raises(_lib.EksError):
        _lib.check(_call(lib, status=None), "eks_smooth_gaps")
    # no trajectories: nothing to do, nothing launched
    assert _call(lib, B=0) == _lib.EKS_OK


def test_debug_key_forces_the_chunk_length(gaps_chunk):
    lib = _lib.load()
    auto = lib.eks_smooth_gaps_chunk_len(2, 2100, 2)
    assert auto % 8 == 0 and 8 <= auto < 2100
    ws_auto = lib.eks_smooth_gaps_workspace_bytes(2, 2100, 2, 2)
    assert gaps_chunk(8) == 0
    assert lib.eks_smooth_gaps_chunk_len(2, 2100, 2) == 8
    assert lib.eks_smooth_gaps_workspace_bytes(2, 2100, 2, 2) != ws_auto  # more chunks
    assert gaps_chunk(13) == 8  # the previous value comes back; rounded up to a multiple of 8
    assert lib.eks_smooth_gaps_chunk_len(2, 2100, 2) == 16
    assert gaps_chunk(136) == 13
    assert lib.eks_smooth_gaps_chunk_len(3, 131, 2) == 136  # >= T: one chunk
    assert gaps_chunk(10 ** 6) == 136
    assert lib.eks_smooth_gaps_chunk_len(3, 131, 2) == 136
    assert gaps_chunk(0) == 10 ** 6
    assert lib.eks_smooth_gaps_chunk_len(2, 2100, 2) == auto
    assert lib.eks_smooth_gaps_workspace_bytes(2, 2100, 2, 2) == ws_auto
    # the other passes' keys are their own
    _lib.debug_set(_lib.EKS_DBG_PVAR_CHUNK, 8)
    try:
        assert lib.eks_smooth_gaps_chunk_len(2, 2100, 2) == auto
    finally:
        _lib.debug_set(_lib.EKS_DBG_PVAR_CHUNK, 0)
    # a short trajectory is a single chunk on the 8-step grid
    assert lib.eks_smooth_gaps_chunk_len(4, 1, 2) == 8
    assert lib.eks_smooth_gaps_chunk_len(4, 2, 3) == 8


def test_smooth_gaps_op_registered_with_fake_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eks_amd.ops as ops
    assert "smooth_gaps" in ops.OPS and hasattr(torch.ops.eks, "smooth_gaps")
    dump = torch._C._dispatch_dump("eks::smooth_gaps")
    assert "CUDA: registered at" in dump and "Meta: registered at" in dump and "CPU:" not in dump
    with FakeTensorMode():
        obs = torch.empty((3, 100, 5, 8), dtype=torch.float32)
        params = torch.empty((3, 62), dtype=torch.float64)  # eks_param_len(8, 3)
        out, var, nll, nobs, st = torch.ops.eks.smooth_gaps(obs, params, 8, 3, "median")
        assert out.shape == (3, 100, 8) and out.dtype == torch.float64
        assert var.shape == (3, 100, 8) and var.dtype == torch.float64
        assert nll.shape == (3,) and nll.dtype == torch.float64
        assert nobs.shape == (3,) and nobs.dtype == torch.int32
        assert st.shape == (3,) and st.dtype == torch.int32
    with pytest.raises((RuntimeError, NotImplementedError)):  # no CPU kernel
        torch.ops.eks.smooth_gaps(torch.zeros((1, 4, 3, 2)),
                                  torch.zeros((1, 20), dtype=torch.float64), 2, 2, "median")


def test_smooth_gaps_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from eks_amd import batch
    obs = torch.zeros((1, 4, 3, 2))
    params = torch.zeros((1, 20), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch.smooth_gaps(obs, params, n=2, r=2)


def test_wrappers_take_allow_missing():
    import inspect
    from eks_amd.smoothers import (ensemble_kalman_smoother_multi_cam,
                                   ensemble_kalman_smoother_single_view)
    for f in (ensemble_kalman_smoother_multi_cam, ensemble_kalman_smoother_single_view):
        assert inspect.signature(f).parameters["allow_missing"].default is False


# ---------------------------------------------------------------------------
# pinning the references
# ---------------------------------------------------------------------------
def _agree(a, b, what):
    assert np.isfinite(b["out"]).all() and np.isfinite(b["var"]).all() and np.isfinite(b["nll"])
    d_out = float(np.abs(a["out"] - b["out"]).max())
    d_var = float((np.abs(a["var"] - b["var"]) / np.abs(b["var"])).max())
    d_nll = abs(a["nll"] - b["nll"]) / abs(b["nll"]) if b["nll"] != 0 else abs(a["nll"])
    print(f"[gaps ref] {what}: out {d_out:.2e} px, var rel {d_var:.2e}, nll rel {d_nll:.2e}")
    assert d_out <= OUT_TOL, (what, d_out)
    assert d_var <= VAR_RTOL, (what, d_var)
    assert d_nll <= NLL_RTOL, (what, d_nll)
    assert a["nobs"] == b["nobs"]


@pytest.mark.parametrize("kind,n", [("sv", 2), ("mc", 8)])
def test_dense_reference_equals_the_oracle_on_complete_data(kind, n):
    from oracle import eks_oracle as O
    st = G.members(kind, 2, 131)
    for b in range(2):
        p = G.model_of(kind, st[b])
        y, ev = O.ensemble_array(st[b])
        yc = y - p["means"]
        mf, Vf, S = O.filtering_pass(yc, p["m0"], p["S0"], p["C"], np.eye(n), p["A"], p["Q"], ev)
        ms, Vs, _ = O.smooth_backward(yc, mf, Vf, S, p["A"])
        ref = dict(out=ms @ p["C"].T + p["means"],
                   var=np.einsum("ji,tik,jk->tj", p["C"], Vs, p["C"]),
                   nll=O.compute_nll(yc, p["m0"], p["S0"], p["C"], p["A"], p["Q"], ev),
                   nobs=131 * n)
        _agree(G.dense(y, ev, p), ref, f"{kind} b={b} dense vs oracle")


@pytest.mark.parametrize("L", [8, 136])
def test_chunked_model_agrees_with_the_dense_reference_singleview(L):
    g, models, ref, mask = G.case_sv131()
    assert mask[0, 45:85].all() and mask[:2, 0].all() and mask[:2, -1].all() and not mask[2].any()
    for b in range(3):
        y, ev = G.ensemble(g[b])
        assert (~G.observed(y, ev) == mask[b]).all()
        _agree(G.chunked(y, ev, models[b], L), ref[b], f"sv b={b} L={L}")


@pytest.mark.parametrize("L", [8, 136])
def test_chunked_model_agrees_with_the_dense_reference_multicam(L):
    st = G.members("mc", 1, 131)
    p = G.model_of("mc", st[0])
    mask = np.random.default_rng(5).random((1, 131, 8)) < 0.5
    mask[0, 20:60, 2:] = True   # one camera only: 2 observations for r = 3
    mask[0, 70, 1:] = True      # a single column
    mask[0, 90:100] = True      # nothing observed
    y, ev = G.ensemble(G.knock_out(st, mask)[0])
    _agree(G.chunked(y, ev, p, L), G.dense(y, ev, p), f"mc L={L}")


def test_absorbing_a_step_is_composing_its_element():
    """The one-inverse step of G1 against the step element of the issue's
    formulas composed with compose_elem, and the element applied to a state
    against the filter step (compose_state's convention)."""
    rng = np.random.default_rng(3)
    for r in (2, 3):
        def spd(k=r):
            X = rng.normal(size=(r, k))
            return X @ X.T
        A, Q, P = rng.normal(size=(r, r)), spd(), spd()
        m = rng.normal(size=r)
        E = (np.eye(r), np.zeros(r), np.zeros((r, r)), np.zeros(r), np.zeros((r, r)))
        for W in (spd(), spd(1), np.zeros((r, r))):  # full rank, rank one, nothing observed
            w = W @ rng.normal(size=r)
            St = G.step_elem(A, Q, W, w)
            E2 = G.compose_elem(E, St)
            E1 = G.absorb(E, True, A, Q, W, w)
            for a, b in zip(E1, E2):
                np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-12)
            m1, P1 = G.compose_state(m, P, St)
            m2, P2, _ = G.filter_step(1, A, Q, W, w, 0.0, m, P)
            np.testing.assert_allclose(m1, m2, rtol=1e-10, atol=1e-12)
            np.testing.assert_allclose(P1, P2, rtol=1e-10, atol=1e-12)
            E = E1
        if r == 2:
            Z = np.zeros((r, r))
            for a, b in zip(G.step_elem(A, Q, Z, np.zeros(r)), (A, np.zeros(r), Q, np.zeros(r), Z)):
                np.testing.assert_array_equal(a, b)  # W = 0: the prediction (A, 0, Q, 0, 0)


def test_nothing_observed_is_the_prior_carried_forward():
    st = G.members("sv", 1, 20)
    p = G.model_of("sv", st[0])
    p["m0"] = np.array([1.5, -2.0])
    p["A"] = np.array([[0.9, 0.1], [0.0, 0.8]])
    y = np.full((20, 2), np.nan)
    ev = np.full((20, 2), np.nan)
    for res in (G.dense(y, ev, p), G.chunked(y, ev, p, 8)):
        m = p["m0"]
        for t in range(20):
            if t > 0:
                m = p["A"] @ m
            np.testing.assert_allclose(res["ms"][t], m, rtol=1e-12, atol=0)
        assert res["nll"] == 0.0 and res["nobs"] == 0
