"""CPU-side checks of the likelihood sweep (eks_nll_sweep): symbols, workspace
and chunk-length queries, argument errors before any launch, the debug key, the
torch operator's registration and shapes, the bracket rule of
batch.select_smooth_param, and a numpy model of the algorithm against the
oracle.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest

from eks_amd import _lib

NEW = ("eks_nll_sweep", "eks_nll_sweep_workspace_bytes", "eks_nll_sweep_chunk_len")


@pytest.fixture
def sweep_chunk():
    """eks_debug_set(EKS_DBG_SWEEP_CHUNK, v) for one test, reset afterwards."""
    yield lambda v: _lib.debug_set(_lib.EKS_DBG_SWEEP_CHUNK, v)
    _lib.debug_set(_lib.EKS_DBG_SWEEP_CHUNK, 0)


def test_symbols_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/eks_hip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert _lib.EKS_DBG_SWEEP_CHUNK == 8
    assert lib.eks_version() >= 102


def _a256(nbytes):
    return (nbytes + 255) // 256 * 256


def _formula(B, K, T, r, L):
    NC = -(-T // L)
    EL = r * r + r + r * (r + 1) // 2 + r + r * (r + 1) // 2  # Elem<R>::len
    return (_a256(T * B * (r * (r + 3) // 2) * 8) + _a256(NC * K * B * (EL + 1) * 8)
            + _a256(NC * B * 8))


@pytest.mark.parametrize("B,K,T,n,r", [(17, 16, 1000, 8, 3), (17, 16, 1000, 2, 2),
                                       (3, 7, 131, 2, 2), (2176, 8, 500, 2, 2), (1, 1, 1, 1, 2)])
def test_workspace_is_the_formula(B, K, T, n, r):
    lib = _lib.load()
    L = lib.eks_nll_sweep_chunk_len(B, K, T, r)
    assert L % 8 == 0 and L >= 8
    assert lib.eks_nll_sweep_workspace_bytes(B, K, T, n, r) == _formula(B, K, T, r, L)


def test_workspace_limits():
    lib = _lib.load()
    # n does not enter once the rows are formed
    assert lib.eks_nll_sweep_workspace_bytes(17, 9, 1000, 64, 3) == \
        lib.eks_nll_sweep_workspace_bytes(17, 9, 1000, 8, 3)
    for n, r in [(8, 4), (65, 3), (2, 1), (0, 2)]:
        assert lib.eks_nll_sweep_workspace_bytes(17, 9, 1000, n, r) == 0, (n, r)
    assert lib.eks_nll_sweep_workspace_bytes(0, 9, 1000, 2, 2) == 0
    assert lib.eks_nll_sweep_workspace_bytes(17, 0, 1000, 2, 2) == 0
    assert lib.eks_nll_sweep_workspace_bytes(17, 9, 0, 2, 2) == 0
    assert lib.eks_nll_sweep_chunk_len(17, 9, 1000, 4) == 0
    assert lib.eks_nll_sweep_chunk_len(17, 0, 1000, 2) == 0


def test_debug_key_forces_the_chunk_length(sweep_chunk):
    lib = _lib.load()
    auto = lib.eks_nll_sweep_chunk_len(2, 7, 2100, 2)
    assert auto % 8 == 0 and 8 <= auto < 2100
    ws_auto = lib.eks_nll_sweep_workspace_bytes(2, 7, 2100, 2, 2)
    assert sweep_chunk(8) == 0
    assert lib.eks_nll_sweep_chunk_len(2, 7, 2100, 2) == 8
    assert lib.eks_nll_sweep_workspace_bytes(2, 7, 2100, 2, 2) == _formula(2, 7, 2100, 2, 8)
    assert lib.eks_nll_sweep_workspace_bytes(2, 7, 2100, 2, 2) != ws_auto  # more chunks
    assert sweep_chunk(13) == 8  # the previous value comes back; rounded up to a multiple of 8
    assert lib.eks_nll_sweep_chunk_len(2, 7, 2100, 2) == 16
    assert sweep_chunk(136) == 13
    assert lib.eks_nll_sweep_chunk_len(3, 7, 131, 2) == 136  # >= T: one chunk
    assert sweep_chunk(10 ** 6) == 136
    assert lib.eks_nll_sweep_chunk_len(3, 7, 131, 2) == 136
    assert sweep_chunk(0) == 10 ** 6
    assert lib.eks_nll_sweep_chunk_len(2, 7, 2100, 2) == auto
    assert lib.eks_nll_sweep_workspace_bytes(2, 7, 2100, 2, 2) == ws_auto
    # a short trajectory is a single chunk on the 8-step grid
    assert lib.eks_nll_sweep_chunk_len(4, 7, 1, 2) == 8 and lib.eks_nll_sweep_chunk_len(4, 7, 2, 3) == 8
    # the other passes' keys are untouched
    assert _lib.debug_set(_lib.EKS_DBG_PVAR_CHUNK, 0) == 0


def _call(lib, obs=8, dtype=_lib.EKS_F32, B=3, T=100, E=5, n=2, r=2, mode=_lib.EKS_MEDIAN,
          params=8, K=7, nll=8, ws=8, ws_bytes=1 << 30, status=8):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return lib.eks_nll_sweep(p(obs), dtype, B, T, E, n, r, 0, 0, 0, 0, mode, p(params), K, p(nll),
                             p(ws), ws_bytes, p(status), None)


def test_argument_errors_do_not_launch():
    lib = _lib.load()
    # (the pointers are never dereferenced: every call below fails validation)
    for arg in ("obs", "params", "nll", "status"):
        assert _call(lib, **{arg: None}) == _lib.EKS_ERR_ARG, arg
        assert b"NULL" in lib.eks_last_error()
    assert _call(lib, T=0) == _lib.EKS_ERR_ARG
    assert _call(lib, K=-1) == _lib.EKS_ERR_ARG
    assert _call(lib, B=-1) == _lib.EKS_ERR_ARG
    assert _call(lib, E=0) == _lib.EKS_ERR_ARG
    assert _call(lib, dtype=9) == _lib.EKS_ERR_ARG
    assert _call(lib, mode=7) == _lib.EKS_ERR_ARG
    assert _call(lib, r=4, n=8) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, r=3, n=65) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, E=lib.eks_max_members() + 1) == _lib.EKS_ERR_UNSUPPORTED
    # a workspace that is missing or too small
    assert _call(lib, ws=None) == _lib.EKS_ERR_ARG and b"workspace" in lib.eks_last_error()
    need = lib.eks_nll_sweep_workspace_bytes(3, 7, 100, 2, 2)
    assert need > 0 and _call(lib, ws_bytes=need - 1) == _lib.EKS_ERR_ARG
    with pytest.raises(_lib.EksError):
        _lib.check(_call(lib, status=None), "eks_nll_sweep")
    # no trajectories or no candidates: nothing to do, nothing launched
    assert _call(lib, B=0) == _lib.EKS_OK
    assert _call(lib, K=0) == _lib.EKS_OK


def test_nll_sweep_op_registered_with_fake_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eks_amd.ops as ops
    assert "nll_sweep" in ops.OPS and hasattr(torch.ops.eks, "nll_sweep")
    dump = torch._C._dispatch_dump("eks::nll_sweep")
    assert "CUDA: registered at" in dump and "Meta: registered at" in dump and "CPU:" not in dump
    with FakeTensorMode():
        obs = torch.empty((3, 100, 5, 8), dtype=torch.float32)
        params = torch.empty((7 * 3, 62), dtype=torch.float64)  # eks_param_len(8, 3)
        nll, st = torch.ops.eks.nll_sweep(obs, params, 7, 8, 3, "median")
        assert nll.shape == (7, 3) and nll.dtype == torch.float64
        assert st.shape == (7, 3) and st.dtype == torch.int32
    with pytest.raises((RuntimeError, NotImplementedError)):  # no CPU kernel
        torch.ops.eks.nll_sweep(torch.zeros((1, 4, 3, 2)), torch.zeros((2, 20), dtype=torch.float64),
                                2, 2, 2, "median")


def test_sweep_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from eks_amd import batch
    obs = torch.zeros((1, 4, 3, 2))
    params = torch.zeros((2, 20), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch.nll_sweep(obs, params, K=2, n=2, r=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        batch.select_smooth_param(obs, params[:1], n=2, r=2)


# -- the bracket rule -----------------------------------------------------------------
def test_bracket_rule():
    import torch
    from eks_amd import batch
    g0 = torch.tensor(batch.DEFAULT_SWEEP_GRID, dtype=torch.float64)
    assert g0.numel() == 9 and g0[0] == 1e-4 and g0[-1] == 1e4
    grid = g0.unsqueeze(0).repeat(3, 1)
    best = torch.tensor([4, 0, 8])  # interior, both edges
    g1 = batch.sweep_bracket(grid, best)
    assert g1.shape == (3, 9) and bool((g1[:, 1:] > g1[:, :-1]).all())
    # interior: from the lower to the upper neighbour, both included; spacing 10^(1/4)
    assert g1[0, 0] == 1e-1 and g1[0, -1] == 1e1
    np.testing.assert_allclose(np.log10(g1[0].numpy()), np.linspace(-1, 1, 9), atol=1e-14)
    # edges: clipped at the grid's ends, which stay in the grid
    assert g1[1, 0] == 1e-4 and g1[1, -1] == 1e-3
    assert g1[2, 0] == 1e3 and g1[2, -1] == 1e4
    np.testing.assert_allclose(np.log10(g1[1].numpy()), np.linspace(-4, -3, 9), atol=1e-14)
    # a second round from an interior point: spacing 10^(1/16)
    g2 = batch.sweep_bracket(g1, torch.tensor([4, 4, 4]))
    np.testing.assert_allclose(np.diff(np.log10(g2[0].numpy())), 1 / 16, atol=1e-14)
    # pure: the inputs are unchanged
    assert torch.equal(grid[0], g0)
    # scaling the Q slice: only Q changes
    from eks_amd.batch import param_len, scale_q
    base = torch.arange(2 * param_len(2, 2), dtype=torch.float64).reshape(2, -1) + 1
    s = torch.tensor([[2.0, 3.0], [5.0, 7.0], [1.0, 1.0]])
    rows = scale_q(base, s, r=2)
    assert rows.shape == (3, 2, 20)
    q = slice(2 + 8, 2 + 12)
    assert torch.equal(rows[1, 1, q], base[1, q] * 7.0) and torch.equal(rows[2], base)
    keep = torch.ones(20, dtype=torch.bool)
    keep[q] = False
    assert torch.equal(rows[0][:, keep], base[:, keep])


def test_refine_zero_is_the_grid_argmin(monkeypatch):
    """select_smooth_param with refine=0 and refine=2 on a synthetic NLL curve
    (the device call replaced by a function of the Q scale): the per-trajectory
    argmin, ties to the smallest s, at_edge, and the refinement's spacing."""
    import torch
    from eks_amd import batch
    opt = torch.tensor([0.37, 1e-4, 3e5])  # log-parabola minima: interior, at / beyond the edges
    P = batch.param_len(2, 2)
    base = torch.zeros((3, P), dtype=torch.float64)
    base[:, 10:14] = 1.0

    def fake_sweep(obs, rows, *, K, n, r, mode="median", **kw):
        s = rows.view(K, 3, P)[:, :, 10]  # Q0 = 1: the scale itself
        return (torch.log10(s) - torch.log10(opt)) ** 2

    monkeypatch.setattr(batch, "nll_sweep", fake_sweep)
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch)
    res = batch.select_smooth_param(None, base, n=2, r=2, refine=0)
    assert res["smooth_param"].tolist() == [1.0, 1e-4, 1e4]
    assert res["at_edge"].tolist() == [False, True, True]
    assert torch.equal(res["params"][:, 10:14], res["smooth_param"].unsqueeze(1).expand(3, 4))
    res2 = batch.select_smooth_param(None, base, n=2, r=2, refine=2)
    assert bool((res2["nll"] <= res["nll"]).all())
    assert abs(np.log10(res2["smooth_param"][0].item() / 0.37)) <= 1 / 32 + 1e-12
    assert res2["at_edge"].tolist() == [False, True, True]
    # ties go to the smallest s
    monkeypatch.setattr(batch, "nll_sweep",
                        lambda obs, rows, *, K, n, r, mode="median", **kw:
                        torch.zeros((K, 3), dtype=torch.float64))
    res = batch.select_smooth_param(None, base, n=2, r=2, refine=1)
    assert res["smooth_param"].tolist() == [1e-4] * 3


# -- a numpy model of the algorithm ---------------------------------------------------
LOG_2PI = float(np.log(2 * np.pi))


def reduce_to_rows(y, ev, C, off):
    """Per step: the r scalar rows (rows of L^T, values, variances) and kappa_t."""
    T, n = y.shape
    r = C.shape[1]
    rows, kappa = [], np.zeros(T)
    for t in range(T):
        z = y[t] - off
        Ri = 1.0 / ev[t]
        W = (C.T * Ri) @ C
        w = C.T @ (Ri * z)
        # W = L D L^T
        L, D = np.eye(r), np.zeros(r)
        for i in range(r):
            D[i] = W[i, i] - np.sum(L[i, :i] ** 2 * D[:i])
            for j in range(i + 1, r):
                L[j, i] = (W[j, i] - np.sum(L[j, :i] * L[i, :i] * D[:i])) / D[i]
        assert np.all(D > 0)
        yt = np.linalg.solve(L, w) / D
        xh = np.linalg.solve(L.T, yt)
        rho = np.sum((z - C @ xh) ** 2 * Ri)
        kappa[t] = 0.5 * ((n - r) * LOG_2PI + np.sum(np.log(ev[t])) + np.sum(np.log(D)) + rho)
        rows.append((L.T.copy(), yt, 1.0 / D))
    return rows, kappa


def model_nll(rows, kappa, m0, S0, A, Q, L=None):
    """NLL of the r-row scalar filter over the rows plus sum kappa.  L = None:
    the sequential filter; else chunks of L steps: chunk 0 the plain filter,
    the others filtering elements built row by row with their likelihood
    constant, folded left to right with the closed-form chunk shares."""
    T, r = len(rows), len(m0)
    L = T if L is None else L
    I = np.eye(r)
    m, P = m0.copy(), S0.copy()
    total = 0.0
    for t in range(min(L, T)):  # chunk 0
        if t > 0:
            m, P = A @ m, A @ P @ A.T + Q
        Ct, yt, rv = rows[t]
        for i in range(r):
            c = Ct[i]
            v = P @ c
            s = c @ v + rv[i]
            e = yt[i] - c @ m
            total += 0.5 * (LOG_2PI + np.log(s) + e * e / s)
            m = m + v * e / s
            P = P - np.outer(v, v) / s
    for s0 in range(L, T, L):
        Ab, bb, Cb, eta, Jb, K = I.copy(), np.zeros(r), np.zeros((r, r)), np.zeros(r), \
            np.zeros((r, r)), 0.0
        for t in range(s0, min(T, s0 + L)):
            Ab, bb, Cb = A @ Ab, A @ bb, A @ Cb @ A.T + Q
            Ct, yt, rv = rows[t]
            for i in range(r):
                c = Ct[i]
                v, g = Cb @ c, Ab.T @ c
                s = c @ v + rv[i]
                e0 = yt[i] - c @ bb
                K += 0.5 * (LOG_2PI + np.log(s) + e0 * e0 / s)
                eta = eta + g * e0 / s
                Jb = Jb + np.outer(g, g) / s
                bb = bb + v * e0 / s
                Ab = Ab - np.outer(v, g) / s
                Cb = Cb - np.outer(v, v) / s
        Wm = I + P @ Jb
        h = eta - Jb @ m
        total += (K - eta @ m + 0.5 * m @ Jb @ m - 0.5 * h @ np.linalg.solve(Wm, P @ h)
                  + 0.5 * np.log(np.linalg.det(Wm)))
        Mi = np.linalg.inv(Wm)
        m, P = Ab @ Mi @ (m + P @ eta) + bb, Ab @ Mi @ P @ Ab.T + Cb
    return total + float(np.sum(kappa))


@pytest.mark.parametrize("kind", ["sv", "mc"])
def test_numpy_model_of_the_algorithm_matches_the_oracle(kind):
    """The reduction to r scalar rows + kappa, sequential and chunked at L = 8
    (17 chunks, the last of 3 steps), against oracle.compute_nll on the sv
    (3, 131) and mc V = 4 (3, 131) data, 7 candidates each: rtol 1e-11, 20x the
    4.5e-13 of the sequential form.  The chunked model's own figure: 1.3e-15
    (sv) / 4.52e-13 (mc); sequential 2.2e-15 (sv) / 4.52e-13 (mc)."""
    from oracle import eks_oracle as O
    import sweep_data as D
    st, models, ref = D.dataset(kind, 3, 131)
    worst = {"seq": 0.0, "chunked": 0.0}
    for b in range(3):
        p = models[b]
        preds, ev = O.ensemble_array(st[b])
        rows, kappa = reduce_to_rows(preds, ev, p["C"], p["means"])
        if kind == "sv":  # C = I: the rows are the observations themselves, kappa = 0
            assert np.abs(kappa).max() < 1e-12 and all(np.array_equal(R[0], np.eye(2)) for R in rows)
        for k, s in enumerate(D.SCALES):
            for name, L in (("seq", None), ("chunked", 8)):
                got = model_nll(rows, kappa, p["m0"], p["S0"], p["A"], s * p["Q"], L)
                worst[name] = max(worst[name], abs(got - ref[k, b]) / abs(ref[k, b]))
    print(f"[sweep] numpy model vs oracle, {kind}: sequential {worst['seq']:.3e}, "
          f"chunked L=8 {worst['chunked']:.3e}")
    assert worst["seq"] <= 1e-11 and worst["chunked"] <= 1e-11
    # the properties of the inputs the GPU tests rely on
    assert np.min(np.abs(ref)) / 131 >= 4.6
    order = np.sort(ref, axis=0)
    assert np.all((np.argmin(ref, axis=0) > 0) & (np.argmin(ref, axis=0) < len(D.SCALES) - 1))
    assert np.min((order[1] - order[0]) / np.abs(order[0])) >= 5.5e-4
