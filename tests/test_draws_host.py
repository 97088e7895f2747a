"""CPU-side checks of the posterior trajectory draws (eks_draws_gaps,
eks_draws_noise): symbols, workspace and chunk-length queries, argument errors
before any launch, the torch operators' registration, batch.draws_gaps's
noise / seed rule -- no kernel is launched here -- and tests/draws_ref.py
pinned against itself: the backward sampler fed the T r one-hot noise vectors
against the dense joint posterior, zero noise against gaps_ref.dense, and the
numpy model of the generator against the moments of a standard normal.

The four cases: single-view (n = 2, r = 2) and 4-camera (n = 8, r = 3), T = 24,
each with 25 % random gaps, a 5-frame void and the first and last frame
missing, and each complete.  Bound of the identity M M^T = Sigma: 1e-12
relative to max |Sigma| (measured here: <= 5.5e-15; cond Sigma <= 1.4e3).

The generator: 2^20 normals of seed 20261021 (B = 4, S = 64, T = 2048, r = 2);
measured |mean| 3.1e-4 (bound 4.9e-3), |var - 1| 9.5e-4 (6.9e-3), lag-1
correlations along t, s, i 4.4e-4, 2.6e-4, 2.2e-3 (4.9e-3).
"""
import ctypes

import numpy as np
import pytest

import draws_ref as D
import gaps_ref as G
from eks_amd import _lib

NEW = ("eks_draws_gaps", "eks_draws_gaps_workspace_bytes", "eks_draws_gaps_chunk_len",
       "eks_draws_noise")
SEED, SHAPE = 20261021, (4, 64, 2048, 2)


def test_symbols_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared, f"{name} not declared in include/eks_hip.h"
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert _lib.EKS_DBG_DRAWS_RAW == 11
    assert lib.eks_version() >= 108


def test_workspace_and_chunk_len():
    lib = _lib.load()
    for n, r in [(2, 2), (8, 3)]:
        base = lib.eks_smooth_gaps_workspace_bytes(17, 1000, n, r)
        prev = 0
        for S in (0, 1, 4, 5, 64, 1000):
            w = lib.eks_draws_gaps_workspace_bytes(17, S, 1000, n, r)
            assert w >= base and w >= prev, (n, r, S)
            prev = w
        # the factors of every step: r r + r (r + 1) / 2 doubles per trajectory
        assert lib.eks_draws_gaps_workspace_bytes(17, 1, 1000, n, r) - base >= \
            1000 * 17 * (r * r + r * (r + 1) // 2) * 8
    for n, r in [(8, 4), (65, 3), (2, 1), (0, 2)]:
        assert lib.eks_draws_gaps_workspace_bytes(17, 4, 1000, n, r) == 0, (n, r)
    assert lib.eks_draws_gaps_workspace_bytes(0, 4, 1000, 2, 2) == 0
    assert lib.eks_draws_gaps_workspace_bytes(17, 4, 0, 2, 2) == 0
    assert lib.eks_draws_gaps_workspace_bytes(17, -1, 1000, 2, 2) == 0
    assert lib.eks_draws_gaps_workspace_bytes(1 << 20, 1 << 20, 10, 2, 2) == 0  # B S > 2^28
    for B, T, r in [(17, 1000, 2), (17, 100000, 3), (3, 131, 2), (4, 1, 2), (2, 2100, 4)]:
        assert lib.eks_draws_gaps_chunk_len(B, T, r) == lib.eks_smooth_gaps_chunk_len(B, T, r)
    _lib.debug_set(_lib.EKS_DBG_GAPS_CHUNK, 8)
    try:
        assert lib.eks_draws_gaps_chunk_len(2, 2100, 2) == 8
    finally:
        _lib.debug_set(_lib.EKS_DBG_GAPS_CHUNK, 0)


def _call(lib, obs=8, dtype=_lib.EKS_F32, B=3, T=100, E=5, n=2, r=2, mode=_lib.EKS_MEDIAN,
          params=8, S=4, draws=8, out=None, pvar=None, ws=8, ws_bytes=1 << 30, status=8):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return lib.eks_draws_gaps(p(obs), dtype, B, T, E, n, r, 0, 0, 0, 0, mode, p(params), S, None,
                              0, 0, 0, 1, p(draws), 0, 0, 0, 0, None, p(out), 0, 0, 0, p(pvar),
                              p(ws), ws_bytes, p(status), None)


def test_argument_errors_do_not_launch():
    lib = _lib.load()
    # (the pointers are never dereferenced: every call below fails validation)
    assert _call(lib, S=-1) == _lib.EKS_ERR_ARG and b"S>=0" in lib.eks_last_error()
    assert _call(lib, draws=None) == _lib.EKS_ERR_ARG and b"NULL" in lib.eks_last_error()
    assert _call(lib, status=None) == _lib.EKS_ERR_ARG
    assert _call(lib, obs=None) == _lib.EKS_ERR_ARG
    assert _call(lib, params=None) == _lib.EKS_ERR_ARG
    assert _call(lib, T=0) == _lib.EKS_ERR_ARG
    assert _call(lib, dtype=9) == _lib.EKS_ERR_ARG
    assert _call(lib, mode=7) == _lib.EKS_ERR_ARG
    assert _call(lib, pvar=8) == _lib.EKS_ERR_ARG  # pvar has out's strides
    assert _call(lib, r=4, n=8) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, r=3, n=65) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, E=lib.eks_max_members() + 1) == _lib.EKS_ERR_UNSUPPORTED
    assert _call(lib, ws=None) == _lib.EKS_ERR_ARG and b"workspace" in lib.eks_last_error()
    need = lib.eks_draws_gaps_workspace_bytes(3, 4, 100, 2, 2)
    assert need > 0 and _call(lib, ws_bytes=need - 1) == _lib.EKS_ERR_ARG
    # the smoother's own workspace is not enough
    assert _call(lib, ws_bytes=lib.eks_smooth_gaps_workspace_bytes(3, 100, 2, 2)) == \
        _lib.EKS_ERR_ARG
    assert _call(lib, B=0) == _lib.EKS_OK  # no trajectories: nothing launched
    assert lib.eks_draws_noise(3, 4, 10, 5, 1, ctypes.c_void_p(8), 0, 0, 0, None) == \
        _lib.EKS_ERR_UNSUPPORTED
    assert lib.eks_draws_noise(-1, 4, 10, 2, 1, ctypes.c_void_p(8), 0, 0, 0, None) == \
        _lib.EKS_ERR_ARG
    assert lib.eks_draws_noise(3, 4, 10, 2, 1, None, 0, 0, 0, None) == _lib.EKS_ERR_ARG
    assert lib.eks_draws_noise(3, 0, 10, 2, 1, None, 0, 0, 0, None) == _lib.EKS_OK


def test_ops_registered_with_fake_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import eks_amd.ops as ops
    for name in ("draws_gaps", "draws_noise"):
        assert name in ops.OPS and hasattr(torch.ops.eks, name)
        dump = torch._C._dispatch_dump("eks::" + name)
        assert "CUDA: registered at" in dump and "Meta: registered at" in dump
        assert "CPU:" not in dump
    with FakeTensorMode():
        obs = torch.empty((3, 100, 5, 8), dtype=torch.float32)
        params = torch.empty((3, 62), dtype=torch.float64)  # eks_param_len(8, 3)
        noise = torch.empty((3, 7, 100, 3), dtype=torch.float64)
        draws, latent, out, st = torch.ops.eks.draws_gaps(obs, params, noise, 8, 3, "median")
        assert draws.shape == (3, 7, 100, 8) and draws.dtype == torch.float64
        assert latent.shape == (3, 7, 100, 3) and latent.dtype == torch.float64
        assert out.shape == (3, 100, 8) and st.shape == (3,) and st.dtype == torch.int32
        z = torch.ops.eks.draws_noise(obs, 3, 7, 100, 3, 5)
        assert z.shape == (3, 7, 100, 3) and z.dtype == torch.float64


def test_batch_draws_gaps_wants_one_of_noise_and_seed():
    from eks_amd import batch
    with pytest.raises(ValueError, match="exactly one"):
        batch.draws_gaps(None, None, n=2, r=2, S=3)
    with pytest.raises(ValueError, match="exactly one"):
        batch.draws_gaps(None, None, n=2, r=2, noise=object(), seed=1)


@pytest.mark.parametrize("kind,gaps", D.CASES)
def test_reference_pinned_against_the_dense_posterior(kind, gaps):
    _, model, y, ev, mask = D.case(kind, 24, gaps)
    T, r = 24, model["m0"].shape[0]
    if gaps:
        assert mask[0, 9:14].all() and mask[0, 0].all() and mask[0, -1].all()
        assert 0.25 < mask.mean() < 0.6
    else:
        assert not mask.any()
    Sigma, mean = D.joint(y, ev, model)
    assert np.isfinite(Sigma).all() and np.isfinite(mean).all()
    res = D.draws(y, ev, model, D.one_hot(T, r))
    M = D.responses(res["latent"], res["ms"])
    err = float(np.abs(M @ M.T - Sigma).max() / np.abs(Sigma).max())
    dense = G.dense(y, ev, model)
    zero = D.draws(y, ev, model, np.zeros((2, T, r)))
    e_mean = float(np.abs(mean @ model["C"].T + model["means"] - dense["out"]).max())
    e_zero = float(np.abs(zero["draws"] - dense["out"][None]).max())
    print(f"[draws_ref] {kind} gaps={gaps}: M M^T vs Sigma {err:.3e}, cond {np.linalg.cond(Sigma):.3e}, "
          f"joint mean vs dense {e_mean:.3e} px, zero noise vs dense {e_zero:.3e} px")
    assert err <= 1e-12
    assert e_mean <= 1e-10 and e_zero <= 1e-10
    # the diagonal blocks are dense's Vs
    for t in range(T):
        blk = Sigma[t * r:(t + 1) * r, t * r:(t + 1) * r]
        assert np.abs(blk - dense["Vs"][t]).max() <= 1e-12 * np.abs(Sigma).max()


def test_philox_known_answers():
    # Random123's kat_vectors, philox4x32-10
    z = np.zeros(1, dtype=np.uint64)
    f = np.full(1, 0xFFFFFFFF, dtype=np.uint64)
    assert [int(v[0]) for v in D.philox4x32_10((z, z, z, z), (0, 0))] == \
        [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v[0]) for v in D.philox4x32_10((f, f, f, f), (0xFFFFFFFF, 0xFFFFFFFF))] == \
        [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_generator_model_moments():
    z = D.normals(SEED, *SHAPE)
    N = z.size
    assert N == 2 ** 20 and np.isfinite(z).all() and np.abs(z).max() < 8.6
    k = D.raw(SEED, 2, 3, 5, 3)
    assert k.max() < 2 ** 53 and len(np.unique(k)) == k.size

    def corr(a, b):
        return float(abs(np.corrcoef(a.ravel(), b.ravel())[0, 1]))

    mean, var = float(abs(z.mean())), float(abs(z.var() - 1.0))
    ct, cs = corr(z[:, :, 1:], z[:, :, :-1]), corr(z[:, 1:], z[:, :-1])
    ci = corr(z[..., 0], z[..., 1])
    print(f"[draws_ref] seed {SEED}: |mean| {mean:.3e}, |var - 1| {var:.3e}, lag-1 t {ct:.3e}, "
          f"s {cs:.3e}, i {ci:.3e}")
    assert mean <= 5 / np.sqrt(N)
    assert var <= 5 * np.sqrt(2 / N)
    assert max(ct, cs, ci) <= 5 / np.sqrt(N)
    # a sub-range reproduces the same values; r = 3 shares components 0, 1 with r = 2
    sub = D.normals(SEED, 2, 3, 7, 2, b0=1, s0=5, t0=100)
    assert np.array_equal(sub, z[1:3, 5:8, 100:107])
    assert np.array_equal(D.normals(SEED, 2, 3, 7, 3)[..., :2], z[:2, :3, :7])
    assert not np.array_equal(D.normals(SEED + 1, 2, 3, 7, 2), z[:2, :3, :7])
