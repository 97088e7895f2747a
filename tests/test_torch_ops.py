"""torch.ops.eks.* are C++ registrations (eks_amd/csrc/torch_ops.cpp,
TORCH_LIBRARY) with CUDA-key and Meta kernels: checked here without a GPU --
the library loads, every operator's dispatch table names only the C++ file,
the Meta kernels propagate shapes (FakeTensor tracing), and a CPU tensor is a
dispatch error (no CPU fallback).  Numerics: tests/test_gpu_parity.py."""
import pytest

torch = pytest.importorskip("torch")


def test_ops_registered_in_cpp():
    import eks_amd.ops as ops
    for op in ops.OPS:
        dump = torch._C._dispatch_dump(f"eks::{op}")
        assert "torch_ops.cpp" in dump, dump
        for key in ("CUDA", "Meta"):
            assert f"{key}: registered at" in dump, (op, key, dump)
        assert "CPU:" not in dump and ".py" not in dump, dump


def test_meta_shapes():
    import eks_amd.ops  # noqa: F401
    m = lambda *s, dt=torch.float32: torch.empty(s, device="meta", dtype=dt)  # noqa: E731
    f8 = torch.float64
    obs = m(6, 50, 5, 2)
    p, v = torch.ops.eks.ensemble(obs, "median")
    assert p.shape == v.shape == (6, 50, 2) and p.dtype == f8
    out, st = torch.ops.eks.smooth(obs, m(6, 20, dt=f8), 2, 2, "median", 0, 0)
    assert out.shape == (6, 50, 2) and out.dtype == f8 and st.shape == (6,) and st.dtype == torch.int32
    assert torch.ops.eks.nll(obs, m(6, 20, dt=f8), 2, 2, "median", 0).shape == (6,)
    prm, st = torch.ops.eks.fit(obs, "singleview", 2, 2, 0.01, 25.0, "median")
    assert prm.shape == (6, 20)
    y = m(3, 40, 8, dt=f8)
    mf, Vf, S, nll, st = torch.ops.eks.forward(y, y, m(3, 3, dt=f8), m(3, 3, 3, dt=f8),
                                               m(3, 3, 3, dt=f8), m(3, 3, 3, dt=f8),
                                               m(3, 8, 3, dt=f8))
    assert mf.shape == (3, 40, 3) and Vf.shape == S.shape == (3, 40, 3, 3) and nll.shape == (3,)
    ms, Vs, CV, st = torch.ops.eks.backward(mf, Vf, S, m(3, 3, 3, dt=f8))
    assert ms.shape == (3, 40, 3) and CV.shape == (3, 39, 3, 3)
    q, st = torch.ops.eks.newton_filter(y, y, m(3, dt=f8), m(3, 3, dt=f8), m(3, 3, dt=f8),
                                        m(8, 3, dt=f8), m(3, 3, dt=f8), 1)
    assert q.shape == (3, 40, 3)
    assert torch.ops.eks.interp1d(m(10, dt=f8), m(10, 4, dt=f8), m(7, dt=f8)).shape == (7, 4)
    _member_op_meta_shapes(2, 2)
    _member_op_meta_shapes(8, 3)


def _member_op_meta_shapes(n, r):
    """Shape, dtype and contiguity of every output of the nine later operators
    at B=3, T=5, E=4, K=2, S=2."""
    import eks_amd.ops  # noqa: F401
    from eks_amd import _lib
    lib = _lib.load()
    B, T, E, K, S = 3, 5, 4, 2, 2
    f4, f8, i4, u1 = torch.float32, torch.float64, torch.int32, torch.uint8
    m = lambda *s, dt=f8: torch.empty(s, device="meta", dtype=dt)  # noqa: E731
    P = lib.eks_param_len(n, r)
    obs, prm, rows = m(B, T, E, n, dt=f4), m(B, P), m(K * B, P)
    eks = torch.ops.eks
    yev32 = lib.eks_yev_bytes(B, T, n, _lib.EKS_F32, E, _lib.EKS_MEDIAN)
    yev64 = lib.eks_yev_bytes(B, T, n, _lib.EKS_F64, E, _lib.EKS_MEDIAN)
    cases = {
        "smooth_var": (eks.smooth_var(obs, prm, n, r),
                       [((B, T, n), f8), ((B, T, r, r), f8), ((B,), i4)]),
        "smooth_gaps": (eks.smooth_gaps(obs, prm, n, r, "median"),
                        [((B, T, n), f8), ((B, T, n), f8), ((B,), f8), ((B,), i4), ((B,), i4)]),
        "draws_gaps": (eks.draws_gaps(obs, prm, m(B, S, T, r), n, r, "median"),
                       [((B, S, T, n), f8), ((B, S, T, r), f8), ((B, T, n), f8), ((B,), i4)]),
        "draws_noise": ((eks.draws_noise(obs, B, S, T, r, 7),), [((B, S, T, r), f8)]),
        "nll_sweep": (eks.nll_sweep(obs, rows, K, n, r, "median"), [((K, B), f8), ((K, B), i4)]),
        "nll_sweep_gaps": (eks.nll_sweep_gaps(obs, rows, K, n, r, "median"),
                           [((K, B), f8), ((B,), i4), ((K, B), i4)]),
        "fit_gaps": (eks.fit_gaps(obs, "multicam" if n > r else "singleview", n, r, 1.0, 25.0,
                                  "median"),
                     [((B, P), f8), ((B,), i4), ((yev32,), u1), ((B,), i4), ((B,), i4)]),
        "ensemble_gaps": (eks.ensemble_gaps(obs, "median", 2), [((yev64,), u1), ((T, n, B), u1)]),
    }
    if n == 8:
        cases["fit_pupil"] = (eks.fit_pupil(obs, "median"),
                              [((B, 6), f8), ((B,), i4), ((B,), i4), ((yev64,), u1)])
    else:  # the pupil model has 8 coordinates: another n is refused by the Meta kernel too
        with pytest.raises(RuntimeError, match="obs must be viewed as"):
            eks.fit_pupil(obs, "median")
    for name, (outs, want) in cases.items():
        assert len(outs) == len(want), name
        for k, (t, (shape, dt)) in enumerate(zip(outs, want)):
            assert t.device.type == "meta" and tuple(t.shape) == shape and t.dtype == dt, (name, k)
            assert t.is_contiguous(), (name, k)


def test_cpu_tensor_is_a_dispatch_error():
    import eks_amd.ops  # noqa: F401
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.eks.ensemble(torch.zeros((1, 4, 3, 2)), "median")
