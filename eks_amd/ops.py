"""``torch.ops.eks.*``: the C ABI entry points as PyTorch operators registered
in C++ ("the torch extension wraps the same functions").

    import eks_amd.ops                       # loads libeks_torch.so
    preds, vars_ = torch.ops.eks.ensemble(obs, "median")
    mf, Vf, S, nll, status = torch.ops.eks.forward(y, ev, m0, S0, A, Q, C)
    ms, Vs, CV, status = torch.ops.eks.backward(mf, Vf, S, A)
    out, status = torch.ops.eks.smooth(obs, params, 2, 2, "median", 0, 0)

The operators are defined by ``TORCH_LIBRARY(eks, ...)`` in
``eks_amd/csrc/torch_ops.cpp`` (built into ``eks_amd/lib/libeks_torch.so`` by
``eks_amd.build``), each with a CUDA-key kernel that calls libeks_hip.so on
the current stream and a Meta kernel for shape propagation (FakeTensor /
``torch.compile``): no Python frame in their dispatch and no CPU kernel (a
CPU tensor is a dispatch error).  Layout conventions are those of
``eks_amd.batch``: obs is (B, T, E, n) with any strides.

    ensemble   eks/ensemble_kalman.py:4-57        forward   :59-117 (filtering_pass)
    backward   :120-164 (smooth_backward)          nll       compute_nll
    smooth     the fused hot path                  fit       eks/multiview_pca_smoother.py:684-731
    newton_filter  eks/newton_eks.py:115-148       interp1d  eks/multiview_pca_smoother.py:86-96
    smooth_var (obs, params, n, r) -> (var (B,T,n), Vs (B,T,r,r), status): the posterior
               variances diag(C Vs C^T) of smooth's output and the smoothed covariances
    nll_sweep  (obs, params (K*B, P), K, n, r, mode) -> (nll (K,B), status (K,B)): the NLL
               of K candidate models per trajectory, the members reduced once
    nll_sweep_gaps (obs, params (K*B, P), K, n, r, mode) -> (nll (K,B), nobs (B), status (K,B)):
               nll_sweep through missing observations, the NLL over the observed entries
    smooth_gaps (obs, params, n, r, mode) -> (out, var (B,T,n), nll (B), nobs (B), status):
               the smoother through missing observations (non-finite ensemble average
               or variance), its posterior variances and the NLL over the observed entries
    draws_gaps (obs, params, noise (B,S,T,r), n, r, mode) -> (draws (B,S,T,n), latent (B,S,T,r),
               out (B,T,n), status): joint draws from smooth_gaps's posterior (batch.draws_gaps;
               the seeded form there).  draws_noise (like, B, S, T, r, seed) -> the noise
               (B,S,T,r) a seeded call generates, on like's device
    ensemble_gaps (obs, mode, min_members) -> (yev bytes (EKS_YEV64 planes), nvalid (T,n,B) uint8):
               the ensemble over the finite members of each column, missing only where
               fewer than min_members are finite
    fit_pupil  (obs (B,T,E,8), mode) -> (stats (B,6), ncomplete (B), status (B), yev bytes):
               the pupil model's statistics over the complete frames, and the EKS_YEV64
               ensemble planes of eks_ensemble_gaps(min_members=E)
"""
from __future__ import annotations

import os

import torch

from . import _lib

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libeks_torch.so")

OPS = ("ensemble", "forward", "backward", "smooth", "smooth_var", "smooth_gaps", "draws_gaps",
       "draws_noise", "nll",
       "nll_sweep", "nll_sweep_gaps", "fit", "fit_gaps", "ensemble_gaps", "fit_pupil", "newton_filter",
       "interp1d")


def _load():
    if not os.path.exists(LIB):
        raise RuntimeError(f"{LIB} is missing: build it (python -m eks_amd.build). "
                           "eks_amd has no CPU fallback.")
    _lib.load()  # libeks_hip.so first (libeks_torch.so links it)
    torch.ops.load_library(LIB)


_load()
