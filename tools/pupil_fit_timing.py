"""Cost of the pupil model fitted on the device (eks_fit_pupil) beside the host
path it replaces.

    python tools/pupil_fit_timing.py [--reps 15] [--warmup 3] [--host-reps 1] [--shapes c5 wide]

Shapes: config 5's (B = 1, T = 1 000 000: frames across a wave) and B = 256,
T = 10 000 (trajectory-fastest lanes); E = 5 float32 members, time-major,
synthetic pupil keypoints (a random walk of diameter and centre seen by E noisy
members).  For each it prints the median device time of ``batch.fit_pupil``
with and without the hand-off planes (events around the calls after warm-up),
its two kernels' times (eks_profile_begin / _end events around each launch),
the bytes the call moves -- E * 8 * 4 read and, with planes, 2 * 8 * 8 written
per frame -- over that time as a fraction of the achievable HBM rate
(6.3 TB/s, MI355X_MICROARCH: the stream bound), and the wall-clock time of the
host path: a device-to-host copy of the members, ``core.ensemble_array``, and
``fit.pupil_model`` for every trajectory (``--host-reps`` runs).  One JSON line
per row follows the table.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pvar_timing import timed  # noqa: E402

SHAPES = {"c5": (1, 1_000_000), "wide": (256, 10_000)}
E, N = 5, 8
HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy), not the 8 TB/s spec


def pupil_members(torch, B, T, seed=0):
    """(B, T, E, 8) float32 view of a time-major (T, E, 8, B) buffer."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    f32 = dict(generator=g, device="cuda", dtype=torch.float32)
    z = torch.randn((T, 3, B), **f32).mul_(0.05).cumsum(0)
    d, cx, cy = z[:, 0] + 16.0, z[:, 1] + 52.0, z[:, 2] + 51.0
    clean = torch.stack([cx, cy - d / 2, cx, cy + d / 2, cx + d / 2, cy, cx - d / 2, cy], 1)
    obs = torch.randn((T, E, N, B), **f32).add_(clean.unsqueeze(1))
    return obs.permute(3, 0, 1, 2)


def host_path(torch, obs):
    """What the wrappers did before: members to the host, the ensemble through
    core.ensemble_array, fit.pupil_model per trajectory."""
    from eks_amd import core, fit
    st = obs.permute(0, 2, 1, 3).contiguous().cpu().numpy()  # (B, E, T, 8)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b in range(st.shape[0]):
            preds, _ = core.ensemble_array(st[b])
            fit.pupil_model(preds, np.eye(3))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-max-b", type=int, default=16,
                    help="trajectories of the host path that are timed (scaled to B)")
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    a = ap.parse_args(argv)
    from eks_amd import _lib, batch
    torch = _lib.require_gpu()
    lib = _lib.load()
    rows = []
    for name in a.shapes:
        B, T = SHAPES[name]
        obs = pupil_members(torch, B, T)
        res = batch.fit_pupil(obs, keep_yev=True)
        yev = res["yev"]
        assert int(res["status"].abs().sum()) == 0 and bool((res["ncomplete"] == T).all())
        assert bool(torch.isfinite(res["stats"]).all())
        read = B * T * E * N * 4
        written = B * T * N * 16
        fit_ms = timed(torch, lambda: batch.fit_pupil(obs, check=False), a.reps, a.warmup)
        yev_ms = timed(torch, lambda: batch.fit_pupil(obs, check=False, keep_yev=yev), a.reps,
                       a.warmup)
        row = dict(shape=name, B=B, T=T, E=E, workspace_bytes=int(
            lib.eks_fit_pupil_workspace_bytes(B, T)), read_bytes=read, written_bytes=written,
            fit_ms=fit_ms, fit_yev_ms=yev_ms,
            fit_stream_fraction=read / HBM_BYTES_PER_S / (fit_ms * 1e-3),
            fit_yev_stream_fraction=(read + written) / HBM_BYTES_PER_S / (yev_ms * 1e-3))
        _lib.profile_begin(a.reps + 1)
        for _ in range(a.reps):
            batch.fit_pupil(obs, check=False, keep_yev=yev)
        torch.cuda.synchronize()
        row["kernels_ms"] = {k: v / a.reps for k, v in _lib.profile_end()}
        hb = min(B, a.host_max_b)
        host = []
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_path(torch, obs[:hb])
            host.append((time.perf_counter() - t0) * 1e3 * B / hb)
        row["host_path_ms"] = statistics.median(host)
        row["host_trajectories_timed"] = hb
        row["host_over_device"] = row["host_path_ms"] / yev_ms
        rows.append(row)
        del obs, yev, res
    print(f"{'shape':6}{'B':>5}{'T':>9} {'fit':>8} {'fit+yev':>8} {'stream':>7} {'stream+yev':>10} "
          f"{'host':>10} {'ratio':>8}   kernels (ms)")
    for w in rows:
        ks = "  ".join(f"{k[2:]} {v:.4f}" for k, v in w["kernels_ms"].items())
        print(f"{w['shape']:6}{w['B']:>5}{w['T']:>9} {w['fit_ms']:>8.4f} {w['fit_yev_ms']:>8.4f} "
              f"{w['fit_stream_fraction']:>7.3f} {w['fit_yev_stream_fraction']:>10.3f} "
              f"{w['host_path_ms']:>10.1f} {w['host_over_device']:>8.0f}   {ks}")
    for w in rows:
        print(json.dumps(w))


if __name__ == "__main__":
    main()
