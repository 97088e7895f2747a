"""Cost of the posterior-variance pass (eks_smooth_var) beside the mean smoother.

    python tools/pvar_timing.py [--reps 15] [--warmup 3] [--shapes c2 c3 c4] [--chunk 0 32 64]

For each shape -- config 2 (17 x 100 000, (r, n) = (2, 2)), config 3
(17 x 50 000, (3, 8)) and config 4's 128-video shard (2176 x 10 000, (2, 2)),
E = 5 float32 members, time-major -- it prints the median time of
``batch.smooth`` alone (the yardstick: means only, same library), of
``batch.smooth(want_var=True)``, of the variance pass alone, the pass's five
kernels separately (eks_profile_begin / _end events around each launch) and
its workspace size.  Times are device events around the calls after warm-up;
members are generated and the models fitted (eks_fit) on the device.
``--chunk`` repeats every shape with forced chunk lengths (EKS_DBG_PVAR_CHUNK;
0 = automatic).  One JSON line per row follows the table.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"c2": (17, 100_000, 2, 2, "singleview"), "c3": (17, 50_000, 8, 3, "multicam"),
          "c4": (2176, 10_000, 2, 2, "singleview")}


def members(torch, B, T, n, E=5, seed=0):
    """(B, T, E, n) float32 view of a time-major (T, E, n, B) buffer: a random
    walk seen by E noisy members."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    walk = torch.randn((T, 1, n, B), generator=g, device="cuda", dtype=torch.float32).mul_(2.0)
    walk = walk.cumsum(0).add_(250.0)
    obs = torch.randn((T, E, n, B), generator=g, device="cuda", dtype=torch.float32)
    obs.mul_(1.5).add_(walk)
    return obs.permute(3, 0, 1, 2)


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--chunk", nargs="+", type=int, default=[0],
                    help="chunk lengths of the variance pass to time (0 = automatic)")
    a = ap.parse_args(argv)
    from eks_amd import _lib, batch
    torch = _lib.require_gpu()
    lib = _lib.load()
    rows = []
    for name in a.shapes:
        B, T, n, r, kind = SHAPES[name]
        obs = members(torch, B, T, n)
        params, _ = batch.fit(obs, kind=kind, n=n, r=r, smooth_param=10.0 if r == 2 else 0.01,
                              quantile_keep=50.0 if r == 2 else 25.0)
        flags = _lib.EKS_MODEL_A_IDENTITY | (_lib.EKS_MODEL_C_IDENTITY if r == n else 0)
        mean = lambda: batch.smooth(obs, params, n=n, r=r, flags=flags)  # noqa: E731
        both = lambda: batch.smooth(obs, params, n=n, r=r, flags=flags, want_var=True)  # noqa: E731
        var = lambda: batch.smooth_var(obs, params, n=n, r=r)  # noqa: E731
        smooth_ms = timed(torch, mean, a.reps, a.warmup)
        for chunk in a.chunk:
            _lib.debug_set(_lib.EKS_DBG_PVAR_CHUNK, chunk)
            rows.append(measure(torch, lib, a, name, mean, both, var, smooth_ms))
        _lib.debug_set(_lib.EKS_DBG_PVAR_CHUNK, 0)
        del obs
    report(rows)


def measure(torch, lib, a, name, mean, both, var, smooth_ms):
    from eks_amd import _lib
    B, T, n, r, _ = SHAPES[name]
    st = both()["status"]
    assert int(st.abs().sum()) == 0, "status bits set"
    row = dict(shape=name, B=B, T=T, n=n, r=r,
               chunk_len=int(lib.eks_smooth_var_chunk_len(B, T, r)),
               workspace_bytes=int(lib.eks_smooth_var_workspace_bytes(B, T, n, r)),
               smooth_workspace_bytes=int(lib.eks_smooth_workspace_bytes(B, T, n, r, 5, 0)),
               smooth_ms=smooth_ms,
               smooth_want_var_ms=timed(torch, both, a.reps, a.warmup),
               var_pass_ms=timed(torch, var, a.reps, a.warmup))
    _lib.profile_begin(a.reps + 1)
    for _ in range(a.reps):
        var()
    torch.cuda.synchronize()
    row["kernels_ms"] = {k: v / a.reps for k, v in _lib.profile_end()}
    return row


def report(rows):
    print(f"{'shape':6}{'B':>6}{'T':>8} (r,n)  {'L':>4} {'smooth':>9} {'+want_var':>10} "
          f"{'var pass':>9}   kernels of the variance pass (ms)")
    for w in rows:
        ks = "  ".join(f"{k[5:]} {v:.3f}" for k, v in w["kernels_ms"].items())
        print(f"{w['shape']:6}{w['B']:>6}{w['T']:>8} ({w['r']},{w['n']})  {w['chunk_len']:>4} "
              f"{w['smooth_ms']:>9.3f} {w['smooth_want_var_ms']:>10.3f} {w['var_pass_ms']:>9.3f}   "
              f"{ks}   ws {w['workspace_bytes'] / 2**20:.1f} MiB")
    for w in rows:
        print(json.dumps(w))


if __name__ == "__main__":
    main()
