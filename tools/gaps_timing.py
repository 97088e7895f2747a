"""Cost of smoothing through missing observations (eks_smooth_gaps) beside the
closest existing route, ``batch.smooth(want_var=True)`` on the same data
without gaps.

    python tools/gaps_timing.py [--reps 15] [--warmup 3] [--shapes c2 c3 c4] [--chunk 0 32 64]

For each shape -- config 2 (17 x 100 000, (r, n) = (2, 2)), config 3
(17 x 50 000, (3, 8)) and config 4's 128-video shard (2176 x 10 000, (2, 2)),
E = 5 float32 members, time-major -- the models are fitted on the complete
members (eks_fit); then 10 % of the entries, at random, and one 100-frame hole
per trajectory get a NaN in member 0.  It prints the median time of
``batch.smooth(want_var=True)`` on the complete members, of
``batch.smooth_gaps(want_var=True, want_nll=True)`` on the members with gaps,
the five kernels of that call separately (eks_profile_begin / _end events
around each launch) and its workspace size.  Times are device events around
the calls after warm-up.  ``--chunk`` repeats every shape with forced chunk
lengths (EKS_DBG_GAPS_CHUNK; 0 = automatic).  One JSON line per row follows
the table.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pvar_timing import SHAPES, members, timed  # noqa: E402


def with_gaps(torch, obs, frac=0.1, hole=100, seed=1):
    """A copy of the (B, T, E, n) member view (same time-major layout) whose
    member 0 is NaN on ``frac`` of the (b, t, j) entries and on ``hole``
    frames of every trajectory."""
    B, T, E, n = obs.shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    # (T, E, n, B); clone: .contiguous() of a time-major view is the view itself
    tm = obs.permute(1, 2, 3, 0).clone(memory_format=torch.contiguous_format)
    miss = torch.rand((T, n, B), generator=g, device="cuda") < frac
    start = torch.randint(0, max(T - hole, 1), (B,), generator=g, device="cuda")
    t = torch.arange(T, device="cuda").unsqueeze(1)
    miss |= ((t >= start) & (t < start + hole)).unsqueeze(1)
    tm[:, 0][miss] = float("nan")
    return tm.permute(3, 0, 1, 2), int(miss.sum().item())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--chunk", nargs="+", type=int, default=[0],
                    help="chunk lengths of eks_smooth_gaps to time (0 = automatic)")
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
        gobs, n_missing = with_gaps(torch, obs)
        route = lambda: batch.smooth(obs, params, n=n, r=r, flags=flags, want_var=True)  # noqa: E731
        gaps = lambda: batch.smooth_gaps(gobs, params, n=n, r=r, want_var=True,  # noqa: E731
                                         want_nll=True)
        route_ms = timed(torch, route, a.reps, a.warmup)
        for chunk in a.chunk:
            _lib.debug_set(_lib.EKS_DBG_GAPS_CHUNK, chunk)
            res = gaps()
            assert int(res["status"].abs().sum()) == 0, "status bits set"
            assert bool(torch.isfinite(res["out"]).all()) and bool(torch.isfinite(res["var"]).all())
            assert int(res["nobs"].sum().item()) == B * T * n - n_missing
            row = dict(shape=name, B=B, T=T, n=n, r=r, missing=n_missing / (B * T * n),
                       chunk_len=int(lib.eks_smooth_gaps_chunk_len(B, T, r)),
                       workspace_bytes=int(lib.eks_smooth_gaps_workspace_bytes(B, T, n, r)),
                       smooth_want_var_ms=route_ms,
                       smooth_gaps_ms=timed(torch, gaps, a.reps, a.warmup))
            _lib.profile_begin(a.reps + 1)
            for _ in range(a.reps):
                gaps()
            torch.cuda.synchronize()
            row["kernels_ms"] = {k: v / a.reps for k, v in _lib.profile_end()}
            rows.append(row)
        _lib.debug_set(_lib.EKS_DBG_GAPS_CHUNK, 0)
        del obs, gobs
    report(rows)


def report(rows):
    print(f"{'shape':6}{'B':>6}{'T':>8} (r,n)  {'L':>4} {'smooth+var':>11} {'smooth_gaps':>12} "
          f"{'ratio':>6}   kernels of eks_smooth_gaps (ms)")
    for w in rows:
        ks = "  ".join(f"{k[5:]} {v:.3f}" for k, v in w["kernels_ms"].items())
        print(f"{w['shape']:6}{w['B']:>6}{w['T']:>8} ({w['r']},{w['n']})  {w['chunk_len']:>4} "
              f"{w['smooth_want_var_ms']:>11.3f} {w['smooth_gaps_ms']:>12.3f} "
              f"{w['smooth_gaps_ms'] / w['smooth_want_var_ms']:>6.2f}   "
              f"{ks}   ws {w['workspace_bytes'] / 2**20:.1f} MiB")
    for w in rows:
        print(json.dumps(w))


if __name__ == "__main__":
    main()
