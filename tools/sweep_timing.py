"""Cost of the likelihood sweep (eks_nll_sweep) beside K filter-only calls.

    python tools/sweep_timing.py [--reps 15] [--warmup 3] [--shapes c2 c3 c4] [--chunk 0 16 32]

For each shape -- config 2 (17 x 100 000, (r, n) = (2, 2), K = 16), config 3
(17 x 50 000, (3, 8), K = 16) and config 4's 128-video shard (2176 x 10 000,
(2, 2), K = 8), E = 5 float32 members, time-major -- it prints the median time
of ``batch.nll_sweep`` (check=False: no host round trip), of K back-to-back
``batch.nll`` calls on the same candidates (the only route without the sweep:
the yardstick), the sweep's kernels separately (eks_profile_begin / _end
events around each launch), its workspace size and the largest relative
difference between the two routes' NLLs.  Times are device events around the
calls after warm-up; members are generated and the models fitted (eks_fit,
smooth_param = 1) on the device, the candidates are Q x 10 ** linspace(-3, 3, K).
``--chunk`` repeats every shape with forced chunk lengths
(EKS_DBG_SWEEP_CHUNK; 0 = automatic).  One JSON line per row follows the table.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pvar_timing import members, timed  # noqa: E402

SHAPES = {"c2": (17, 100_000, 2, 2, "singleview", 16), "c3": (17, 50_000, 8, 3, "multicam", 16),
          "c4": (2176, 10_000, 2, 2, "singleview", 8)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--chunk", nargs="+", type=int, default=[0],
                    help="chunk lengths of the sweep to time (0 = automatic)")
    a = ap.parse_args(argv)
    from eks_amd import _lib, batch
    torch = _lib.require_gpu()
    lib = _lib.load()
    rows = []
    for name in a.shapes:
        B, T, n, r, kind, K = SHAPES[name]
        obs = members(torch, B, T, n)
        params, _ = batch.fit(obs, kind=kind, n=n, r=r, smooth_param=1.0,
                              quantile_keep=50.0 if r == 2 else 25.0)
        s = 10.0 ** torch.linspace(-3, 3, K, dtype=torch.float64, device="cuda")
        cand = batch.scale_q(params, s.unsqueeze(1).expand(K, B), r=r).contiguous()
        flat = cand.view(K * B, -1)
        flags = _lib.EKS_MODEL_A_IDENTITY | (_lib.EKS_MODEL_C_IDENTITY if r == n else 0)

        def k_calls():
            return torch.stack([batch.nll(obs, cand[k], n=n, r=r, flags=flags, check=False)
                                for k in range(K)])

        def sweep():
            return batch.nll_sweep(obs, flat, K=K, n=n, r=r, check=False)

        ref = k_calls()
        calls_ms = timed(torch, k_calls, a.reps, a.warmup)
        for chunk in a.chunk:
            _lib.debug_set(_lib.EKS_DBG_SWEEP_CHUNK, chunk)
            status = torch.empty((K, B), dtype=torch.int32, device="cuda")
            got = batch.nll_sweep(obs, flat, K=K, n=n, r=r, check=False, status=status)
            assert int(status.abs().sum()) == 0, "status bits set"
            row = dict(shape=name, B=B, T=T, n=n, r=r, K=K,
                       chunk_len=int(lib.eks_nll_sweep_chunk_len(B, K, T, r)),
                       workspace_bytes=int(lib.eks_nll_sweep_workspace_bytes(B, K, T, n, r)),
                       nll_workspace_bytes=int(lib.eks_smooth_workspace_bytes(B, T, n, r, 5, 0)),
                       max_rel_diff=float(((got - ref).abs() / ref.abs()).max()),
                       k_calls_ms=calls_ms, sweep_ms=timed(torch, sweep, a.reps, a.warmup))
            _lib.profile_begin(a.reps + 1)
            for _ in range(a.reps):
                sweep()
            torch.cuda.synchronize()
            row["kernels_ms"] = {k: v / a.reps for k, v in _lib.profile_end()}
            rows.append(row)
        _lib.debug_set(_lib.EKS_DBG_SWEEP_CHUNK, 0)
        del obs
    report(rows)


def report(rows):
    print(f"{'shape':6}{'B':>6}{'T':>8} (r,n) {'K':>3} {'L':>4} {'K x nll':>9} {'sweep':>9} "
          f"{'ratio':>6} {'max rel':>9}   kernels of the sweep (ms)")
    for w in rows:
        ks = "  ".join(f"{k[5:]} {v:.3f}" for k, v in w["kernels_ms"].items())
        print(f"{w['shape']:6}{w['B']:>6}{w['T']:>8} ({w['r']},{w['n']}) {w['K']:>3} "
              f"{w['chunk_len']:>4} {w['k_calls_ms']:>9.3f} {w['sweep_ms']:>9.3f} "
              f"{w['k_calls_ms'] / w['sweep_ms']:>6.2f} {w['max_rel_diff']:>9.2e}   "
              f"{ks}   ws {w['workspace_bytes'] / 2**20:.1f} MiB")
    for w in rows:
        print(json.dumps(w))


if __name__ == "__main__":
    main()
