"""Cost of the ensemble over the valid members (eks_ensemble_gaps) beside the
fit's worst pass (k_fit_worst), which reads the same members with the same
lanes.

    python tools/ensemble_gaps_timing.py [--reps 15] [--warmup 3] [--shapes c4 long] [--shard 1]

Shapes: config 4 (17 408 x 10 000, E = 5, n = 2; ``--shard k`` takes 1 / k of
its trajectories) and 17 x 100 000 with n = 8, float32 members, time-major.
Each is timed without gaps and with 20 % of the members NaN, min_members = 3:
the median of ``batch.ensemble_gaps`` (events around the call after warm-up,
with and without the nvalid plane) and its kernel alone (eks_profile_begin /
_end), in ms and in effective TB/s over the bytes the kernel has to move,
E n 4 read and 16 n (+ n) written per frame.  ``batch.fit_gaps`` on the same
members in the same session gives k_fit_worst's time; its bytes are E n 4
read and 8 + 12 n written per frame (the worst row, float32 y and float64 ev
planes).  One JSON line per row follows the table.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pvar_timing import members, timed  # noqa: E402

SHAPES = {"c4": (17_408, 10_000, 2, 2, "singleview"), "long": (17, 100_000, 8, 3, "multicam")}
E = 5


def kernel_ms(torch, _lib, fn, reps, name):
    _lib.profile_begin(reps + 1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return {k: v / reps for k, v in _lib.profile_end()}[name]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--shard", type=int, default=1, help="1 / shard of config 4's trajectories")
    a = ap.parse_args(argv)
    from eks_amd import _lib, batch
    torch = _lib.require_gpu()
    rows = []
    for name in a.shapes:
        B, T, n, r, kind = SHAPES[name]
        if name == "c4":
            B //= a.shard
        obs = members(torch, B, T, n, E=E)
        frames = B * T
        kw = dict(kind=kind, n=n, r=r, smooth_param=10.0 if r == 2 else 0.01,
                  quantile_keep=50.0 if r == 2 else 25.0, check=False)
        fitted = batch.fit_gaps(obs, **kw)
        fit_yev = fitted["yev"]
        worst = kernel_ms(torch, _lib, lambda: batch.fit_gaps(obs, keep_yev=fit_yev, **kw),
                          a.reps, "k_fit_worst")
        worst_bytes = frames * (E * n * 4 + 8 + 12 * n)
        del fitted, fit_yev
        for label, frac in (("no gaps", 0.0), ("20 % NaN", 0.20)):
            if frac:
                g = torch.Generator(device="cuda").manual_seed(1)
                base = obs.permute(1, 2, 3, 0)  # the (T, E, n, B) buffer
                base.masked_fill_(torch.rand(base.shape, generator=g, device="cuda") < frac,
                                  float("nan"))
            res = batch.ensemble_gaps(obs, n=n, min_members=3, want_nvalid=True)
            yev = res["yev"]
            valid = float((res["nvalid"] >= 3).double().mean().item())
            del res
            run = lambda nv=False: batch.ensemble_gaps(obs, n=n, min_members=3,  # noqa: E731
                                                       want_nvalid=nv, keep_yev=yev)
            nbytes = frames * (E * n * 4 + 16 * n)
            k = kernel_ms(torch, _lib, run, a.reps, "k_ens_gaps")
            row = dict(shape=name, input=label, B=B, T=T, E=E, n=n, observed=valid,
                       call_ms=timed(torch, run, a.reps, a.warmup),
                       call_nvalid_ms=timed(torch, lambda: run(True), a.reps, a.warmup),
                       kernel_ms=k, tbps=nbytes / k / 1e9, bytes_per_frame=E * n * 4 + 16 * n,
                       k_fit_worst_ms=worst, k_fit_worst_tbps=worst_bytes / worst / 1e9)
            row["ratio_to_fit_worst"] = row["tbps"] / row["k_fit_worst_tbps"]
            rows.append(row)
            del yev
        del obs
    report(rows)


def report(rows):
    print(f"{'shape':6}{'input':>9}{'B':>7}{'T':>8} (E,n) {'observed':>9} {'call':>8} {'+nvalid':>8} "
          f"{'kernel':>8} {'TB/s':>6} | {'fit_worst':>9} {'TB/s':>6} {'ratio':>6}")
    for w in rows:
        print(f"{w['shape']:6}{w['input']:>9}{w['B']:>7}{w['T']:>8} ({w['E']},{w['n']}) "
              f"{w['observed']:>9.3f} {w['call_ms']:>8.3f} {w['call_nvalid_ms']:>8.3f} "
              f"{w['kernel_ms']:>8.3f} {w['tbps']:>6.2f} | {w['k_fit_worst_ms']:>9.3f} "
              f"{w['k_fit_worst_tbps']:>6.2f} {w['ratio_to_fit_worst']:>6.2f}")
    for w in rows:
        print(json.dumps(w))


if __name__ == "__main__":
    main()
