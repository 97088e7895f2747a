"""Cost of the model fit through missing observations (eks_fit_gaps) beside
the fit on the same shape without gaps and beside the host route.

    python tools/fit_gaps_timing.py [--reps 15] [--warmup 3] [--host-reps 3] [--shapes c2 c3 c4]

For each shape -- config 2 (17 x 100 000, (r, n) = (2, 2)), config 3
(17 x 50 000, (3, 8)) and config 4's 128-video shard (2176 x 10 000, (2, 2)),
E = 5 float32 members, time-major -- 10 % of the entries, at random, and one
100-frame hole per trajectory get a NaN in member 0 (tools/gaps_timing.py
with_gaps).  It prints the median time of ``batch.fit_gaps`` on the members
with gaps, of its selection kernel alone (eks_profile_begin / _end events
around each launch; the other kernels of the call follow), of
``batch.fit(keep_yev=True)`` on the members without gaps -- the yardstick:
the same worst pass, accumulation, merge and final kernels around eks_fit's
own selection -- and of the host route the wrappers take with
``allow_missing=True``: the ensemble on the device, a copy to the host, and
``fit.singleview_model`` / ``fit.multicam_model`` on the complete frames of
one trajectory after the other (wall clock, ``--host-reps`` runs).  Device
times are events around the calls after warm-up.  One JSON line per row
follows the table.
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

from tools.gaps_timing import with_gaps  # noqa: E402
from tools.pvar_timing import SHAPES, members, timed  # noqa: E402


def host_route(torch, gobs, kind, s, q):
    """The wrappers' fit with allow_missing=True for every trajectory."""
    from eks_amd import fit
    from eks_amd.smoothers import _complete_frames
    import eks_amd.ops  # noqa: F401
    preds, ev = torch.ops.eks.ensemble(gobs, "median")
    preds, ev = preds.cpu().numpy(), ev.cpu().numpy()
    f = fit.singleview_model if kind == "singleview" else fit.multicam_model
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b in range(preds.shape[0]):
            ok = _complete_frames(preds[b], ev[b])
            f(preds[b][ok], ev[b][ok], s, q)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    a = ap.parse_args(argv)
    from eks_amd import _lib, batch
    torch = _lib.require_gpu()
    lib = _lib.load()
    rows = []
    for name in a.shapes:
        B, T, n, r, kind = SHAPES[name]
        obs = members(torch, B, T, n)
        gobs, n_missing = with_gaps(torch, obs)
        s, q = (10.0, 50.0) if r == 2 else (0.01, 25.0)
        kw = dict(kind=kind, n=n, r=r, smooth_param=s, quantile_keep=q)
        yev = batch.fit(obs, keep_yev=True, **kw)[2]
        res = batch.fit_gaps(gobs, keep_yev=yev, **kw)
        assert int(res["status"].abs().sum()) == 0, "status bits set"
        assert bool(torch.isfinite(res["params"]).all())
        nc, nk = res["ncomplete"].double(), res["nkept"].double()
        fit_ms = timed(torch, lambda: batch.fit(obs, keep_yev=yev, check=False, **kw),
                       a.reps, a.warmup)
        gaps = lambda: batch.fit_gaps(gobs, keep_yev=yev, check=False, **kw)  # noqa: E731
        row = dict(shape=name, B=B, T=T, n=n, r=r, missing=n_missing / (B * T * n),
                   complete=float(nc.mean().item()) / T, kept=float(nk.mean().item()) / T,
                   workspace_bytes=int(lib.eks_fit_gaps_workspace_bytes(B, T, n)),
                   fit_keep_yev_ms=fit_ms, fit_gaps_ms=timed(torch, gaps, a.reps, a.warmup))
        _lib.profile_begin(a.reps + 1)
        for _ in range(a.reps):
            gaps()
        torch.cuda.synchronize()
        row["kernels_ms"] = {k: v / a.reps for k, v in _lib.profile_end()}
        _lib.profile_begin(a.reps + 1)
        for _ in range(a.reps):
            batch.fit(obs, keep_yev=yev, check=False, **kw)
        torch.cuda.synchronize()
        row["fit_kernels_ms"] = {k: v / a.reps for k, v in _lib.profile_end()}
        host = []
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_route(torch, gobs, kind, s, q)
            host.append((time.perf_counter() - t0) * 1e3)
        row["host_route_ms"] = statistics.median(host)
        rows.append(row)
        del obs, gobs, yev, res
    report(rows)


def report(rows):
    print(f"{'shape':6}{'B':>6}{'T':>8} (r,n) {'complete':>9} {'fit+yev':>8} {'fit_gaps':>9} "
          f"{'select':>7} {'host':>9}   kernels of eks_fit_gaps | of eks_fit (ms)")
    for w in rows:
        ks = "  ".join(f"{k[2:]} {v:.3f}" for k, v in w["kernels_ms"].items())
        kf = "  ".join(f"{k[2:]} {v:.3f}" for k, v in w["fit_kernels_ms"].items())
        sel = sum(v for k, v in w["kernels_ms"].items() if k == "k_fit_select_gaps")
        print(f"{w['shape']:6}{w['B']:>6}{w['T']:>8} ({w['r']},{w['n']}) {w['complete']:>9.3f} "
              f"{w['fit_keep_yev_ms']:>8.3f} {w['fit_gaps_ms']:>9.3f} {sel:>7.3f} "
              f"{w['host_route_ms']:>9.1f}   {ks} | {kf}")
    for w in rows:
        print(json.dumps(w))


if __name__ == "__main__":
    main()
