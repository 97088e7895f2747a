"""Cost of a joint posterior draw (eks_draws_gaps) beside one call of the
smoother it rides on (eks_smooth_gaps): is a draw cheaper than the smoother
call Matheron's rule would spend on it?

    python tools/draws_timing.py [--reps 9] [--warmup 2] [--shapes c2 c3] [--S 64]

For each shape -- config 2 (17 x 100 000 frames, (n, r) = (2, 2)) and config
3's model at the same length (17 x 100 000, (8, 3)), E = 5 float32 members,
time-major -- the models are fitted on the complete members (eks_fit); then
10 % of the entries, at random, and one 100-frame hole per trajectory get a NaN
in member 0 (tools/gaps_timing.py).  In one run it times, alternating,
``batch.smooth_gaps`` and ``batch.draws_gaps`` with S draws, seeded and from an
explicit noise tensor (``batch.draws_noise``, timed separately), and prints

    t_draw = (t(draws_gaps, S) - t(smooth_gaps)) / S
    ratio  = t_draw / t(smooth_gaps)          (must be < 1, expected << 1)
    GB/s   = the draw stage's bytes, counted from the shapes below, over
             t(draws_gaps, S) - t(smooth_gaps), against 6.3 TB/s achievable HBM

Times are device events around the calls after warm-up, the median of
``--reps`` rounds.  Bytes of the draw stage per call (kDrawTile = 4 draws per
lane, FL = r r + r (r + 1) / 2 factor doubles per step):
    D1      B T (r (r + 1) / 2 + FL) 8                    P_t in, factors out
    D2, D4  2 B T ceil(S / 4) FL 8 + B T ceil(S / 4) r 8   factors per tile, ms_t
    draws   B S T n 8 out;  explicit noise: 2 B S T r 8 in
One JSON line per row follows the table.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gaps_timing import with_gaps  # noqa: E402
from tools.pvar_timing import members  # noqa: E402

SHAPES = {"c2": (17, 100_000, 2, 2, "singleview"), "c3": (17, 100_000, 8, 3, "multicam")}
HBM_BYTES_PER_S = 6.3e12  # achievable (8.0e12 peak)
TILE = 4


def stage_bytes(B, S, T, n, r, explicit):
    fl = r * r + r * (r + 1) // 2
    tiles = -(-S // TILE)
    b = B * T * (r * (r + 1) // 2 + fl) * 8
    b += 2 * B * T * tiles * fl * 8 + B * T * tiles * r * 8
    b += B * S * T * n * 8
    if explicit:
        b += 2 * B * S * T * r * 8
    return b


def timed_round_robin(torch, fns, reps, warmup):
    """Median ms of every fn, the fns alternating inside each round."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ({k: statistics.median(v) for k, v in ms.items()},
            {k: (min(v), max(v)) for k, v in ms.items()})


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--S", type=int, default=64)
    a = ap.parse_args(argv)
    from eks_amd import _lib, batch
    torch = _lib.require_gpu()
    lib = _lib.load()
    S = a.S
    rows = []
    for name in a.shapes:
        B, T, n, r, kind = SHAPES[name]
        obs = members(torch, B, T, n)
        params, _ = batch.fit(obs, kind=kind, n=n, r=r, smooth_param=10.0 if r == 2 else 0.01,
                              quantile_keep=50.0 if r == 2 else 25.0)
        gobs, _ = with_gaps(torch, obs)
        del obs
        noise = batch.draws_noise(B, S, T, r, 1)
        fns = {
            "smooth_gaps": lambda: batch.smooth_gaps(gobs, params, n=n, r=r),
            "draws_seeded": lambda: batch.draws_gaps(gobs, params, n=n, r=r, S=S, seed=1),
            "draws_noise_given": lambda: batch.draws_gaps(gobs, params, n=n, r=r, noise=noise),
            "draws_noise": lambda: batch.draws_noise(B, S, T, r, 1),
        }
        res = fns["draws_seeded"]()
        assert int(res["status"].abs().sum()) == 0, "status bits set"
        assert bool(torch.isfinite(res["draws"]).all())
        same = bool(torch.equal(res["draws"], fns["draws_noise_given"]()["draws"]))
        print(f"[{name}] seeded draws equal the draws from draws_noise's tensor bit for bit: {same}")
        del res
        med, spread = timed_round_robin(torch, fns, a.reps, a.warmup)
        row = dict(shape=name, B=B, T=T, n=n, r=r, S=S,
                   chunk_len=int(lib.eks_draws_gaps_chunk_len(B, T, r)),
                   workspace_bytes=int(lib.eks_draws_gaps_workspace_bytes(B, S, T, n, r)),
                   ms=med, ms_min_max=spread)
        for mode, explicit in (("draws_seeded", False), ("draws_noise_given", True)):
            stage_ms = med[mode] - med["smooth_gaps"]
            nbytes = stage_bytes(B, S, T, n, r, explicit)
            row[mode] = dict(t_draw_ms=stage_ms / S, ratio=stage_ms / S / med["smooth_gaps"],
                             stage_bytes=nbytes, bytes_per_s=nbytes / (stage_ms * 1e-3),
                             hbm_share=nbytes / (stage_ms * 1e-3) / HBM_BYTES_PER_S)
        rows.append(row)
        del gobs, noise
    report(rows)


def report(rows):
    print(f"{'shape':6}{'B':>4}{'T':>8} (n,r) {'S':>4} {'L':>4} {'smooth_gaps':>12} "
          f"{'draws(S)':>10} {'t_draw':>8} {'ratio':>7} {'GB/s':>7} {'of HBM':>7}  mode")
    for w in rows:
        for mode in ("draws_seeded", "draws_noise_given"):
            d = w[mode]
            print(f"{w['shape']:6}{w['B']:>4}{w['T']:>8} ({w['n']},{w['r']}) {w['S']:>4} "
                  f"{w['chunk_len']:>4} {w['ms']['smooth_gaps']:>12.3f} {w['ms'][mode]:>10.3f} "
                  f"{d['t_draw_ms']:>8.4f} {d['ratio']:>7.4f} {d['bytes_per_s'] / 1e9:>7.0f} "
                  f"{d['hbm_share']:>7.1%}  {mode[6:]}")
        print(f"{'':6}draws_noise alone {w['ms']['draws_noise']:.3f} ms, workspace "
              f"{w['workspace_bytes'] / 2**20:.1f} MiB")
    for w in rows:
        print(json.dumps(w))


if __name__ == "__main__":
    main()
