"""Cost of the likelihood sweep through missing observations
(eks_nll_sweep_gaps) beside the two routes it replaces or parallels.

    python tools/gaps_sweep_timing.py [--reps 15] [--warmup 3] [--shapes c2 c3 c4 pupil]
                                      [--chunk 0 32 64]

Shapes, E = 5 float32 members, time-major: config 2 (17 x 100 000, (r, n) =
(2, 2), K = 16), config 3 (17 x 50 000, (3, 8), K = 16), config 4's 128-video
shard (2176 x 10 000, (2, 2), K = 8) and one pupil video of 1 000 000 frames
((3, 8), K = 64: an 8 x 8 grid of (diameter_s, com_s), the candidates differ in
A and Q).  The models are fitted on the complete members (eks_fit; the pupil
model on the host); then 20 % of the entries, at random, and one 40-frame void
per trajectory get a NaN in member 0.  It prints the median time of

  * ``batch.nll_sweep_gaps`` on the members with gaps (check=False: no host
    round trip), and its kernels separately (eks_profile_begin / _end events
    around each launch);
  * K back-to-back ``batch.smooth_gaps(want_nll=True)`` calls on the same
    candidates: the only gap-aware NLL without the sweep, the yardstick;
  * ``batch.nll_sweep`` on the same members without gaps: what a complete
    data set pays,

the largest relative difference between the first two routes' NLLs, the
workspace size and the plane bytes a candidate reads per step, (Sym + r)
doubles in k_gs_elem and (Sym + r + 1) in k_gs_share (nll_sweep reads
r (r + 3) / 2 doubles once).  Times are device events around the calls after
warm-up.  ``--chunk`` repeats every shape with forced chunk lengths
(EKS_DBG_GAPS_SWEEP_CHUNK; 0 = automatic).  One JSON line per row follows the
table.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gaps_timing import with_gaps  # noqa: E402
from tools.pvar_timing import members, timed  # noqa: E402

SHAPES = {"c2": (17, 100_000, 2, 2, "singleview", 16), "c3": (17, 50_000, 8, 3, "multicam", 16),
          "c4": (2176, 10_000, 2, 2, "singleview", 8), "pupil": (1, 1_000_000, 8, 3, "pupil", 64)}


def make_case(torch, name):
    """(members (B, T, E, n) view, candidate rows (K, B, P)) of a shape."""
    import numpy as np
    from eks_amd import batch
    B, T, n, r, kind, K = SHAPES[name]
    if kind == "pupil":
        from eks_amd import fit, synthetic
        st = synthetic.pupil_obs(np.random.default_rng(0), 5, T)  # (E, T, 8)
        obs = batch.make_time_major(st[None], dtype=np.float32)
        preds = np.median(st.astype(np.float64), axis=0)
        grid = 1.0 - 10.0 ** np.linspace(-4, -1, 8)
        base = fit.pupil_model(preds, np.eye(3))
        var = np.diag(base["S0"])
        # (pupil_model's A and Q at every grid point; the rest does not depend on A)
        models = [dict(base, A=np.diag([d, c, c]), Q=np.diag(var * (1 - np.array([d, c, c]) ** 2)))
                  for d in grid for c in grid]
        stk = lambda k: np.stack([m[k] for m in models])  # noqa: E731
        cand = batch.pack_params(stk("m0"), stk("S0"), stk("A"), stk("Q"), stk("C"), stk("offset"))
        return obs, cand.view(K, B, -1)
    obs = members(torch, B, T, n)
    params, _ = batch.fit(obs, kind=kind, n=n, r=r, smooth_param=1.0,
                          quantile_keep=50.0 if r == 2 else 25.0)
    s = 10.0 ** torch.linspace(-3, 3, K, dtype=torch.float64, device="cuda")
    return obs, batch.scale_q(params, s.unsqueeze(1).expand(K, B), r=r).contiguous()


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
        obs, cand = make_case(torch, name)
        flat = cand.view(K * B, -1)
        gobs, n_missing = with_gaps(torch, obs, frac=0.2, hole=40)

        def k_calls():
            return torch.stack([batch.smooth_gaps(gobs, cand[k], n=n, r=r, want_nll=True)["nll"]
                                for k in range(K)])

        def sweep():
            return batch.nll_sweep_gaps(gobs, flat, K=K, n=n, r=r, check=False)

        def complete():
            return batch.nll_sweep(obs, flat, K=K, n=n, r=r, check=False)

        ref = k_calls()
        calls_ms = timed(torch, k_calls, a.reps, a.warmup)
        complete_ms = timed(torch, complete, a.reps, a.warmup)
        sym = r * (r + 1) // 2
        for chunk in a.chunk:
            _lib.debug_set(_lib.EKS_DBG_GAPS_SWEEP_CHUNK, chunk)
            res = sweep()
            assert int(res["status"].abs().sum()) == 0, "status bits set"
            assert int(res["nobs"].sum().item()) == B * T * n - n_missing
            row = dict(shape=name, B=B, T=T, n=n, r=r, K=K, missing=n_missing / (B * T * n),
                       chunk_len=int(lib.eks_nll_sweep_gaps_chunk_len(B, K, T, r)),
                       workspace_bytes=int(lib.eks_nll_sweep_gaps_workspace_bytes(B, K, T, n, r)),
                       plane_bytes_per_candidate_step=8 * (2 * sym + 2 * r + 1),
                       nll_sweep_bytes_per_candidate_step=8 * (r * (r + 3) // 2),
                       max_rel_diff=float(((res["nll"] - ref).abs() / ref.abs()).max()),
                       k_calls_ms=calls_ms, nll_sweep_complete_ms=complete_ms,
                       sweep_ms=timed(torch, sweep, a.reps, a.warmup))
            _lib.profile_begin(a.reps + 1)
            for _ in range(a.reps):
                sweep()
            torch.cuda.synchronize()
            row["kernels_ms"] = {k: v / a.reps for k, v in _lib.profile_end()}
            rows.append(row)
        _lib.debug_set(_lib.EKS_DBG_GAPS_SWEEP_CHUNK, 0)
        del obs, gobs
    report(rows)


def report(rows):
    print(f"{'shape':6}{'B':>6}{'T':>8} (r,n) {'K':>3} {'L':>5} {'K x gaps':>9} {'sweep':>9} "
          f"{'ratio':>6} {'nll_sweep':>10} {'to it':>6} {'max rel':>9}   kernels of the sweep (ms)")
    for w in rows:
        ks = "  ".join(f"{k[5:]} {v:.3f}" for k, v in w["kernels_ms"].items())
        print(f"{w['shape']:6}{w['B']:>6}{w['T']:>8} ({w['r']},{w['n']}) {w['K']:>3} "
              f"{w['chunk_len']:>5} {w['k_calls_ms']:>9.3f} {w['sweep_ms']:>9.3f} "
              f"{w['k_calls_ms'] / w['sweep_ms']:>6.2f} {w['nll_sweep_complete_ms']:>10.3f} "
              f"{w['sweep_ms'] / w['nll_sweep_complete_ms']:>6.2f} {w['max_rel_diff']:>9.2e}   "
              f"{ks}   ws {w['workspace_bytes'] / 2**20:.1f} MiB")
    for w in rows:
        print(json.dumps(w))


if __name__ == "__main__":
    main()
