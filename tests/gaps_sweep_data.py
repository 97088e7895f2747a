"""Inputs and references of the gap-aware likelihood sweep
(test_gaps_sweep_host.py, test_gpu_gaps_sweep.py): computed once per case and
shared, read only.

A case is members with gaps (gaps_ref.knock_out: member 0 of every masked
(b, t, j) is NaN), the models of the complete data, and the NLL of
gaps_ref.dense for every (candidate, trajectory), the candidates being the
models with Q scaled by sweep_data.SCALES.

``chunked_sweep`` is a numpy model of the device algorithm
(eks_amd/csrc/gap_sweep.hpp): the information-form sums once per trajectory,
then per candidate the chunk elements (absorb), the prefix over them
(compose_elem), and the NLL shares of the filter re-run from the entering
states (filter_step), added in ascending chunk order.
"""
import functools

import numpy as np

import gaps_ref as G
import sweep_data as D

SCALES = D.SCALES
KEYS = ("m0", "S0", "A", "Q", "C", "means")


def scaled(p, s):
    """The model ``p`` with Q scaled by s."""
    q = {k: p[k] for k in KEYS}
    q["Q"] = s * p["Q"]
    return q


def dense_table(g, cands, mode="median"):
    """NLL (K, B) and nobs (B,) of gaps_ref.dense; cands[k][b] is candidate k
    of trajectory b, g the members (B, E, T, n) with gaps."""
    B = g.shape[0]
    ref = np.zeros((len(cands), B))
    nobs = np.zeros(B, dtype=np.int64)
    for b in range(B):
        y, ev = G.ensemble(g[b], mode)
        for k, ms in enumerate(cands):
            res = G.dense(y, ev, ms[b])
            ref[k, b] = res["nll"]
            nobs[b] = res["nobs"]
    return ref, nobs


def scale_candidates(models, scales=SCALES):
    return [[scaled(m, s) for m in models] for s in scales]


def rows_of(cands):
    """cands[k][b] as numpy (K * B, P) rows: row k * B + b = candidate k of trajectory b."""
    return np.stack([G.pack(m) for ms in cands for m in ms])


def _case(g, models, mask):
    ref, nobs = dense_table(g, scale_candidates(models))
    for a in (g, mask, ref, nobs):
        a.setflags(write=False)
    return dict(g=g, models=models, mask=mask, ref=ref, nobs=nobs)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(g (B, E, T, n), models, mask (B, T, n), ref (K, B), nobs (B,)).

    sv131     gaps_ref.case_sv131: (2,2), B = 3, 20 % gaps, 40-frame voids
    mc131     (3,8), B = 3, the masks of test_gpu_gaps.multicam_gaps: whole
              cameras missing, 2 observations for r = 3, a 10-frame void
    mc300     n = 10 (five cameras), B = 2, T = 300, 20 % gaps, four cameras
              out over 40 frames
    pupil131  (3,8) pupil, B = 2, a 20-frame blink and 20 % gaps
    sv2100    (2,2), B = 2, test_gpu_gaps.test_singleview_wave_scan's mask
    """
    if name == "sv131":
        g, models, _, mask = G.case_sv131()
        return _case(np.array(g), models, mask.copy())
    if name == "mc131":
        from test_gpu_gaps import multicam_gaps
        g, models, mask = multicam_gaps()
        return _case(g, models, mask)
    if name == "mc300":
        st = G.members("mc", 2, 300, V=5)
        models = [G.model_of("mc", st[b]) for b in range(2)]
        mask = np.random.default_rng(10).random((2, 300, 10)) < 0.2
        mask[0, 100:140, :8] = True
        return _case(G.knock_out(st, mask), models, mask)
    if name == "pupil131":
        st, models = pupil_complete(), D.dataset("pupil", 2, 131)[1]
        models = [{k: m[k] for k in KEYS} for m in models]
        mask = np.random.default_rng(131).random((2, 131, 8)) < 0.2
        mask[0, 40:60] = True
        return _case(G.knock_out(st, mask), models, mask)
    if name == "sv2100":
        st = G.members("sv", 2, 2100)
        models = [G.model_of("sv", st[b]) for b in range(2)]
        mask = np.random.default_rng(2100).random((2, 2100, 2)) < 0.2
        mask[0, 1000:1040] = True
        mask[:, 0] = True
        mask[:, -1] = True
        return _case(G.knock_out(st, mask), models, mask)
    raise KeyError(name)


def pupil_complete():
    """The members of pupil131 without gaps (B, E, T, 8)."""
    return D.dataset("pupil", 2, 131)[0].astype(np.float32).astype(np.float64)


def pupil_grid_candidates(st, grid):
    """cands[k][b]: the pupil model of complete members st (B, E, T, 8) at
    A = diag(d, c, c) for every (d, c) of the grid."""
    return [[{k: D.model_of("pupil", st[b], A=(d, c, c))[k] for k in KEYS}
             for b in range(st.shape[0])] for d, c in grid]


def chunked_sweep(y, ev, cands, L):
    """The NLL of every candidate model of one trajectory by the device
    algorithm with chunks of L steps (L >= T: the sequential form)."""
    T = y.shape[0]
    r = cands[0]["m0"].shape[0]
    W, w, kap = G.info_sums(y, ev, cands[0])  # C and offset are candidate 0's
    NC = (T + L - 1) // L
    bounds = [(c * L, min(T, (c + 1) * L)) for c in range(NC)]
    out = []
    for p in cands:
        m0, S0, A, Q = p["m0"], p["S0"], p["A"], p["Q"]
        elems = []
        for c, (s, e) in enumerate(bounds):
            if c == 0:
                E = (np.zeros((r, r)), m0.copy(), S0.copy(), np.zeros(r), np.zeros((r, r)))
            else:
                E = (np.eye(r), np.zeros(r), np.zeros((r, r)), np.zeros(r), np.zeros((r, r)))
            for t in range(s, e):
                E = G.absorb(E, t > 0, A, Q, W[t], w[t])
            elems.append(E)
        enter = [(m0, S0)]
        X = elems[0]
        for c in range(1, NC):
            enter.append((X[1], X[2]))
            X = G.compose_elem(X, elems[c])
        nll = 0.0
        for c, (s, e) in enumerate(bounds):
            m, P = enter[c]
            share = 0.0
            for t in range(s, e):
                m, P, sh = G.filter_step(t, A, Q, W[t], w[t], kap[t], m, P)
                share += sh
            nll += share
        out.append(nll)
    return np.array(out)
