"""Exact observations (columns whose members all agree: ev == 0, a zero on
R_t's diagonal) placed on the chunk grids of the time-parallel smoothers, and
the host-side references that go with them.

``build`` takes (B, E, T, n) float64 members (tests/test_gpu_ragged._members)
and makes chosen (b, t, column) entries agree across the members.  Where the
entries go is computed from a *grid* (``plan_grid``: L and LS of algo 2,
algo 3's fine chunk and its two unit lengths, all read from
eks_smooth_plan_info), never from literals, so a retuning of the chunk plans
moves the frames with it.

Contract of every pattern (asserted by ``check_invariants`` on every build):
  * a frame holds at most r exact columns (more is the reference's singular
    S: that input has no reference and is not used),
  * with ``pupil=True`` a frame never holds both columns of a folded pair,
  * trajectory 0, trajectories 63 and 64 and the last one are never changed.

The agreed value is member 0's, rounded to float32: E equal float32 values
sum exactly in float64, so np.var -- and with it oracle.ensemble_array -- is
exactly 0 there for every E, also for the float64 member sources.

Also here: the oracle's filter / RTS / NLL recursions in any numpy float type
(``reference``; np.longdouble with a small pivoted elimination is the
yardstick of tests/test_exact_host.py), and a numpy model of the device's
filtering element (``elem``, ``compose_state``: kf_steps.hpp absorb_scalar /
elem_absorb / compose_state) that pins where the scan may break down.
"""
import itertools
import math

import numpy as np

PATTERNS = ("first", "last", "ckpt", "unit", "tail", "full_rank", "run", "cycle", "agree", "ulp")
PUPIL_PAIRS = ((0, 2), (5, 7))
# pupil column order for the patterns: folded columns first, so that the
# one-column patterns land on them (one column per frame keeps the pair rule)
PUPIL_COLS = (7, 0, 2, 5, 1, 3, 4, 6)
LOG_2PI = math.log(2.0 * math.pi)


# ---------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------
def plan_grid(B, T, n, r, E, smoothing=True, algo3=True):
    """The chunk grids of a (B, T, n, r, E) call, from eks_smooth_plan_info:
    L, LS (algo 2), F = fine_len3, U = k3_bwd's unit (4 fine chunks) and UF =
    k3_fwd's unit (8 fine chunks at r = 2) in steps.  ``algo3=False`` (filter
    only calls, the runtime-n kernels): the L grid alone."""
    from eks_amd import _lib
    p2 = _lib.plan_info(B, T, n, r, E, 2, smoothing=smoothing)
    assert p2["algo"] == 2 and p2["NC"] > 1, p2
    g = dict(T=T, L=p2["L"], LS=p2["LS"], F=None, U=None, UF=None)
    if algo3:
        p3 = _lib.plan_info(B, T, n, r, E, 3)
        assert p3["algo"] == 3 and p3["NCc"] == -(-p3["NCf"] // 4), p3
        kpu = [k for k in (4, 8) if p3["NCu"] == -(-p3["NCf"] // k)]
        assert len(kpu) == 1, p3        # T long enough to tell the two unit sizes apart
        g.update(F=p3["fine_len3"], U=4 * p3["fine_len3"], UF=kpu[0] * p3["fine_len3"])
    return g


def clean_rows(B):
    """Trajectories no pattern changes: they show that no flag leaks."""
    return {b for b in (0, 63, 64, B - 1) if 0 <= b < B}


def _bases(B, njobs):
    """[(first trajectory, width)]: each base hosts the pattern's jobs on
    ``width`` consecutive changeable trajectories (jobs fold onto them when
    there are fewer), in the first wave, past lane 64 and near the end."""
    clean = clean_rows(B)
    out = []
    for base in (1, 65, B - 1 - njobs):
        if base < 1 or any(abs(base - b0) < njobs for b0, _ in out):
            continue
        w = 0
        while w < njobs and base + w < B and base + w not in clean:
            w += 1
        if w:
            out.append((base, w))
    assert out, (B, njobs)
    return out


def mid(step, T):
    """A multiple of ``step`` near T / 2 that begins a chunk >= 1."""
    t = max(1, (T // 2) // step) * step
    assert step <= t < T, (step, T)
    return t


def best_columns(C, r):
    """The r rows of C with the smallest condition number: r exact columns pin
    the state down to C[cols]^-1 y, so nearly dependent rows are the
    reference's singular S in the limit (see check_conditioning)."""
    C = np.asarray(C)
    if C.shape[0] == r:
        return tuple(range(r))
    return min(itertools.combinations(range(C.shape[0]), r),
               key=lambda s: np.linalg.cond(C[list(s)]))


def pattern_jobs(pattern, g, r, cols, rcols=None):
    """The pattern as a list of jobs, one trajectory each where there is room:
    a job is a list of (t, columns).  ``rcols``: the columns of the patterns
    that make r columns exact at once (default: the first r of ``cols``)."""
    T, L, LS, F = g["T"], g["L"], g["LS"], g["F"]
    col = lambda i: [cols[(i + 1) % len(cols)]]  # noqa: E731  one column, varied over the jobs
    rcols = list(rcols) if rcols is not None else list(cols[:r])
    assert len(rcols) == r
    steps = [L] + ([F] if F and F != L else [])
    if pattern == "first":
        m = L * F // math.gcd(L, F) if F else L
        ts = [mid(m, T)] if m < T else [mid(s, T) for s in steps]
        return [[(t, col(i))] for i, t in enumerate(ts)]
    if pattern == "last":
        ts = sorted({mid(s, T) - 1 for s in steps})
        return [[(t, col(i))] for i, t in enumerate(ts)]
    if pattern == "ckpt":
        s = mid(L, T)
        t0 = s + LS * max(1, (L // LS) // 2)
        assert s <= t0 - 1 and t0 + 1 < min(s + L, T) and t0 % LS == 0, (g, t0)
        return [[(t0 - 1, col(0)), (t0, col(0)), (t0 + 1, col(0))]]
    if pattern == "unit":
        k = max(1, (T // 2) // g["U"])
        k -= 1 if k % 2 == 0 else 0     # an odd multiple: a 4-chunk boundary that is no 8-chunk one
        us = sorted({u for u in (k * g["U"], max(1, (T // 2) // g["UF"]) * g["UF"]) if u < T})
        assert us, g
        return [[(u - 1, col(i)), (u, col(i))] for i, u in enumerate(us)]
    if pattern == "tail":
        starts = sorted({(T - 1) // s * s for s in steps})
        return [[(t, col(i)) for t in sorted({s0, T - 1})] for i, s0 in enumerate(starts)]
    if pattern in ("full_rank", "ulp"):
        jobs = []
        for s in steps:
            k = mid(s, T)
            ts = (k + s // 2, k + s - 1, k + s)
            assert k < ts[0] < ts[1] < ts[2] < T, (g, ts)
            jobs.append([(t, rcols) for t in ts])
        return jobs
    if pattern == "run":
        k = min(mid(L, T), (T // L - 2) * L)
        assert k >= L and k + 2 * L <= T, g
        return [[(t, col(0)) for t in range(k, k + 2 * L)],
                [(t, rcols) for t in range(k, k + 2 * L)]]
    if pattern == "cycle":
        return [[(t, [cols[t % len(cols)]]) for t in range(1, T)]]
    if pattern == "agree":
        return [[(t, rcols) for t in range(T)]]
    raise ValueError(pattern)


def check_invariants(mask, r, pupil=False):
    """At most r exact columns in a frame, never a whole folded pupil pair,
    and the clean trajectories untouched."""
    assert mask.dtype == bool and mask.ndim == 3
    assert int(mask.sum(axis=2).max()) <= r, "more than r exact columns in one frame"
    if pupil:
        for a, b in PUPIL_PAIRS:
            assert not (mask[:, :, a] & mask[:, :, b]).any(), "both columns of a folded pair"
    assert not mask[sorted(clean_rows(mask.shape[0]))].any(), "a clean trajectory was changed"


# largest condition number of the rows of C that are exact in one frame
COND_MAX = 10.0


def check_conditioning(mask, models, r):
    """The exact columns of every frame, taken together, must be a
    well-conditioned observation of the state: cond(C[cols]) <= COND_MAX.
    S's exact block is C[cols] P C[cols]^T with no noise floor, so its
    condition number is up to cond(C[cols])^2 cond(P): rows that are nearly
    dependent approach the singular S of more than r exact columns, where the
    float64 oracle itself is off (measured: three columns with cond 88 at
    (3, 8) put the oracle 2e-8 px and 1e-8 of the NLL from long double)."""
    for b in np.nonzero(mask.any(axis=(1, 2)))[0]:
        for cs in {tuple(np.nonzero(f)[0]) for f in mask[b] if f.sum() >= 2}:
            assert len(cs) <= r
            cond = float(np.linalg.cond(np.asarray(models[b]["C"])[list(cs)]))
            assert cond <= COND_MAX, (int(b), cs, cond)


def build(pattern, stacks, grid, r, cols=None, pupil=False, models=None):
    """-> (members with the pattern's entries made exact, (B, T, n) bool mask
    of those entries, the changed trajectories).  ``ulp``: member 1 of every
    such entry is one float32 ulp above the others (ev ~ 1e-11, not 0).
    With ``models`` (the fits of ``stacks``) the patterns that make r columns
    exact at once take, per trajectory, the r best-conditioned rows of its C."""
    st = np.array(stacks, dtype=np.float64)
    B, E, T, n = st.shape
    assert T == grid["T"] and E >= 2
    if cols is None:
        cols = PUPIL_COLS if pupil else tuple(range(n))
    if pattern == "ulp":
        assert np.array_equal(st, st.astype(np.float32)), "ulp: float32 member sources only"
    njobs = len(pattern_jobs(pattern, grid, r, cols))
    mask = np.zeros((B, T, n), dtype=bool)
    changed = []
    for base, width in _bases(B, njobs):
        for i in range(njobs):
            b = base + i % width
            rcols = best_columns(models[b]["C"], r) if models is not None else None
            job = pattern_jobs(pattern, grid, r, cols, rcols)[i]
            changed.append(b)
            for t, cs in job:
                for c in cs:
                    v = np.float32(st[b, 0, t, c])
                    st[b, :, t, c] = np.float64(v)
                    if pattern == "ulp":
                        st[b, 1, t, c] = np.float64(np.nextafter(v, np.float32(np.inf)))
                    mask[b, t, c] = True
    check_invariants(mask, r, pupil)
    return st, mask, sorted(set(changed))


def fit_models(stacks, n, smooth_param=0.05):
    """tests/test_gpu_ragged._fit_models with the smoothing parameter free."""
    from oracle import eks_oracle as O
    models = []
    for st in stacks:
        preds, ev = O.ensemble_array(st)
        p = (O.singleview_params if n == 2 else O.multicam_params)(preds, ev, smooth_param, 25)
        models.append(dict(m0=p["m0"], S0=p["S0"], A=p["A"], Q=p["Q"], C=p["C"],
                           offset=p["means"]))
    return models


def singular_q_model(preds):
    """(2, 2): Q singular, A couples the noise-driven coordinate into the
    other one, so every predicted covariance past the first step is regular
    and so is the reference at every t; only an element that *starts* at an
    exact observation of column 1 sees c Q c = 0 with nothing added to it."""
    return dict(m0=np.zeros(2), S0=np.diag([30.0, 20.0]), A=np.array([[1.0, 0.0], [0.3, 1.0]]),
                Q=np.diag([0.5, 0.0]), C=np.eye(2), offset=preds.mean(axis=0))


# ---------------------------------------------------------------------------
# the oracle's recursions in any float type
# ---------------------------------------------------------------------------
def _eliminate(a, b):
    """Gaussian elimination with partial pivoting in the arrays' own type
    (np.linalg has no long double): -> (x with a x = b, log |det a|)."""
    a = a.copy()
    b = b.copy().reshape(len(a), -1)
    k = len(a)
    logdet = a.dtype.type(0)
    for i in range(k):
        p = i + int(np.argmax(np.abs(a[i:, i])))
        if p != i:
            a[[i, p]] = a[[p, i]]
            b[[i, p]] = b[[p, i]]
        if a[i, i] == 0:
            raise np.linalg.LinAlgError("Singular matrix")
        logdet += np.log(np.abs(a[i, i]))
        f = a[i + 1:, i] / a[i, i]
        a[i + 1:] -= f[:, None] * a[i]
        b[i + 1:] -= f[:, None] * b[i]
    x = np.zeros_like(b)
    for i in range(k - 1, -1, -1):
        x[i] = (b[i] - a[i, i + 1:] @ x[i + 1:]) / a[i, i]
    return x, logdet


def reference(st, m, dtype=np.longdouble):
    """oracle.filtering_pass, smooth_backward and compute_nll of one
    trajectory's members (E, T, n) in ``dtype`` -> (out (T, n), nll, mf, Vf)."""
    from oracle import eks_oracle as O
    preds, ev = O.ensemble_array(st)        # exact in float64 for float32-valued members
    c = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    C, A, Q, ev = c(m["C"]), c(m["A"]), c(m["Q"]), c(ev)
    y = c(preds) - c(m["offset"])
    T, n = y.shape
    r = len(m["m0"])
    mf, Vf, S = np.zeros((T, r), dtype), np.zeros((T, r, r), dtype), np.zeros((T, r, r), dtype)
    pm, pP = c(m["m0"]), c(m["S0"])
    nll = dtype(0)
    for t in range(T):
        if t:
            pm, pP = A @ mf[t - 1], A @ Vf[t - 1] @ A.T + Q
            S[t - 1] = pP
        sig = np.diag(ev[t]) + C @ pP @ C.T
        e = y[t] - C @ pm
        x, logdet = _eliminate(sig, np.concatenate([e[:, None], C @ pP], axis=1))
        mf[t] = pm + pP @ C.T @ x[:, 0]
        Vf[t] = pP - pP @ C.T @ x[:, 1:]
        nll += dtype(0.5) * (n * dtype(LOG_2PI) + logdet + e @ x[:, 0])
    ms = np.zeros_like(mf)
    ms[-1] = mf[-1]
    for t in range(T - 2, -1, -1):
        gain = _eliminate(S[t], A @ Vf[t])[0].T
        ms[t] = mf[t] + gain @ (ms[t + 1] - A @ mf[t])
    return ms @ C.T + c(m["offset"]), nll, mf, Vf


# ---------------------------------------------------------------------------
# numpy model of the device's filtering element (kf_steps.hpp)
# ---------------------------------------------------------------------------
def elem(y, ev, m, s, e):
    """The element of steps [s, e) as k_c1_elem / k3_fwd build it: from the
    identity, every step a predict (elem_predict) and then one scalar
    absorption per column (absorb_scalar).  -> (Ab, bb, Cb, eta, Jb, ok); ok
    is false when a pivot s = c Cb c + ev was not positive (the kernels'
    ``ok = ok && !(s <= 0)``: EKS_STATUS_SCAN)."""
    r = len(m["m0"])
    A, Q, C = m["A"], m["Q"], m["C"]
    Ab, bb, Cb, eta, Jb = np.eye(r), np.zeros(r), np.zeros((r, r)), np.zeros(r), np.zeros((r, r))
    ok = True
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(s, e):
            Ab, bb, Cb = A @ Ab, A @ bb, A @ Cb @ A.T + Q
            for i in range(y.shape[1]):
                c = C[i]
                v, g = Cb @ c, Ab.T @ c
                sc = c @ v + ev[t, i]
                ok = ok and not (sc <= 0)
                e0 = y[t, i] - c @ bb
                eta = eta + g * e0 / sc
                Jb = Jb + np.outer(g, g) / sc
                k = v / sc
                bb, Ab, Cb = bb + k * e0, Ab - np.outer(k, g), Cb - np.outer(k, v)
    return Ab, bb, Cb, eta, Jb, ok


def compose_state(mm, P, el):
    """Filtered state at s - 1 combined with the element of [s, e):
    P' = Ab (I + P Jb)^-1 P Ab^T + Cb, m' = Ab (I + P Jb)^-1 (m + P eta) + bb."""
    Ab, bb, Cb, eta, Jb = el[:5]
    Mi = np.linalg.inv(np.eye(len(mm)) + P @ Jb)
    m2 = Ab @ (Mi @ (mm + P @ eta)) + bb
    P2 = Ab @ Mi @ P @ Ab.T + Cb
    return m2, 0.5 * (P2 + P2.T)
