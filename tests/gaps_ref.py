"""References of the missing-observation smoother (test_gaps_host.py,
test_gpu_gaps.py), float64 numpy, shared and read only.

``dense``    the textbook form: per step the observed rows of C are selected,
             the innovation system is solved, the RTS recursions follow and
             the NLL is summed over the observed entries.
``chunked``  a model of the device algorithm (eks_amd/csrc/gap_smooth.hpp):
             information-form sums W_t, w_t, kappa_t, step elements composed
             per chunk, a prefix over the chunk elements, the filter re-run
             from the entering state, and the RTS maps composed right to left.

Column (t, j) is missing iff its ensemble average or variance is not finite.
"""
import functools
import warnings

import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))


def ensemble(stack, mode="median"):
    """(avg, var) of members (E, T, n) as the oracle's ensemble_array, quiet
    about the NaN / inf members that mark gaps."""
    from oracle import eks_oracle as O
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return O.ensemble_array(stack, mode)


def observed(y, ev):
    return np.isfinite(y) & np.isfinite(ev)


def pack(p):
    """One model dict (oracle ``*_params``) as a packed parameter row."""
    return np.concatenate([p["m0"].ravel(), p["S0"].ravel(), p["A"].ravel(), p["Q"].ravel(),
                           p["C"].ravel(), p["means"].ravel()])


def dense(y, ev, p):
    """y, ev (T, n) ensemble averages / variances with non-finite gaps; p a
    model dict (m0, S0, A, Q, C, means).  Returns dict(out (T, n), var (T, n),
    ms (T, r), Vs (T, r, r), nll, nobs, and the model's C and off)."""
    m0, S0, A, Q, C, off = p["m0"], p["S0"], p["A"], p["Q"], p["C"], p["means"]
    T, n = y.shape
    r = m0.shape[0]
    seen = observed(y, ev)
    mf = np.zeros((T, r))
    Vf = np.zeros((T, r, r))
    nll = 0.0
    m, P = m0.copy(), S0.copy()
    for t in range(T):
        if t > 0:
            m = A @ m
            P = A @ P @ A.T + Q
        v = np.nonzero(seen[t])[0]
        if v.size:
            Cv = C[v]
            sig = np.diag(ev[t, v]) + Cv @ P @ Cv.T
            e = (y[t, v] - off[v]) - Cv @ m
            K = np.linalg.solve(sig, Cv @ P).T
            _, logdet = np.linalg.slogdet(sig)
            nll += 0.5 * (v.size * LOG_2PI + logdet + e @ np.linalg.solve(sig, e))
            m = m + K @ e
            P = P - K @ Cv @ P
            P = 0.5 * (P + P.T)
        mf[t], Vf[t] = m, P
    ms = np.zeros((T, r))
    Vs = np.zeros((T, r, r))
    ms[T - 1], Vs[T - 1] = mf[T - 1], Vf[T - 1]
    for t in range(T - 2, -1, -1):
        S = A @ Vf[t] @ A.T + Q
        J = np.linalg.solve(S, A @ Vf[t]).T
        ms[t] = mf[t] + J @ (ms[t + 1] - A @ mf[t])
        Vs[t] = Vf[t] + J @ (Vs[t + 1] - S) @ J.T
    return dict(out=ms @ C.T + off, var=np.einsum("ji,tik,jk->tj", C, Vs, C), ms=ms, Vs=Vs,
                nll=float(nll), nobs=int(seen.sum()), C=C, off=off)


# ---------------------------------------------------------------------------
# the chunked information-form algorithm
# ---------------------------------------------------------------------------
def info_sums(y, ev, p):
    """W (T, r, r), w (T, r), kappa (T,) over the observed columns."""
    C, off = p["C"], p["means"]
    T, n = y.shape
    r = C.shape[1]
    seen = observed(y, ev)
    W = np.zeros((T, r, r))
    w = np.zeros((T, r))
    kap = np.zeros(T)
    for t in range(T):
        for j in np.nonzero(seen[t])[0]:
            z = y[t, j] - off[j]
            W[t] += np.outer(C[j], C[j]) / ev[t, j]
            w[t] += C[j] * z / ev[t, j]
            kap[t] += LOG_2PI + np.log(ev[t, j]) + z * z / ev[t, j]
    return W, w, kap


def step_elem(A, Q, W, w):
    """(Ab, bb, Cb, eta, Jb) of one step t > 0, N = (I + Q W)^-1."""
    N = np.linalg.inv(np.eye(len(w)) + Q @ W)
    Ab = N @ A
    Cb = N @ Q
    return Ab, Cb @ w, Cb, Ab.T @ w, Ab.T @ W @ A


def absorb(E, predict, A, Q, W, w):
    """One step absorbed into the element on the right (the form G1 runs, one
    inverse per step): the element is predicted through (A, Q) when
    ``predict``, then updated with (W, w), N = (I + C' W)^-1.  Equal to
    compose_elem(E, step_elem(A, Q, W, w))."""
    Ab, bb, Cb, eta, Jb = E
    if predict:
        Ab, bb, Cb = A @ Ab, A @ bb, A @ Cb @ A.T + Q
    N = np.linalg.inv(np.eye(len(w)) + Cb @ W)
    NA = N @ Ab
    return (NA, N @ (bb + Cb @ w), N @ Cb, eta + NA.T @ (w - W @ bb), Jb + NA.T @ W @ Ab)


def compose_elem(Ei, Ej):
    """Ei (earlier) then Ej (Sarkka & Garcia-Fernandez 2021, Lemma 8)."""
    Ai, bi, Ci, ei, Ji = Ei
    Aj, bj, Cj, ej, Jj = Ej
    M = np.linalg.inv(np.eye(len(bi)) + Ci @ Jj)
    return (Aj @ M @ Ai, Aj @ M @ (bi + Ci @ ej) + bj, Aj @ M @ Ci @ Aj.T + Cj,
            Ai.T @ M.T @ (ej - Jj @ bi) + ei, Ai.T @ M.T @ Jj @ Ai + Ji)


def compose_state(m, P, E):
    Ab, bb, Cb, eta, Jb = E
    M = np.linalg.inv(np.eye(len(m)) + P @ Jb)
    return Ab @ M @ (m + P @ eta) + bb, Ab @ M @ P @ Ab.T + Cb


def filter_step(t, A, Q, W, w, kap, m, P):
    """One information-form step: the filtered (m, P) and the step's NLL share."""
    if t > 0:
        m = A @ m
        P = A @ P @ A.T + Q
    M = np.eye(len(m)) + P @ W
    Pn = np.linalg.solve(M, P)
    Pn = 0.5 * (Pn + Pn.T)
    u = w - W @ m
    _, logdet = np.linalg.slogdet(M)
    share = 0.5 * (kap + logdet - 2.0 * w @ m + m @ W @ m - u @ Pn @ u)
    return m + Pn @ u, Pn, share


def chunked(y, ev, p, L):
    """The device algorithm with chunks of L steps (L >= T: the sequential form)."""
    m0, S0, A, Q, C, off = p["m0"], p["S0"], p["A"], p["Q"], p["C"], p["means"]
    T, n = y.shape
    r = m0.shape[0]
    W, w, kap = info_sums(y, ev, p)
    NC = (T + L - 1) // L
    bounds = [(c * L, min(T, (c + 1) * L)) for c in range(NC)]
    # G1: the chunk elements (chunk 0: the filter from the prior as the
    # constant element (0, m, P, 0, 0); the others start from the identity)
    elems = []
    for c, (s, e) in enumerate(bounds):
        if c == 0:
            E = (np.zeros((r, r)), m0.copy(), S0.copy(), np.zeros(r), np.zeros((r, r)))
        else:
            E = (np.eye(r), np.zeros(r), np.zeros((r, r)), np.zeros(r), np.zeros((r, r)))
        for t in range(s, e):
            E = absorb(E, t > 0, A, Q, W[t], w[t])
        elems.append(E)
    # G2: the state entering every chunk
    enter = [(m0, S0)]
    X = elems[0]
    for c in range(1, NC):
        enter.append((X[1], X[2]))
        X = compose_elem(X, elems[c])
    # G3: the filter from the entering state, NLL shares, the RTS maps
    mf = np.zeros((T, r))
    Vf = np.zeros((T, r, r))
    shares, maps = [], []
    for c, (s, e) in enumerate(bounds):
        m, P = enter[c]
        G, g, Lm, share = np.eye(r), np.zeros(r), np.zeros((r, r)), 0.0
        for t in range(s, e):
            m, P, sh = filter_step(t, A, Q, W[t], w[t], kap[t], m, P)
            share += sh
            mf[t], Vf[t] = m, P
            if t + 1 < T:
                S = A @ P @ A.T + Q
                J = np.linalg.solve(S, A @ P).T
                d = m - J @ A @ m
                D = P - J @ S @ J.T
                g, Lm, G = g + G @ d, Lm + G @ D @ G.T, G @ J
            else:
                g, Lm, G = g + G @ m, Lm + G @ P @ G.T, np.zeros((r, r))
        shares.append(share)
        maps.append((G, g, Lm))
    # G4: (ms, Vs) entering every chunk from the right
    back = [None] * NC
    X = maps[NC - 1]
    for c in range(NC - 2, -1, -1):
        back[c] = (X[1], X[2])
        G, g, Lm = maps[c]
        X = (G @ X[0], g + G @ X[1], Lm + G @ X[2] @ G.T)
    # G5: right to left over every chunk
    ms = np.zeros((T, r))
    Vs = np.zeros((T, r, r))
    for c, (s, e) in enumerate(bounds):
        if e < T:
            m_, V_ = back[c]
        for t in range(e - 1, s - 1, -1):
            if t + 1 < T:
                S = A @ Vf[t] @ A.T + Q
                J = np.linalg.solve(S, A @ Vf[t]).T
                m_ = J @ m_ + (mf[t] - J @ A @ mf[t])
                V_ = J @ V_ @ J.T + (Vf[t] - J @ S @ J.T)
            else:
                m_, V_ = mf[t], Vf[t]
            ms[t], Vs[t] = m_, V_
    return dict(out=ms @ C.T + off, var=np.einsum("ji,tik,jk->tj", C, Vs, C), ms=ms, Vs=Vs,
                nll=float(sum(shares)), nobs=int(observed(y, ev).sum()))


# ---------------------------------------------------------------------------
# shared inputs: members with gaps, the models of the complete data
# ---------------------------------------------------------------------------
def members(kind, B, T, V=4, E=5, seed=None):
    """(B, E, T, n) float32-exact float64 members without gaps."""
    from eks_amd import synthetic
    rng = np.random.default_rng(7 * B + T if seed is None else seed)
    if kind == "sv":
        st = synthetic.singleview_obs(rng, E, T, K=B).transpose(2, 0, 1, 3)
    else:
        st = synthetic.multiview_obs(rng, V, E, T, K=B).transpose(2, 0, 1, 3)
    return st.astype(np.float32).astype(np.float64)


def model_of(kind, stack):
    """The oracle's model of complete members (E, T, n), smooth_param = 1."""
    from oracle import eks_oracle as O
    preds, ev = O.ensemble_array(stack)
    if kind == "sv":
        p = O.singleview_params(preds, ev, 1.0, 50.0)
    else:
        p = O.multicam_params(preds, ev, 1.0, 25.0)
    return {k: p[k] for k in ("m0", "S0", "A", "Q", "C", "means")}


def knock_out(st, mask):
    """A copy of members (B, E, T, n) with member 0 of every masked (b, t, j)
    set to NaN: the column's average and variance become NaN."""
    out = st.copy()
    out[:, 0][mask] = np.nan
    return out


def reference(st_gaps, models, mode="median"):
    """[dense(...)] per trajectory of members (B, E, T, n)."""
    res = []
    for b in range(st_gaps.shape[0]):
        y, ev = ensemble(st_gaps[b], mode)
        res.append(dense(y, ev, models[b]))
    return res


@functools.lru_cache(maxsize=None)
def case_sv131():
    """Case 1: (2,2), B = 3, T = 131: 20 % random gaps, a 40-frame run with
    nothing observed across chunk boundaries of 8, first and last frame
    missing; trajectory 2 without any gap."""
    st = members("sv", 3, 131)
    models = [model_of("sv", st[b]) for b in range(3)]
    rng = np.random.default_rng(131)
    mask = rng.random((3, 131, 2)) < 0.2
    mask[0, 45:85] = True
    mask[1, 3:43] = True
    mask[:2, 0] = True
    mask[:2, -1] = True
    mask[2] = False
    g = knock_out(st, mask)
    ref = reference(g, models)
    g.setflags(write=False)
    return g, models, ref, mask
