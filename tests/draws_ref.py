"""References of the posterior trajectory draws (test_draws_host.py,
test_gpu_draws.py), float64 numpy, shared and read only.

``draws``   the sequential backward sampler on gaps_ref.dense's filter:
            delta_{T-1} = chol(P_{T-1}) z_{T-1},
            delta_t = J_t delta_{t+1} + chol(D_t) z_t, x_t = ms_t + delta_t,
            with np.linalg.cholesky.
``joint``   the dense smoothing posterior of the whole trajectory, independent
            of any recursion: the block-tridiagonal precision Lambda of
            (x_0 .. x_{T-1}) given the observed columns, Sigma = Lambda^-1 and
            the mean Sigma eta.
``philox4x32_10`` / ``uniform_bits`` / ``normals``  a model of the seeded
            generator, written from the layout in include/eks_hip.h.

Fed the T r one-hot noise vectors, the responses M of ``draws`` satisfy
M M^T = Sigma: that is what pins the sampler, exactly and without statistics.
"""
import functools

import numpy as np

import gaps_ref as G


def filtered(y, ev, p):
    """gaps_ref.dense's filter: mf (T, r), Vf (T, r, r)."""
    m0, S0, A, Q, C, off = p["m0"], p["S0"], p["A"], p["Q"], p["C"], p["means"]
    T = y.shape[0]
    r = m0.shape[0]
    seen = G.observed(y, ev)
    mf = np.zeros((T, r))
    Vf = np.zeros((T, r, r))
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
            m = m + K @ e
            P = P - K @ Cv @ P
            P = 0.5 * (P + P.T)
        mf[t], Vf[t] = m, P
    return mf, Vf


def draws(y, ev, p, z):
    """z (S, T, r) standard normal (or any) noise -> dict(latent (S, T, r),
    draws (S, T, n), ms (T, r), out (T, n))."""
    A, Q, C, off = p["A"], p["Q"], p["C"], p["means"]
    z = np.asarray(z, dtype=np.float64)
    S, T, r = z.shape
    mf, Vf = filtered(y, ev, p)
    ms = np.zeros((T, r))
    delta = np.zeros((S, T, r))
    ms[T - 1] = mf[T - 1]
    delta[:, T - 1] = z[:, T - 1] @ np.linalg.cholesky(Vf[T - 1]).T
    for t in range(T - 2, -1, -1):
        Sp = A @ Vf[t] @ A.T + Q
        J = np.linalg.solve(Sp, A @ Vf[t]).T
        D = Vf[t] - J @ Sp @ J.T
        Lc = np.linalg.cholesky(0.5 * (D + D.T))
        ms[t] = mf[t] + J @ (ms[t + 1] - A @ mf[t])
        delta[:, t] = delta[:, t + 1] @ J.T + z[:, t] @ Lc.T
    latent = ms[None] + delta
    return dict(latent=latent, draws=latent @ C.T + off, ms=ms, out=ms @ C.T + off)


def joint(y, ev, p):
    """The dense posterior of the stacked state: Sigma (T r, T r), mean (T, r)."""
    m0, S0, A, Q = p["m0"], p["S0"], p["A"], p["Q"]
    T = y.shape[0]
    r = m0.shape[0]
    W, w, _ = G.info_sums(y, ev, p)
    Qi, S0i = np.linalg.inv(Q), np.linalg.inv(S0)
    AQA, AQ = A.T @ Qi @ A, A.T @ Qi
    Lam = np.zeros((T * r, T * r))
    eta = np.zeros(T * r)
    for t in range(T):
        blk = W[t] + (S0i if t == 0 else Qi)
        if t < T - 1:
            blk = blk + AQA
            Lam[t * r:(t + 1) * r, (t + 1) * r:(t + 2) * r] = -AQ
            Lam[(t + 1) * r:(t + 2) * r, t * r:(t + 1) * r] = -AQ.T
        Lam[t * r:(t + 1) * r, t * r:(t + 1) * r] = blk
        eta[t * r:(t + 1) * r] = w[t] + (S0i @ m0 if t == 0 else 0.0)
    Sigma = np.linalg.inv(Lam)
    Sigma = 0.5 * (Sigma + Sigma.T)
    return Sigma, (Sigma @ eta).reshape(T, r)


def one_hot(T, r):
    """The T r one-hot noise vectors as (T r, T, r): draw t r + i has z_t[i] = 1."""
    return np.eye(T * r).reshape(T * r, T, r)


def responses(latent, ms):
    """M (T r, T r) with M[:, s] = the stacked deviation of draw s from the mean."""
    S, T, r = latent.shape
    return (latent - ms[None]).reshape(S, T * r).T


# ---------------------------------------------------------------------------
# the shared cases: T = 24 with 25 % random gaps, a 5-frame void, first and
# last frame missing ("gaps"), and the same members complete
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(kind, T=24, gaps=True):
    """(members (1, E, T, n) with gaps, model, y (T, n), ev (T, n), mask)."""
    st = G.members(kind, 1, T)
    model = G.model_of(kind, st[0])
    n = st.shape[3]
    mask = np.zeros((1, T, n), dtype=bool)
    if gaps:
        mask = np.random.default_rng(1000 * T + n).random((1, T, n)) < 0.25
        mask[0, 9:14] = True
        mask[0, 0] = True
        mask[0, -1] = True
    g = G.knock_out(st, mask)
    y, ev = G.ensemble(g[0])
    for a in (g, y, ev, mask):
        a.setflags(write=False)
    return g, model, y, ev, mask


CASES = (("sv", True), ("mc", True), ("sv", False), ("mc", False))


# ---------------------------------------------------------------------------
# the generator (include/eks_hip.h, eks_draws_gaps)
# ---------------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays holding 32-bit words; key (k0, k1) ints -> four
    uint64 arrays of 32-bit words."""
    x0, x1, x2, x3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * x0
        p1 = np.uint64(M1) * x2
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
        x0, x1, x2, x3 = hi1 ^ x1 ^ np.uint64(k0), lo1, hi0 ^ x3 ^ np.uint64(k1), lo0
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return x0, x1, x2, x3


def uniform_bits(seed, b, s, t, block):
    """The 53-bit integers (k1, k2) of a block; b, s, t broadcastable int arrays."""
    b, s, t = np.broadcast_arrays(np.asarray(b, dtype=np.uint64), np.asarray(s, dtype=np.uint64),
                                  np.asarray(t, dtype=np.uint64))
    ctr = (t & MASK32, (t >> np.uint64(32)) | np.uint64(block << 8), s, b)
    x0, x1, x2, x3 = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return ((x0 << np.uint64(21)) | (x1 >> np.uint64(11)),
            (x2 << np.uint64(21)) | (x3 >> np.uint64(11)))


def raw(seed, B, S, T, r, b0=0, s0=0, t0=0):
    """(B, S, T, r) the integers behind every component: k1 for an even i, k2
    for an odd one (what eks_draws_noise writes under EKS_DBG_DRAWS_RAW)."""
    b, s, t = np.meshgrid(np.arange(b0, b0 + B), np.arange(s0, s0 + S), np.arange(t0, t0 + T),
                          indexing="ij")
    out = np.zeros((B, S, T, r), dtype=np.uint64)
    for blk in range((r + 1) // 2):
        k1, k2 = uniform_bits(seed, b, s, t, blk)
        out[..., 2 * blk] = k1
        if 2 * blk + 1 < r:
            out[..., 2 * blk + 1] = k2
    return out


def normals(seed, B, S, T, r, b0=0, s0=0, t0=0):
    """(B, S, T, r) z(b, s, t, i) for b0 <= b < b0 + B and so on."""
    b, s, t = np.meshgrid(np.arange(b0, b0 + B), np.arange(s0, s0 + S), np.arange(t0, t0 + T),
                          indexing="ij")
    z = np.zeros((B, S, T, r))
    for blk in range((r + 1) // 2):
        k1, k2 = uniform_bits(seed, b, s, t, blk)
        u1 = (k1 + np.uint64(1)).astype(np.float64) * 2.0 ** -53
        u2 = k2.astype(np.float64) * 2.0 ** -53
        rad = np.sqrt(-2.0 * np.log(u1))
        ang = 6.283185307179586 * u2
        z[..., 2 * blk] = rad * np.cos(ang)
        if 2 * blk + 1 < r:
            z[..., 2 * blk + 1] = rad * np.sin(ang)
    return z
