// Smoothing through missing observations (eks_smooth_gaps): the
// posterior-variance pipeline of post_var.hpp extended by the means.
//
// Column (t, j) of a trajectory is MISSING iff its ensemble average or its
// ensemble variance is not finite (a NaN member, a +-inf member; a non-finite
// y or ev of a y / ev hand-off); every other column is OBSERVED.  With V_t
// the observed columns of step t and z_j = y_j - offset_j the data enter
// through
//   W_t = sum_{j in V_t} c_j c_j^T / ev_j      w_t = sum_{j in V_t} c_j z_j / ev_j
//   kappa_t = sum_{j in V_t} (log 2 pi + log ev_j + z_j^2 / ev_j)
// so a missing column is a term left out of three sums, and a step with
// nothing observed is W_t = 0, a pure prediction.  W_t may be rank-deficient
// or zero; no branch, pivot or per-n code follows from it.
//
//   filter   m-_0 = m0, P-_0 = S0;  t > 0: m- = A m, P- = A P A^T + Q
//            P = (I + P- W_t)^-1 P-,  u = w_t - W_t m-,  m = m- + P u
//   NLL      nll += 1/2 [kappa_t + log det(I + P- W_t) - 2 w_t^T m- + m-^T W_t m- - u^T P u]
//   RTS      S_t = A P_t A^T + Q, J_t = P_t A^T S_t^-1, d_t = m_t - J_t A m_t,
//            D_t = P_t - J_t S_t J_t^T;  ms_t = J_t ms_{t+1} + d_t,
//            Vs_t = J_t Vs_{t+1} J_t^T + D_t,  ms_{T-1} = m_{T-1}, Vs_{T-1} = P_{T-1}
//   output   out[t][j] = c_j ms_t + offset_j,  pvar[t][j] = c_j Vs_t c_j^T  for every j
//
// One step t > 0 as a filtering element (kf_steps.hpp's Elem<R>, the
// convention of compose_state), N = (I + Q W_t)^-1:
//   Ab = N A,  Cb = N Q,  bb = Cb w_t,  eta = Ab^T w_t,  Jb = Ab^T W_t A
//
// Each trajectory's T steps are cut into NC chunks of L steps; one lane owns
// one (chunk, trajectory) pair (Lane<UNI>).  Five launches, launch boundaries
// the only synchronisation:
//
//  G1 k_gp_elem   members (or the y / ev planes) -> W_t, w_t, kappa_t planes
//                 and the chunk's count of observed entries; the chunk's
//                 Elem<R>, every step absorbed on the right (gp_absorb: the
//                 composition with the step's element, one inverse; chunk 0:
//                 the plain filter from (m0, S0), a constant element)
//  G2 k_gp_fscan  prefix over the elements: (m, P) entering every chunk
//  G3 k_gp_rerun  the filter above from that state over the planes: m_t, P_t
//                 planes, the chunk's NLL share, its Affine map and CovMap
//  G4 k_gp_bscan  suffix over the maps: (ms, Vs) entering every chunk from the
//                 right; nll[b] and nobs[b] summed in ascending chunk order
//  G5 k_gp_final  right to left over the chunk from the m_t, P_t planes: out,
//                 and pvar, ms, Vs if asked
//
// The scans are post_var.hpp's: one lane per trajectory while
// NC <= wave_scan_chunks(), above that one wave per trajectory (each lane
// folds a contiguous run of ceil(NC / 64) chunks, a 64-lane shuffle scan, each
// lane rewrites its run).  The association order depends on (NC, form) alone,
// so two calls give the same bits.
//
// An observed column with ev == 0 makes W_t infinite: EKS_STATUS_SCAN, and
// W_t, w_t, kappa_t are NaN from that step on, with them every value of the
// trajectory.  A singular S_t or I + P J sets EKS_STATUS_SINGULAR; NaN
// operands compare unequal to 0 and set nothing.
#pragma once
#include "post_var.hpp"

namespace eks {

extern long long g_gaps_chunk;  // forced chunk length (EKS_DBG_GAPS_CHUNK), 0: automatic

struct GpArgs {
  const void *obs;
  int dtype;
  long long B, T;
  int E, n;
  long long sb, st, se, sj;
  int median;
  const double *params;
  double *out;
  long long ob, ot, oj;
  double *pvar, *ms, *Vs, *nll;
  int32_t *nobs;
  char *ws;
  int32_t *status;
  hipStream_t stream;
};

// workspace arrays (time-major: B values per plane; doubles but cnt, int32)
struct GpPlan {
  long long L = 0, NC = 0;
  size_t w_off = 0;     // W_t       T  x Sym<R>::len
  size_t sw_off = 0;    // w_t       T  x R
  size_t kap_off = 0;   // kappa_t   T
  size_t m_off = 0;     // m_t       T  x R
  size_t p_off = 0;     // P_t       T  x Sym<R>::len
  size_t elem_off = 0;  // elements  NC x Elem<R>::len
  size_t sin_off = 0;   // (m, P) entering a chunk              NC x (R + Sym<R>::len)
  size_t map_off = 0;   // (Affine, CovMap)   NC x (Affine<R>::len + CovMap<R>::len)
  size_t bin_off = 0;   // (ms, Vs) entering a chunk from the right   NC x (R + Sym<R>::len)
  size_t nll_off = 0;   // NLL shares         NC
  size_t cnt_off = 0;   // observed entries   NC (int32)
  size_t total = 0;
  const char *evsrc = nullptr;  // the caller's ev planes (y / ev input)
};

inline int gp_map_len(int r) { return 2 * r * r + r + pv_sym_len(r); }  // GapMap<R>::len

// Chunk length as launched: pv_chunk_len's rule (a multiple of 8; one chunk
// when it covers T) with its own debug key.
inline long long gp_chunk_len(long long B, long long T, int r) {
  return chunk_len_rule(g_gaps_chunk, call_chunk_len(B, T, r, true, 0), 0.15, 0.11, B, T, r);
}

inline GpPlan gp_make_plan(long long B, long long T, int r, long long L) {
  GpPlan p;
  p.L = L;
  p.NC = (T + L - 1) / L;
  const size_t S = (size_t)pv_sym_len(r), R = (size_t)r, Bz = (size_t)B, NC = (size_t)p.NC;
  Carver ws;
  auto take = [&](size_t planes, size_t bytes) { return ws.take(planes * Bz * bytes); };
  p.w_off = take((size_t)T * S, 8);
  p.sw_off = take((size_t)T * R, 8);
  p.kap_off = take((size_t)T, 8);
  p.m_off = take((size_t)T * R, 8);
  p.p_off = take((size_t)T * S, 8);
  p.elem_off = take(NC * (size_t)elem_len(r), 8);
  p.sin_off = take(NC * (R + S), 8);
  p.map_off = take(NC * (size_t)gp_map_len(r), 8);
  p.bin_off = take(NC * (R + S), 8);
  p.nll_off = take(NC, 8);
  p.cnt_off = take(NC, 4);
  p.total = ws.off;
  return p;
}

// ---------------------------------------------------------------------------
// plane access of the small pieces
// ---------------------------------------------------------------------------
template <int R>
EKS_DEV void gp_load_vec(const double *base, long long plane0, long long B, unsigned b,
                         double (&v)[R]) {
#pragma unroll
  for (int i = 0; i < R; ++i) v[i] = pl(base, plane0 + i, B, b);
}

template <int R>
EKS_DEV void gp_store_vec(double *base, long long plane0, long long B, unsigned b,
                          const double (&v)[R]) {
#pragma unroll
  for (int i = 0; i < R; ++i) pl(base, plane0 + i, B, b) = v[i];
}

template <int R>
EKS_DEV void gp_load_elem(const double *eb, long long c, long long B, unsigned b, Elem<R> &e) {
  e.load(&pl(eb, c * Elem<R>::len, B, b), B);
}

template <int R>
EKS_DEV Elem<R> gp_shfl_up(const Elem<R> &e, int delta) {
  Elem<R> o;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    o.bb[i] = __shfl_up(e.bb[i], delta, 64);
    o.eta[i] = __shfl_up(e.eta[i], delta, 64);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      o.Ab[i][j] = __shfl_up(e.Ab[i][j], delta, 64);
      o.Cb[i][j] = __shfl_up(e.Cb[i][j], delta, 64);
      o.Jb[i][j] = __shfl_up(e.Jb[i][j], delta, 64);
    }
  }
  return o;
}

// ---------------------------------------------------------------------------
// one filter step in information form; (m, P) the state of step t-1 (or the
// prior when t == 0), replaced by the filtered state of step t.  NLL: the
// step's share 1/2 [kappa + log det(I + P- W) - 2 w^T m- + m-^T W m- - u^T P u]
// is added to *nll.
// ---------------------------------------------------------------------------
template <int R>
EKS_DEV bool gp_filter_step(bool predict, const double (&A)[R][R], const double (&Q)[R][R],
                            const double (&W)[R][R], const double (&w)[R], double kappa,
                            double (&m)[R], double (&P)[R][R], double *nll) {
  if (predict) {
    double Am[R];
    matvec<R, R>(A, m, Am);
#pragma unroll
    for (int i = 0; i < R; ++i) m[i] = Am[i];
    pv_predict<R>(P, A, Q);
  }
  double M[R][R], N[R][R], u[R], Wm[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) s = fma(W[i][k], m[k], s);
    Wm[i] = s;
    u[i] = w[i] - s;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      double t = (i == j) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) t = fma(P[i][k], W[k][j], t);
      M[i][j] = t;
    }
  }
  const bool ok = small_inverse<R>(M, N);
  double Pn[R][R];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) s = fma(N[i][k], P[k][j], s);
      Pn[i][j] = s;
    }
  double lin = 0.0, quad = 0.0;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    lin = fma(w[i], m[i], lin);
    quad = fma(m[i], Wm[i], quad);
  }
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) P[i][j] = P[j][i] = Pn[i][j];
  double Pu[R], upu = 0.0;
  matvec<R, R>(P, u, Pu);
#pragma unroll
  for (int i = 0; i < R; ++i) {
    upu = fma(u[i], Pu[i], upu);
    m[i] += Pu[i];
  }
  if (nll) *nll += 0.5 * (kappa + log(small_det<R>(M)) - 2.0 * lin + quad - upu);
  return ok;
}

// One step absorbed into the element on the right: predicted through (A, Q)
// when `predict`, then updated with (W, w).  Equal to compose_elem with the
// step's element (the formulas at the top), with one inverse instead of two,
// N = (I + C' W)^-1:
//   A' = A Ab, b' = A bb, C' = A Cb A^T + Q
//   Ab = N A',  bb = N (b' + C' w),  Cb = N C',
//   eta += (N A')^T (w - W b'),  Jb += (N A')^T W A'
// (CovElem::absorb with the means).  From the identity the first step gives
// the step's element; from (0, m0, S0, 0, 0) the run is the plain filter and
// ends in the constant element (0, m, P, 0, 0).
template <int R>
EKS_DEV bool gp_absorb(Elem<R> &E, bool predict, const double (&A)[R][R],
                       const double (&Q)[R][R], const double (&W)[R][R], const double (&w)[R]) {
  double Ap[R][R], bp[R], Cp[R][R];
  if (predict) {
    matmul<R, R, R>(A, E.Ab, Ap);
    matvec<R, R>(A, E.bb, bp);
    pv_congruence<R>(A, E.Cb, Q, Cp);
  } else {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      bp[i] = E.bb[i];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        Ap[i][j] = E.Ab[i][j];
        Cp[i][j] = E.Cb[i][j];
      }
    }
  }
  double N[R][R], NA[R][R], WAp[R][R], h[R], v[R];
  const bool ok = pv_inv_ipxy<R>(Cp, W, N);
  matmul<R, R, R>(N, Ap, NA);
  matmul<R, R, R>(W, Ap, WAp);
#pragma unroll
  for (int i = 0; i < R; ++i) {
    double s = w[i], t = bp[i];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      s = fma(-W[i][k], bp[k], s);
      t = fma(Cp[i][k], w[k], t);
    }
    h[i] = s;
    v[i] = t;
  }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    double s = E.eta[i], t = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      s = fma(NA[k][i], h[k], s);
      t = fma(N[i][k], v[k], t);
    }
    E.eta[i] = s;
    E.bb[i] = t;
  }
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) {
      double s = E.Jb[i][j], t = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        s = fma(NA[k][i], WAp[k][j], s);
        t = fma(N[i][k], Cp[k][j], t);
      }
      E.Jb[i][j] = E.Jb[j][i] = s;
      E.Cb[i][j] = E.Cb[j][i] = t;
    }
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) E.Ab[i][j] = NA[i][j];
  return ok;
}

// RTS gain of step t from the filtered (m, P): pv_rts's J and D, rts_gain's d
template <int R>
EKS_DEV bool gp_rts(const double (&m)[R], const double (&P)[R][R], const double (&A)[R][R],
                    const double (&Q)[R][R], double (&J)[R][R], double (&d)[R],
                    double (&D)[R][R]) {
  const bool ok = pv_rts<R>(P, A, Q, J, D);
  double Am[R];
  matvec<R, R>(A, m, Am);
#pragma unroll
  for (int i = 0; i < R; ++i) {
    double s = m[i];
#pragma unroll
    for (int k = 0; k < R; ++k) s = fma(-J[i][k], Am[k], s);
    d[i] = s;
  }
  return ok;
}

// The chunk map of the backward pass, means and covariances:
//   ms_first = G ms_in + g,  Vs_first = G Vs_in G^T + L
// (Affine and CovMap; both carry G, with the same bits)
template <int R>
struct GapMap {
  static constexpr int len = Affine<R>::len + CovMap<R>::len;
  Affine<R> a;
  CovMap<R> v;
  EKS_DEV void set_identity() {
    a.set_identity();
    v.set_identity();
  }
  EKS_DEV void load_pl(const double *mb, long long c, long long B, unsigned b) {
    a.load_at([&](int k) { return pl(mb, c * len + k, B, b); });
    v.load_at([&](int k) { return pl(mb, c * len + Affine<R>::len + k, B, b); });
  }
  EKS_DEV void store_pl(double *mb, long long c, long long B, unsigned b) const {
    a.store_at([&](int k, double x) { pl(mb, c * len + k, B, b) = x; });
    v.store_at([&](int k, double x) { pl(mb, c * len + Affine<R>::len + k, B, b) = x; });
  }
  // this (earlier steps) followed by o (later steps)
  EKS_DEV GapMap then(const GapMap &o) const {
    GapMap m;
    m.a = a.after(o.a);
    m.v = v.then(o.v);
    return m;
  }
  EKS_DEV GapMap shfl_down(int delta) const {
    GapMap o;
    o.a = a.shfl_down(delta);
    o.v = v.shfl_down(delta);
    return o;
  }
};

// The information-form sums of step t over its observed columns: W_t (both
// triangles), w_t, kappa_t; `count` gains the observed entries, `exact` is set
// by an observed ev == 0 and, once set, makes the sums NaN.
template <int R, typename T, int E>
EKS_DEV void gp_step_sums(const typename yev_y<T>::type *ob, const double *evp, long long t,
                          long long B, unsigned b, int n, long long st, long long se,
                          long long sj, int Ert, bool median, const double *Cm,
                          const double *off, double (&W)[R][R], double (&w)[R], double &kappa,
                          int &count, bool &exact) {
  constexpr bool kYev = is_yev<T>::value;
  using MT = typename yev_y<T>::type;
  kappa = 0.0;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    w[i] = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) W[i][k] = 0.0;
  }
  for (int j = 0; j < n; ++j) {
    double avg, var;
    if constexpr (kYev) {
      avg = (double)pl(ob, t * n + j, B, b);
      var = pl(evp, t * n + j, B, b);
    } else {
      column_reduce<E, MT>(ob + t * st + j * sj, se, Ert, median, avg, var);
    }
    const bool seen = fabs(avg) < __builtin_inf() && fabs(var) < __builtin_inf();
    if (!seen) continue;
    ++count;
    exact = exact || (var == 0.0);
    const double z = avg - off[j];
    const double inv = 1.0 / var;
    kappa += kLog2Pi + log(var) + z * z * inv;
    double cr[R];
#pragma unroll
    for (int i = 0; i < R; ++i) cr[i] = Cm[j * R + i];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const double ci = cr[i] * inv;
      w[i] = fma(ci, z, w[i]);
#pragma unroll
      for (int k = i; k < R; ++k) W[i][k] = fma(ci, cr[k], W[i][k]);
    }
  }
  if (exact) {  // an infinite W_t: the trajectory is NaN from here on, both ways
    kappa = __builtin_nan("");
#pragma unroll
    for (int i = 0; i < R; ++i) {
      w[i] = __builtin_nan("");
#pragma unroll
      for (int k = i; k < R; ++k) W[i][k] = __builtin_nan("");
    }
  }
  pv_mirror<R>(W);
}

// ===========================================================================
// G1: W_t, w_t, kappa_t planes, the observed count and the chunk's element
// T: float / double members, or YevIn<float / double> (the y / ev planes; E unused)
// ===========================================================================
template <int R, typename T, int E, bool UNI>
__global__ __launch_bounds__(kBlock) void k_gp_elem(GpArgs a, GpPlan p) {
  Lane<UNI> ln;
  if (!ln.init(a.B, p.NC)) return;
  const long long c = ln.c;
  const unsigned b = ln.b;
  const long long B = a.B, TT = a.T;
  const int n = a.n;
  constexpr int S = Sym<R>::len;
  constexpr bool kYev = is_yev<T>::value;
  using MT = typename yev_y<T>::type;
  using L = ParamLayout<R, 0>;
  const bool median = a.median != 0;
  const double *pp = a.params + (long long)b * param_stride<R, 0>(n);
  double A[R][R], Q[R][R];
  load_mat<R, R>(pp + L::A, A);
  load_mat<R, R>(pp + L::Q, Q);
  const double *Cm = pp + L::C, *off = Cm + (long long)n * R;
  const MT *ob = kYev ? (const MT *)a.obs : (const MT *)a.obs + (long long)b * a.sb;
  const double *evp = (const double *)p.evsrc;
  double *wbuf = (double *)(a.ws + p.w_off);
  double *swbuf = (double *)(a.ws + p.sw_off);
  double *kbuf = (double *)(a.ws + p.kap_off);
  const long long s = c * p.L, e = min(TT, s + p.L);
  const bool first = c == 0;
  bool ok = true, exact = false;
  int count = 0;
  Elem<R> El;
  El.set_identity();
  if (first) {  // the prior as a constant element: the run below is the plain filter
#pragma unroll
    for (int i = 0; i < R; ++i) {
      El.bb[i] = pp[L::m0 + i];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        El.Ab[i][j] = 0.0;
        El.Cb[i][j] = pp[L::S0 + i * R + j];
      }
    }
  }
  for (long long t = s; t < e; ++t) {
    double W[R][R], w[R], kappa;
    gp_step_sums<R, T, E>(ob, evp, t, B, b, n, a.st, a.se, a.sj, a.E, median, Cm, off, W, w, kappa,
                          count, exact);
    pv_store_sym<R>(wbuf, t * S, B, b, W);
    gp_store_vec<R>(swbuf, t * R, B, b, w);
    pl(kbuf, t, B, b) = kappa;
    ok = gp_absorb<R>(El, t > 0, A, Q, W, w) && ok;
  }
  El.store(&pl((double *)(a.ws + p.elem_off), c * Elem<R>::len, B, b), B);
  pl((int32_t *)(a.ws + p.cnt_off), c, B, b) = count;
  flag(a.status, b, (exact ? EKS_STATUS_SCAN : 0) | (ok ? 0 : EKS_STATUS_SINGULAR));
}

// ===========================================================================
// G2: prefix scan of the elements.  One lane per trajectory ...
// ===========================================================================
template <int R>
EKS_DEV void gp_store_state(double *sin, long long c, long long B, unsigned b, const Elem<R> &X) {
  constexpr int SL = R + Sym<R>::len;
  gp_store_vec<R>(sin, c * SL, B, b, X.bb);
  pv_store_sym<R>(sin, c * SL + R, B, b, X.Cb);
}

// (eb, sin: the element and entering-state planes of B values, trajectories
// here and rows in gap_sweep.hpp; false: a singular composition)
template <int R>
EKS_DEV bool gp_fscan_lane(const double *eb, double *sin, long long B, long long NC, unsigned b) {
  bool ok = true;
  Elem<R> X;
  gp_load_elem<R>(eb, 0, B, b, X);
  for (long long c = 1; c < NC; ++c) {
    gp_store_state<R>(sin, c, B, b, X);
    if (c + 1 == NC) break;
    Elem<R> e, t;
    gp_load_elem<R>(eb, c, B, b, e);
    ok = compose_elem<R>(X, e, t) && ok;
    X = t;
  }
  return ok;
}

template <int R>
__global__ __launch_bounds__(64) void k_gp_fscan(GpArgs a, GpPlan p) {
  const long long bl = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (bl >= a.B) return;
  const unsigned b = (unsigned)bl;
  const bool ok = gp_fscan_lane<R>((const double *)(a.ws + p.elem_off),
                                   (double *)(a.ws + p.sin_off), a.B, p.NC, b);
  if (!ok) flag(a.status, b, EKS_STATUS_SINGULAR);
}

// ... or one wave per trajectory: lane l folds chunks [l q, (l+1) q), a
// 64-lane shuffle scan gives the prefix before its run, and it rewrites the run
template <int R>
EKS_DEV bool gp_fscan_wave(const double *eb, double *sin, long long B, long long NC, unsigned b,
                           int lane) {
  const long long q = (NC + 63) / 64;
  const long long c0 = min(NC, lane * q), c1 = min(NC, c0 + q);
  bool ok = true;
  Elem<R> F;
  F.set_identity();
  for (long long c = c0; c < c1; ++c) {
    Elem<R> e, t;
    gp_load_elem<R>(eb, c, B, b, e);
    ok = compose_elem<R>(F, e, t) && ok;
    F = t;
  }
#pragma unroll 1
  for (int k = 1; k < 64; k <<= 1) {
    const Elem<R> o = gp_shfl_up<R>(F, k);
    Elem<R> t;
    const bool ok2 = compose_elem<R>(o, F, t);
    if (lane >= k) {
      F = t;
      ok = ok && ok2;
    }
  }
  Elem<R> X = gp_shfl_up<R>(F, 1);
  if (lane == 0) X.set_identity();
  for (long long c = c0; c < c1; ++c) {
    if (c > 0) gp_store_state<R>(sin, c, B, b, X);
    Elem<R> e, t;
    gp_load_elem<R>(eb, c, B, b, e);
    ok = compose_elem<R>(X, e, t) && ok;
    X = t;
  }
  return ok;
}

template <int R>
__global__ __launch_bounds__(64) void k_gp_fscan_w(GpArgs a, GpPlan p) {
  const unsigned b = blockIdx.x;
  const bool ok = gp_fscan_wave<R>((const double *)(a.ws + p.elem_off),
                                   (double *)(a.ws + p.sin_off), a.B, p.NC, b, threadIdx.x);
  if (!ok) flag(a.status, b, EKS_STATUS_SINGULAR);
}

// ===========================================================================
// G3: the filter over the chunk from its entering state: m_t, P_t planes, the
// chunk's NLL share and its RTS maps
// ===========================================================================
template <int R, bool UNI>
__global__ __launch_bounds__(kBlock) void k_gp_rerun(GpArgs a, GpPlan p) {
  Lane<UNI> ln;
  if (!ln.init(a.B, p.NC)) return;
  const long long c = ln.c;
  const unsigned b = ln.b;
  const long long B = a.B, TT = a.T;
  constexpr int S = Sym<R>::len, SL = R + S;
  using L = ParamLayout<R, 0>;
  const double *pp = a.params + (long long)b * param_stride<R, 0>(a.n);
  double A[R][R], Q[R][R], m[R], P[R][R];
  load_mat<R, R>(pp + L::A, A);
  load_mat<R, R>(pp + L::Q, Q);
  if (c == 0) {
    load_vec<R>(pp + L::m0, m);
    load_mat<R, R>(pp + L::S0, P);
  } else {
    const double *sin = (const double *)(a.ws + p.sin_off);
    gp_load_vec<R>(sin, c * SL, B, b, m);
    pv_load_sym<R>(sin, c * SL + R, B, b, P);
  }
  const double *wbuf = (const double *)(a.ws + p.w_off);
  const double *swbuf = (const double *)(a.ws + p.sw_off);
  const double *kbuf = (const double *)(a.ws + p.kap_off);
  double *mbuf = (double *)(a.ws + p.m_off);
  double *pbuf = (double *)(a.ws + p.p_off);
  GapMap<R> F;
  F.set_identity();
  const long long s = c * p.L, e = min(TT, s + p.L);
  bool ok = true;
  double nll = 0.0;
  for (long long t = s; t < e; ++t) {
    double W[R][R], w[R];
    pv_load_sym<R>(wbuf, t * S, B, b, W);
    gp_load_vec<R>(swbuf, t * R, B, b, w);
    const double kappa = pl(kbuf, t, B, b);
    ok = gp_filter_step<R>(t > 0, A, Q, W, w, kappa, m, P, &nll) && ok;
    gp_store_vec<R>(mbuf, t * R, B, b, m);
    pv_store_sym<R>(pbuf, t * S, B, b, P);
    if (t + 1 < TT) {
      double J[R][R], d[R], D[R][R];
      ok = gp_rts<R>(m, P, A, Q, J, d, D) && ok;
      F.v.step(J, D);
      F.a.then(J, d);
    } else {
      F.v.step_const(P);
      F.a.then_const(m);
    }
  }
  F.store_pl((double *)(a.ws + p.map_off), c, B, b);
  pl((double *)(a.ws + p.nll_off), c, B, b) = nll;
  if (!ok) flag(a.status, b, EKS_STATUS_SINGULAR);
}

// ===========================================================================
// G4: suffix scan of the maps.  The suffix from chunk c+1 on ends in the
// trajectory's last step, a constant map (G = 0), so its (g, L) is the
// (ms, Vs) entering chunk c from the right.  nll[b], nobs[b].
// ===========================================================================
template <int R>
EKS_DEV void gp_store_back(double *bin, long long c, long long B, unsigned b, const GapMap<R> &X) {
  constexpr int SL = R + Sym<R>::len;
  gp_store_vec<R>(bin, c * SL, B, b, X.a.g);
  pv_store_sym<R>(bin, c * SL + R, B, b, X.v.L);
}

template <int R>
__global__ __launch_bounds__(64) void k_gp_bscan(GpArgs a, GpPlan p) {
  const long long bl = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (bl >= a.B) return;
  const unsigned b = (unsigned)bl;
  const long long B = a.B;
  const double *mb = (const double *)(a.ws + p.map_off);
  double *bin = (double *)(a.ws + p.bin_off);
  const double *nb = (const double *)(a.ws + p.nll_off);
  const int32_t *cb = (const int32_t *)(a.ws + p.cnt_off);
  double nll = 0.0;
  int cnt = 0;
  for (long long c = 0; c < p.NC; ++c) {
    nll += pl(nb, c, B, b);
    cnt += pl(cb, c, B, b);
  }
  if (a.nll) a.nll[b] = nll;
  if (a.nobs) a.nobs[b] = cnt;
  GapMap<R> X;
  X.load_pl(mb, p.NC - 1, B, b);
  for (long long c = p.NC - 2; c >= 0; --c) {
    gp_store_back<R>(bin, c, B, b, X);
    if (c == 0) break;
    GapMap<R> m;
    m.load_pl(mb, c, B, b);
    X = m.then(X);
  }
}

template <int R>
__global__ __launch_bounds__(64) void k_gp_bscan_w(GpArgs a, GpPlan p) {
  const unsigned b = blockIdx.x;
  const int lane = threadIdx.x;
  const long long B = a.B, NC = p.NC;
  const double *mb = (const double *)(a.ws + p.map_off);
  double *bin = (double *)(a.ws + p.bin_off);
  const double *nb = (const double *)(a.ws + p.nll_off);
  const int32_t *cb = (const int32_t *)(a.ws + p.cnt_off);
  const long long q = (NC + 63) / 64;
  const long long c0 = min(NC, lane * q), c1 = min(NC, c0 + q);
  GapMap<R> F;
  F.set_identity();
  double nll = 0.0;
  int cnt = 0;
  for (long long c = c0; c < c1; ++c) {
    GapMap<R> m;
    m.load_pl(mb, c, B, b);
    F = F.then(m);
    nll += pl(nb, c, B, b);
    cnt += pl(cb, c, B, b);
  }
  // the lanes' sums in ascending lane order: the runs ascend with the lane
  double tn = 0.0;
  int tc = 0;
#pragma unroll 1
  for (int l = 0; l < 64; ++l) {
    tn += __shfl(nll, l, 64);
    tc += __shfl(cnt, l, 64);
  }
  if (lane == 0) {
    if (a.nll) a.nll[b] = tn;
    if (a.nobs) a.nobs[b] = tc;
  }
#pragma unroll 1
  for (int k = 1; k < 64; k <<= 1) {
    const GapMap<R> o = F.shfl_down(k);
    const GapMap<R> m = F.then(o);
    if (lane + k < 64) F = m;
  }
  GapMap<R> X = F.shfl_down(1);
  if (lane == 63) X.set_identity();
  for (long long c = c1 - 1; c >= c0; --c) {
    if (c + 1 < NC) gp_store_back<R>(bin, c, B, b, X);
    GapMap<R> m;
    m.load_pl(mb, c, B, b);
    X = m.then(X);
  }
}

// ===========================================================================
// G5: right to left over the chunk: ms_t, Vs_t and their projections
// ===========================================================================
template <int R, bool UNI>
__global__ __launch_bounds__(kBlock) void k_gp_final(GpArgs a, GpPlan p) {
  Lane<UNI> ln;
  if (!ln.init(a.B, p.NC)) return;
  const long long c = ln.c;
  const unsigned b = ln.b;
  const long long B = a.B, TT = a.T;
  const int n = a.n;
  constexpr int S = Sym<R>::len, SL = R + S;
  using L = ParamLayout<R, 0>;
  const double *pp = a.params + (long long)b * param_stride<R, 0>(n);
  double A[R][R], Q[R][R], ms[R], V[R][R];
  load_mat<R, R>(pp + L::A, A);
  load_mat<R, R>(pp + L::Q, Q);
  const double *Cm = pp + L::C, *off = Cm + (long long)n * R;
  const double *mbuf = (const double *)(a.ws + p.m_off);
  const double *pbuf = (const double *)(a.ws + p.p_off);
  const long long s = c * p.L, e = min(TT, s + p.L);
  if (e < TT) {
    const double *bin = (const double *)(a.ws + p.bin_off);
    gp_load_vec<R>(bin, c * SL, B, b, ms);
    pv_load_sym<R>(bin, c * SL + R, B, b, V);
  } else {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      ms[i] = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) V[i][k] = 0.0;
    }
  }
  double *oo = a.out + (long long)b * a.ob;
  double *vo = a.pvar ? a.pvar + (long long)b * a.ob : nullptr;
  for (long long t = e - 1; t >= s; --t) {
    double m[R], P[R][R];
    gp_load_vec<R>(mbuf, t * R, B, b, m);
    pv_load_sym<R>(pbuf, t * S, B, b, P);
    if (t + 1 < TT) {
      double J[R][R], d[R], D[R][R], Vn[R][R], mn[R];
      gp_rts<R>(m, P, A, Q, J, d, D);  // (G3 has flagged a singular S_t: the same expressions)
      pv_congruence<R>(J, V, D, Vn);
#pragma unroll
      for (int i = 0; i < R; ++i) {
        double sm = d[i];
#pragma unroll
        for (int k = 0; k < R; ++k) sm = fma(J[i][k], ms[k], sm);
        mn[i] = sm;
      }
#pragma unroll
      for (int i = 0; i < R; ++i) {
        ms[i] = mn[i];
#pragma unroll
        for (int k = 0; k < R; ++k) V[i][k] = Vn[i][k];
      }
    } else {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        ms[i] = m[i];
#pragma unroll
        for (int k = 0; k < R; ++k) V[i][k] = P[i][k];
      }
    }
    if (a.ms) store_vec<R>(a.ms + ((long long)b * TT + t) * R, ms);
    if (a.Vs) store_mat<R, R>(a.Vs + ((long long)b * TT + t) * (R * R), V);
    for (int j = 0; j < n; ++j) {
      double cr[R];
#pragma unroll
      for (int i = 0; i < R; ++i) cr[i] = Cm[j * R + i];
      double cm = 0.0;
#pragma unroll
      for (int i = 0; i < R; ++i) cm = fma(cr[i], ms[i], cm);
      oo[t * a.ot + j * a.oj] = cm + off[j];
      if (vo) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
          double vc = 0.0;
#pragma unroll
          for (int k = 0; k < R; ++k) vc = fma(V[i][k], cr[k], vc);
          acc = fma(cr[i], vc, acc);
        }
        vo[t * a.ot + j * a.oj] = acc;
      }
    }
  }
}

// ===========================================================================
// host launcher
// ===========================================================================
template <int R>
int launch_gp(const GpArgs &a, GpPlan p) {
  const bool uni = uniform_lanes(a.B);
  const unsigned gch = lane_grid(p.NC, a.B);
  const bool wave_scan = p.NC > wave_scan_chunks();
  p.evsrc = yev_ev_planes(a.obs, a.dtype, a.B, a.T, a.n);
  int rc;
  prof_call_begin();
  prof_mark(a.stream, "k_gp_elem");
  rc = dispatch_input(a.dtype, a.E, [&](auto ttag, auto Ec) -> int {
    using T = decltype(ttag);
    constexpr int EE = decltype(Ec)::value;
    launch_uni(uni, k_gp_elem<R, T, EE, true>, k_gp_elem<R, T, EE, false>, gch, a.stream, a, p);
    return check_launch("k_gp_elem");
  });
  if (rc) return rc;
  if (p.NC > 1) {
    prof_mark(a.stream, "k_gp_fscan");
    launch_scan(wave_scan, k_gp_fscan<R>, k_gp_fscan_w<R>, a.B, a.stream, a, p);
    if ((rc = check_launch("k_gp_fscan"))) return rc;
  }
  prof_mark(a.stream, "k_gp_rerun");
  launch_uni(uni, k_gp_rerun<R, true>, k_gp_rerun<R, false>, gch, a.stream, a, p);
  if ((rc = check_launch("k_gp_rerun"))) return rc;
  // (a single chunk too: G4 writes nll and nobs)
  prof_mark(a.stream, "k_gp_bscan");
  launch_scan(wave_scan, k_gp_bscan<R>, k_gp_bscan_w<R>, a.B, a.stream, a, p);
  if ((rc = check_launch("k_gp_bscan"))) return rc;
  prof_mark(a.stream, "k_gp_final");
  launch_uni(uni, k_gp_final<R, true>, k_gp_final<R, false>, gch, a.stream, a, p);
  prof_call_end(a.stream);
  return check_launch("k_gp_final");
}

}  // namespace eks
