// Likelihood sweep (eks_nll_sweep): the innovation NLL (compute_nll, SURVEY.md
// §8 A5) of K candidate models for each of B trajectories, the members read
// and reduced once for all candidates.
//
// With R_t = diag(ev[t]) and z_t = y_t - offset the n observations of a step
// enter the likelihood of any model (m0, S0, A, Q) with this C only through
// the r x r quantities
//     W_t = C^T R_t^-1 C = L_t D_t L_t^T   (L unit lower triangular, D diagonal)
//     w_t = C^T R_t^-1 z_t
// and are equivalent to r scalar observations that do not depend on the
// candidate:
//     rows c~_i = row i of L_t^T,  values y~_i = (L_t^-1 w_t)_i / D_i,  variances 1 / D_i
// plus a model-free constant
//     kappa_t = 1/2 [(n - r) log 2 pi + sum_j log ev[t][j] + sum_i log D_i + rho_t],
//     rho_t   = sum_j (z_j - c_j x^_t)^2 / ev[t][j],   x^_t = L_t^-T y~_t
// (the residual of the weighted least-squares fit: no cancelling quadratic
// terms).  NLL(model) = sum_t kappa_t + NLL of the r-row scalar filter over
// (c~, y~, 1/D).  For C = I the rows are the original observations, kappa = 0.
//
// Three launches, launch boundaries the only synchronisation:
//
//  S1 k_sw_reduce  (chunk, trajectory) lanes: per step the ensemble, W_t, w_t,
//                  the LDL^T and kappa_t; time-major planes of B values,
//                  r (r + 3) / 2 doubles per step: the strict upper part of
//                  L_t^T, then y~, then 1 / D; the chunk's kappa share, summed
//                  in step order.  C and offset come from candidate 0's row.
//  S2 k_sw_elem    (chunk, candidate * B + b) lanes: the chunk's filtering
//                  element (Elem<R>) and its likelihood constant from the
//                  planes, r scalar rows per step whatever n is (chunk 0: the
//                  plain filter from the candidate's (m0, S0))
//  S3 k_sw_scan    per (candidate, trajectory): the chunk elements folded left
//                  to right (compose_state), elem_nll_share of every chunk
//                  added in ascending chunk order, then the kappa shares in
//                  ascending chunk order.  One lane per row up to
//                  wave_scan_chunks() chunks; above, one wave per row (lane l
//                  folds a contiguous run of ceil(NC / 64) chunks, a 64-lane
//                  shuffle scan gives the state entering its run, the lanes'
//                  partial sums are added by a fixed butterfly): the
//                  association order depends on NC only.
//
// A single chunk (L >= T) is the sequential form: S1, then k_sw_seq, one lane
// per row running the r-row filter over the planes.
//
// Status.  S1 flags EKS_STATUS_SCAN on every candidate of a trajectory with an
// exact observation (ev == 0: one member, or identical members), a
// non-positive pivot D_i (rank-deficient C, n < r), or a non-finite pivot
// that did not come from a NaN ev; its planes and kappa share are NaN, so all
// its NLLs are NaN: this path does not serve the row, fall back to the filter
// (eks_smooth with out = NULL).  A NaN member makes the NLL NaN and sets no
// bit.  S2 flags EKS_STATUS_BAD_MODEL on a row whose C or offset differ
// bitwise from candidate 0's.  A singular step (innovation variance <= 0, a
// singular I + P J of a composition) sets EKS_STATUS_SINGULAR.
#pragma once
#include "host_api.hpp"

namespace eks {

extern long long g_sweep_chunk;  // forced chunk length (EKS_DBG_SWEEP_CHUNK), 0: automatic

struct SwArgs {
  const void *obs;
  int dtype;
  long long B, T;
  int E, n;
  long long sb, st, se, sj;
  int median;
  const double *params;
  long long K;
  double *nll;
  char *ws;
  int32_t *status;
  hipStream_t stream;
};

// workspace arrays (doubles, time-major planes)
struct SwPlan {
  long long L = 0, NC = 0;
  size_t row_off = 0;   // scalar rows   T  x r (r + 3) / 2 planes of B
  size_t elem_off = 0;  // elements      NC x (Elem<R>::len + 1) planes of K * B
  size_t kap_off = 0;   // kappa shares  NC planes of B
  size_t total = 0;
  const char *evsrc = nullptr;  // the caller's ev planes (y / ev input)
};

inline int sw_row_len(int r) { return r * (r + 3) / 2; }

// Chunk length as launched: a multiple of 8, one chunk when it covers T.
// Automatic: twice the filter-only call's length for B trajectories.  The
// first form, that call's length for K * B trajectories, was retuned from
// measurements (tools/sweep_timing.py --chunk): S1 has B * NC
// lanes, not K * B * NC, so B governs how the chip fills (2176 x 10 000,
// K = 8: L = 632 left S1 at 1.97 ms, 0.92 ms at L = 128), and S3's wave per
// row costs more per chunk than the filter-only scan, which moves the
// optimum up (17 x 100 000, (2,2), K = 16: 0.85 / 0.54 / 0.45 / 0.55 ms at
// L = 16 / 32 / 64 / 128; 17 x 50 000, (3,8): 0.94 / 0.86 / 0.93 at 16 / 32 /
// 64; the shard: 2.91 / 2.23 / 2.20 at 64 / 128 / 256).
inline long long sw_chunk_len(long long B, long long T, int r) {
  return chunk_len_rule(g_sweep_chunk, 2 * call_chunk_len(B, T, r, false, 0), 0, 0, B, T, r);
}

inline SwPlan sw_make_plan(long long B, long long K, long long T, int r, long long L) {
  SwPlan p;
  p.L = L;
  p.NC = (T + L - 1) / L;
  Carver ws;
  auto take = [&](size_t doubles) { return ws.take(doubles * 8); };
  p.row_off = take((size_t)T * (size_t)B * (size_t)sw_row_len(r));
  p.elem_off = take((size_t)p.NC * (size_t)K * (size_t)B * (size_t)(elem_len(r) + 1));
  p.kap_off = take((size_t)p.NC * (size_t)B);
  p.total = ws.off;
  return p;
}

// the r scalar observations of one step: rows of L^T, values, variances
template <int R>
struct SwStep {
  double C[R][R], y[R], rv[R];
};

template <int R>
EKS_DEV void sw_load_step(const double *rows, long long t, long long B, unsigned b, SwStep<R> &s) {
  constexpr int NP = R * (R + 3) / 2, NU = R * (R - 1) / 2;
  int k = 0;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (j > i)
        s.C[i][j] = pl(rows, t * NP + (k++), B, b);
      else
        s.C[i][j] = (i == j) ? 1.0 : 0.0;
    }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    s.y[i] = pl(rows, t * NP + NU + i, B, b);
    s.rv[i] = pl(rows, t * NP + NU + R + i, B, b);
  }
}

// every entry of the state and the element finite (a NaN input propagates as
// NaN and is not an error: only finite operands can report a singular step)
template <int R>
EKS_DEV bool sw_finite(const double (&m)[R], const double (&P)[R][R], const Elem<R> &E) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    s += fabs(m[i]) + fabs(E.bb[i]) + fabs(E.eta[i]);
#pragma unroll
    for (int j = 0; j < R; ++j) s += fabs(P[i][j]) + fabs(E.Ab[i][j]) + fabs(E.Cb[i][j]) + fabs(E.Jb[i][j]);
  }
  return s < __builtin_inf();
}

// C and offset of `row` equal candidate 0's bit for bit
template <int R>
EKS_DEV bool sw_same_obs_model(const double *params, long long row, unsigned b, int n) {
  const long long st = param_stride<R, 0>(n);
  const double *p0 = params + (long long)b * st + ParamLayout<R, 0>::C;
  const double *p1 = params + row * st + ParamLayout<R, 0>::C;
  bool same = true;
  for (int k = 0; k < n * (R + 1); ++k)
    same = same && (__double_as_longlong(p0[k]) == __double_as_longlong(p1[k]));
  return same;
}

// the plain filter over steps [s, e) of the scalar rows
template <int R>
EKS_DEV void sw_filter_run(const double *rows, long long s, long long e, long long B, unsigned b,
                           const double (&A)[R][R], const double (&Q)[R][R], double (&m)[R],
                           double (&P)[R][R], NllAcc &acc, bool &ok) {
  SwStep<R> cur, nxt;
  sw_load_step<R>(rows, s, B, b, nxt);
  for (long long t = s; t < e; ++t) {
    cur = nxt;
    sw_load_step<R>(rows, min(t + 1, e - 1), B, b, nxt);  // next step in flight
    if (t > 0) kf_predict<R, kAGen>(m, P, A, Q);
    kf_update<R, R, kCGen>(m, P, cur.C, cur.y, cur.rv, acc, ok);
  }
}

// ===========================================================================
// S1: the scalar rows and the kappa share of a chunk
// T: float / double members, or YevIn<float / double> (the y / ev planes; E unused)
// ===========================================================================
template <int R, typename T, int E, bool UNI>
__global__ __launch_bounds__(kBlock) void k_sw_reduce(SwArgs a, SwPlan p) {
  Lane<UNI> ln;
  if (!ln.init(a.B, p.NC)) return;
  const long long c = ln.c;
  const unsigned b = ln.b;
  const long long B = a.B, TT = a.T;
  const int n = a.n;
  constexpr bool kYev = is_yev<T>::value;
  using MT = typename yev_y<T>::type;
  constexpr int NP = R * (R + 3) / 2, NU = R * (R - 1) / 2;
  const bool median = a.median != 0;
  const double *pp = a.params + (long long)b * param_stride<R, 0>(n);  // candidate 0's row
  const double *Cm = pp + ParamLayout<R, 0>::C, *off = Cm + (long long)n * R;
  const MT *ob = kYev ? (const MT *)a.obs : (const MT *)a.obs + (long long)b * a.sb;
  const double *evp = (const double *)p.evsrc;
  double *rows = (double *)(a.ws + p.row_off);
  const long long s = c * p.L, e = min(TT, s + p.L);
  auto column = [&](long long t, int j, double &z, double &var) {
    double avg;
    if constexpr (kYev) {
      avg = (double)pl(ob, t * n + j, B, b);
      var = pl(evp, t * n + j, B, b);
    } else {
      column_reduce<E, MT>(ob + t * a.st + j * a.sj, a.se, a.E, median, avg, var);
    }
    z = avg - off[j];
  };
  bool bad = false;
  NllAcc acc;
  for (long long t = s; t < e; ++t) {
    double W[R][R], w[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      w[i] = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) W[i][k] = 0.0;
    }
    bool evnan = false;
    for (int j = 0; j < n; ++j) {
      double z, var, cr[R];
      column(t, j, z, var);
      bad = bad || (var == 0.0);
      evnan = evnan || (var != var);
      const double inv = rcp_nr(var);
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
    // W = L D L^T with U = L^T: V[i][j] = D_i U[i][j] = W[i][j] - sum_{k<i} U[k][i] V[k][j]
    double U[R][R], V[R][R], D[R], Di[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
#pragma unroll
      for (int j = i; j < R; ++j) {
        double v = W[i][j];
#pragma unroll
        for (int k = 0; k < i; ++k) v = fma(-U[k][i], V[k][j], v);
        V[i][j] = v;
      }
      D[i] = V[i][i];
      if (D[i] <= 0.0)
        bad = true;
      else if (!(fabs(D[i]) < __builtin_inf()) && !evnan)
        bad = true;
      Di[i] = rcp_nr(D[i]);
#pragma unroll
      for (int j = i + 1; j < R; ++j) U[i][j] = V[i][j] * Di[i];
    }
    // y~ = D^-1 L^-1 w (forward substitution), x^ = L^-T y~ (backward)
    double u[R], yt[R], xh[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      double v = w[i];
#pragma unroll
      for (int k = 0; k < i; ++k) v = fma(-U[k][i], u[k], v);
      u[i] = v;
      yt[i] = v * Di[i];
    }
#pragma unroll
    for (int i = R - 1; i >= 0; --i) {
      double v = yt[i];
#pragma unroll
      for (int j = i + 1; j < R; ++j) v = fma(-U[i][j], xh[j], v);
      xh[i] = v;
    }
    // rho_t and sum_j log ev: the columns again (the members come from cache)
    for (int j = 0; j < n; ++j) {
      double z, var;
      column(t, j, z, var);
      double rs = z;
#pragma unroll
      for (int k = 0; k < R; ++k) rs = fma(-Cm[j * R + k], xh[k], rs);
      acc.add(rs, var, rcp_nr(var));
      if ((j & 7) == 7) acc.renorm();
    }
#pragma unroll
    for (int i = 0; i < R; ++i) acc.mant *= D[i];
    acc.renorm();
    const double nan = __builtin_nan("");
    int k = 0;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = i + 1; j < R; ++j) pl(rows, t * NP + (k++), B, b) = bad ? nan : U[i][j];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      pl(rows, t * NP + NU + i, B, b) = bad ? nan : yt[i];
      pl(rows, t * NP + NU + R + i, B, b) = bad ? nan : Di[i];
    }
  }
  pl((double *)(a.ws + p.kap_off), c, B, b) =
      bad ? __builtin_nan("") : acc.value((double)(e - s) * (double)(n - R));
  if (bad)
    for (long long k = 0; k < a.K; ++k) flag(a.status, k * B + b, EKS_STATUS_SCAN);
}

// ===========================================================================
// S2: the chunk's filtering element and likelihood constant of every row
// ===========================================================================
template <int R, bool UNI>
__global__ __launch_bounds__(kBlock) void k_sw_elem(SwArgs a, SwPlan p) {
  const long long B = a.B, KB = a.K * a.B, TT = a.T;
  Lane<UNI> ln;
  if (!ln.init(KB, p.NC)) return;
  const long long c = ln.c;
  const unsigned row = ln.b;
  const unsigned b = row % (unsigned)B;
  constexpr int EL = Elem<R>::len;
  using L = ParamLayout<R, 0>;
  const double *pp = a.params + (long long)row * param_stride<R, 0>(a.n);
  double A[R][R], Q[R][R];
  load_mat<R, R>(pp + L::A, A);
  load_mat<R, R>(pp + L::Q, Q);
  const double *rows = (const double *)(a.ws + p.row_off);
  const long long s = c * p.L, e = min(TT, s + p.L);
  bool ok = true;
  NllAcc acc;
  Elem<R> El;
  El.set_identity();
  if (c == 0) {
    if (row >= B && !sw_same_obs_model<R>(a.params, row, b, a.n))
      flag(a.status, row, EKS_STATUS_BAD_MODEL);
    // chunk 0: the plain filter from the prior, summarised as the known
    // filtered state (Ab = 0, bb = m, Cb = P)
    double m[R], P[R][R];
    load_vec<R>(pp + L::m0, m);
    load_mat<R, R>(pp + L::S0, P);
    sw_filter_run<R>(rows, s, e, B, b, A, Q, m, P, acc, ok);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      El.bb[i] = m[i];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        El.Ab[i][j] = 0.0;
        El.Cb[i][j] = P[i][j];
      }
    }
  } else {
    SwStep<R> cur, nxt;
    sw_load_step<R>(rows, s, B, b, nxt);
    for (long long t = s; t < e; ++t) {
      cur = nxt;
      sw_load_step<R>(rows, min(t + 1, e - 1), B, b, nxt);  // next step in flight
      elem_absorb<R, R, kAGen, kCGen>(El, A, Q, cur.C, cur.y, cur.rv, ok, &acc);
    }
  }
  double *eb = (double *)(a.ws + p.elem_off) + c * (EL + 1) * KB + row;
  El.store(eb, KB);
  eb[(long long)EL * KB] = acc.value((double)(e - s) * R);
  if (!ok) flag(a.status, row, EKS_STATUS_SINGULAR);
}

template <int R>
EKS_DEV double sw_load_elem(const double *ebase, long long c, long long KB, long long row,
                            Elem<R> &El) {
  constexpr int EL = Elem<R>::len;
  const double *eb = ebase + c * (EL + 1) * KB + row;
  El.load(eb, KB);
  return eb[(long long)EL * KB];
}

// the share of chunk c given the filtered state before it, and that state
// moved across the chunk
template <int R>
EKS_DEV double sw_chunk_share(double (&m)[R], double (&P)[R][R], const Elem<R> &El, double kc,
                              bool advance, bool &singular) {
  const bool fin = sw_finite<R>(m, P, El);
  bool ok = true;
  const double sh = elem_nll_share<R>(m, P, El, kc, ok);
  if (advance) ok = compose_state<R>(m, P, El) && ok;
  singular = singular || (!ok && fin);
  return sh;
}

// ===========================================================================
// S3: the NLL of every row.  One lane per row ...
// ===========================================================================
template <int R>
__global__ __launch_bounds__(64) void k_sw_scan(SwArgs a, SwPlan p) {
  const long long row = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long B = a.B, KB = a.K * a.B;
  if (row >= KB) return;
  const unsigned b = (unsigned)(row % B);
  const double *ebase = (const double *)(a.ws + p.elem_off);
  const double *kap = (const double *)(a.ws + p.kap_off);
  double m[R], P[R][R];
  Elem<R> El;
  double nll = sw_load_elem<R>(ebase, 0, KB, row, El);  // chunk 0: its constant is its share
  El.state(m, P);
  bool singular = false;
  for (long long c = 1; c < p.NC; ++c) {
    const double kc = sw_load_elem<R>(ebase, c, KB, row, El);
    nll += sw_chunk_share<R>(m, P, El, kc, c + 1 < p.NC, singular);
  }
  for (long long c = 0; c < p.NC; ++c) nll += pl(kap, c, B, b);
  a.nll[row] = nll;
  if (singular) flag(a.status, row, EKS_STATUS_SINGULAR);
}

EKS_DEV double sw_wave_sum(double v) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) v += __shfl_xor(v, k, 64);
  return v;
}

// ... or one wave per row
template <int R>
__global__ __launch_bounds__(64) void k_sw_scan_w(SwArgs a, SwPlan p) {
  const long long row = blockIdx.x;
  const int lane = threadIdx.x;
  const long long B = a.B, KB = a.K * a.B, NC = p.NC;
  const unsigned b = (unsigned)(row % B);
  const double *ebase = (const double *)(a.ws + p.elem_off);
  const double *kap = (const double *)(a.ws + p.kap_off);
  const long long q = (NC + 63) / 64;
  const long long c0 = min(NC, lane * q), c1 = min(NC, c0 + q);
  bool singular = false;
  // the element of this lane's run, then the prefix of the runs before it
  Elem<R> F, El;
  F.set_identity();
  for (long long c = c0; c < c1; ++c) {
    sw_load_elem<R>(ebase, c, KB, row, El);
    Elem<R> t;
    singular = !compose_elem<R>(F, El, t) || singular;
    F = t;
  }
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const Elem<R> o = shfl_elem<R, true>(F, k);
    Elem<R> t;
    const bool ok2 = compose_elem<R>(o, F, t);
    if (lane >= k) {
      F = t;
      singular = singular || !ok2;
    }
  }
  // the prefix up to the run before this lane's holds chunk 0 (Ab = 0): its
  // (bb, Cb) is the filtered state entering the run
  const Elem<R> X = shfl_elem<R, true>(F, 1);
  double m[R], P[R][R];
  X.state(m, P);
  double part = 0.0, kpart = 0.0;
  for (long long c = c0; c < c1; ++c) {
    const double kc = sw_load_elem<R>(ebase, c, KB, row, El);
    if (c == 0) {
      part = kc;  // chunk 0: its constant is its share
      El.state(m, P);
    } else {
      part += sw_chunk_share<R>(m, P, El, kc, c + 1 < c1, singular);
    }
    kpart += pl(kap, c, B, b);
  }
  const double nll = sw_wave_sum(part) + sw_wave_sum(kpart);
  // (a NaN row reports no singular composition: the compositions of NaN
  // elements are not exactly singular, and sw_chunk_share tests finiteness)
  const bool any = __builtin_amdgcn_ballot_w64(singular && nll == nll) != 0;
  if (lane == 0) {
    a.nll[row] = nll;
    if (any) flag(a.status, row, EKS_STATUS_SINGULAR);
  }
}

// ===========================================================================
// the sequential form (one chunk): one lane per row over the planes
// ===========================================================================
template <int R>
__global__ __launch_bounds__(64) void k_sw_seq(SwArgs a, SwPlan p) {
  const long long row = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long B = a.B, KB = a.K * a.B;
  if (row >= KB) return;
  const unsigned b = (unsigned)(row % B);
  using L = ParamLayout<R, 0>;
  const double *pp = a.params + row * param_stride<R, 0>(a.n);
  double A[R][R], Q[R][R], m[R], P[R][R];
  load_mat<R, R>(pp + L::A, A);
  load_mat<R, R>(pp + L::Q, Q);
  load_vec<R>(pp + L::m0, m);
  load_mat<R, R>(pp + L::S0, P);
  if (row >= B && !sw_same_obs_model<R>(a.params, row, b, a.n))
    flag(a.status, row, EKS_STATUS_BAD_MODEL);
  bool ok = true;
  NllAcc acc;
  sw_filter_run<R>((const double *)(a.ws + p.row_off), 0, a.T, B, b, A, Q, m, P, acc, ok);
  a.nll[row] = acc.value((double)a.T * R) + pl((const double *)(a.ws + p.kap_off), 0, B, b);
  if (!ok) flag(a.status, row, EKS_STATUS_SINGULAR);
}

// ===========================================================================
// host launcher
// ===========================================================================
template <int R>
int launch_sw(const SwArgs &a, SwPlan p) {
  const long long KB = a.K * a.B;
  const bool uni = uniform_lanes(a.B), uni_e = uniform_lanes(KB);
  const unsigned g1 = lane_grid(p.NC, a.B), g2 = lane_grid(p.NC, KB);
  p.evsrc = yev_ev_planes(a.obs, a.dtype, a.B, a.T, a.n);
  int rc;
  prof_call_begin();
  prof_mark(a.stream, "k_sw_reduce");
  rc = dispatch_input(a.dtype, a.E, [&](auto ttag, auto Ec) -> int {
    using T = decltype(ttag);
    constexpr int EE = decltype(Ec)::value;
    launch_uni(uni, k_sw_reduce<R, T, EE, true>, k_sw_reduce<R, T, EE, false>, g1, a.stream, a, p);
    return check_launch("k_sw_reduce");
  });
  if (rc) return rc;
  if (p.NC == 1) {
    prof_mark(a.stream, "k_sw_seq");
    hipLaunchKernelGGL((k_sw_seq<R>), dim3(grid_for(KB, 64)), dim3(64), 0, a.stream, a, p);
    prof_call_end(a.stream);
    return check_launch("k_sw_seq");
  }
  prof_mark(a.stream, "k_sw_elem");
  launch_uni(uni_e, k_sw_elem<R, true>, k_sw_elem<R, false>, g2, a.stream, a, p);
  if ((rc = check_launch("k_sw_elem"))) return rc;
  prof_mark(a.stream, "k_sw_scan");
  launch_scan(p.NC > wave_scan_chunks(), k_sw_scan<R>, k_sw_scan_w<R>, KB, a.stream, a, p);
  prof_call_end(a.stream);
  return check_launch("k_sw_scan");
}

}  // namespace eks
