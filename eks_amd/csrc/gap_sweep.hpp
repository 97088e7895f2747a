// Likelihood sweep through missing observations (eks_nll_sweep_gaps): the NLL
// over the observed entries (gap_smooth.hpp's header: the missing rule, the
// information-form filter and its NLL) of K candidate models for each of B
// trajectories, the members read and reduced once for all candidates.
//
// eks_nll_sweep reduces a step to r scalar rows through the LDL^T of W_t and
// needs W_t positive definite; here W_t may be rank-deficient or zero, so the
// candidates read the sums W_t, w_t, kappa_t themselves, Sym + r + 1 doubles
// per step, and run gap_smooth.hpp's step functions on them.  Row k * B + b of
// `params` is candidate k of trajectory b; candidates may differ in m0, S0, A
// and Q, and share candidate 0's C and offset bit for bit.
//
// Five launches, launch boundaries the only synchronisation, no atomics but
// the status bits; the association order is a function of NC only:
//
//  k_gs_reduce  (chunk, trajectory) lanes: members (or the y / ev planes) ->
//               W_t, w_t, kappa_t planes of B values (gp_step_sums, C and
//               offset of candidate 0's row) and the chunk's observed count
//  k_gs_elem    (chunk, row) lanes over the K * B rows: the chunk's Elem<R>
//               from the planes, every step absorbed on the right (gp_absorb);
//               chunk 0: the plain filter from the row's (m0, S0), a constant
//               element
//  k_gs_fscan   per row: prefix over the chunk elements, (m, P) entering every
//               chunk; one lane per row while NC <= wave_scan_chunks(), one
//               wave per row above (gp_fscan_lane / gp_fscan_wave)
//  k_gs_share   (chunk, row) lanes: gp_filter_step from the entering state
//               over the planes; only the chunk's NLL share is kept
//  k_gs_sum     per row: the shares in ascending chunk order -> nll[row]; per
//               trajectory the counts -> nobs[b]; one lane per row, or one
//               wave per row as the scan (each lane its run, then the lanes in
//               ascending order)
//
// A single chunk (L >= T) is the sequential form: k_gs_reduce, then k_gs_seq,
// one lane per row running gp_filter_step over the planes.
//
// Status.  k_gs_reduce flags EKS_STATUS_SCAN on every candidate of a
// trajectory with an observed ev == 0; its sums are NaN from that step on and
// so are its NLLs.  A row whose C or offset differ bitwise from candidate 0's
// gets EKS_STATUS_BAD_MODEL.  A singular I + P W or composition sets
// EKS_STATUS_SINGULAR; NaN operands set nothing.  A trajectory with nothing
// observed has W_t = w_t = kappa_t = 0 everywhere: every share is
// 1/2 log det(I) = 0 and its NLL is exactly 0.0.
#pragma once
#include "gap_smooth.hpp"
#include "nll_sweep.hpp"

namespace eks {

extern long long g_gaps_sweep_chunk;  // forced chunk length (EKS_DBG_GAPS_SWEEP_CHUNK), 0: automatic

struct GsArgs {
  const void *obs;
  int dtype;
  long long B, T;
  int E, n;
  long long sb, st, se, sj;
  int median;
  const double *params;
  long long K;
  double *nll;
  int32_t *nobs;
  char *ws;
  int32_t *status;
  hipStream_t stream;
};

// workspace arrays (time-major planes; doubles but cnt, int32)
struct GsPlan {
  long long L = 0, NC = 0;
  size_t w_off = 0;     // W_t       T  x Sym<R>::len   planes of B
  size_t sw_off = 0;    // w_t       T  x R             planes of B
  size_t kap_off = 0;   // kappa_t   T                  planes of B
  size_t elem_off = 0;  // elements  NC x Elem<R>::len  planes of K * B
  size_t sin_off = 0;   // (m, P) entering a chunk   NC x (R + Sym<R>::len) planes of K * B
  size_t nll_off = 0;   // NLL shares         NC planes of K * B
  size_t cnt_off = 0;   // observed entries   NC planes of B (int32)
  size_t total = 0;
  const char *evsrc = nullptr;  // the caller's ev planes (y / ev input)
};

// Chunk length as launched: a multiple of 8, one chunk when it covers T.
// Automatic: sw_chunk_len's rule, twice the filter-only call's length for B
// trajectories (k_gs_reduce has B * NC lanes like S1 of nll_sweep.hpp).  With
// few trajectories it is not shorter than c sqrt(T), gp_chunk_len's form:
// k_gs_reduce's B * NC lanes do not fill the chip, so its time grows with L,
// while the wave-per-row scan's falls with NC = T / L whatever K * B is.
// From tools/gaps_sweep_timing.py --chunk, total ms of the call:
//   one pupil video of 1 000 000 frames, (3,8), K = 64:
//     7.67 / 4.53 / 3.31 / 3.24 / 3.42 / 3.49 at L = 32 / 64 / 96 / 128 / 152 / 200
//     (32 is the first rule's: k_gs_fscan 5.69 ms of 64 waves)
//   17 x 100 000, (2,2), K = 16: 0.72 / 0.59 / 0.59 / 0.64 / 0.80 at 32 / 64 / 96 / 128 / 200
//   17 x 50 000, (3,8), K = 16:  0.98 / 1.00 / 1.06 / 1.15 / 1.32 at 32 / 40 / 64 / 96 / 128
// c = 0.20 at r = 2 and 0.13 at r = 3 give 64, 32 and 136 there.  The shard
// (2176 x 10 000, uniform lanes) keeps the first rule's 176: 5.49 / 3.97 /
// 3.06 / 2.94 / 2.92 at 32 / 64 / 128 / 176 / 200.
inline long long gs_chunk_len(long long B, long long T, int r) {
  return chunk_len_rule(g_gaps_sweep_chunk, 2 * call_chunk_len(B, T, r, false, 0), 0.20, 0.13, B, T,
                        r);
}

inline GsPlan gs_make_plan(long long B, long long K, long long T, int r, long long L) {
  GsPlan p;
  p.L = L;
  p.NC = (T + L - 1) / L;
  const size_t S = (size_t)pv_sym_len(r), R = (size_t)r, Bz = (size_t)B, KB = (size_t)(K * B),
               NC = (size_t)p.NC;
  Carver ws;
  auto take = [&](size_t planes, size_t width, size_t bytes) {
    return ws.take(planes * width * bytes);
  };
  p.w_off = take((size_t)T * S, Bz, 8);
  p.sw_off = take((size_t)T * R, Bz, 8);
  p.kap_off = take((size_t)T, Bz, 8);
  p.elem_off = take(NC * (size_t)elem_len(r), KB, 8);
  p.sin_off = take(NC * (R + S), KB, 8);
  p.nll_off = take(NC, KB, 8);
  p.cnt_off = take(NC, Bz, 4);
  p.total = ws.off;
  return p;
}

// the model of a row and the state entering its chunk 0
template <int R>
EKS_DEV void gs_load_model(const double *pp, double (&A)[R][R], double (&Q)[R][R]) {
  using L = ParamLayout<R, 0>;
  load_mat<R, R>(pp + L::A, A);
  load_mat<R, R>(pp + L::Q, Q);
}

// gp_filter_step over steps [s, e) of the planes of trajectory b
template <int R>
EKS_DEV bool gs_filter_run(const char *ws, const GsPlan &p, long long s, long long e, long long B,
                           unsigned b, const double (&A)[R][R], const double (&Q)[R][R],
                           double (&m)[R], double (&P)[R][R], double &nll) {
  constexpr int S = Sym<R>::len;
  const double *wbuf = (const double *)(ws + p.w_off);
  const double *swbuf = (const double *)(ws + p.sw_off);
  const double *kbuf = (const double *)(ws + p.kap_off);
  bool ok = true;
  for (long long t = s; t < e; ++t) {
    double W[R][R], w[R];
    pv_load_sym<R>(wbuf, t * S, B, b, W);
    gp_load_vec<R>(swbuf, t * R, B, b, w);
    const double kappa = pl(kbuf, t, B, b);
    ok = gp_filter_step<R>(t > 0, A, Q, W, w, kappa, m, P, &nll) && ok;
  }
  return ok;
}

// ===========================================================================
// k_gs_reduce: W_t, w_t, kappa_t planes and the observed count of a chunk
// T: float / double members, or YevIn<float / double> (the y / ev planes; E unused)
// ===========================================================================
template <int R, typename T, int E, bool UNI>
__global__ __launch_bounds__(kBlock) void k_gs_reduce(GsArgs a, GsPlan p) {
  Lane<UNI> ln;
  if (!ln.init(a.B, p.NC)) return;
  const long long c = ln.c;
  const unsigned b = ln.b;
  const long long B = a.B, TT = a.T;
  const int n = a.n;
  constexpr int S = Sym<R>::len;
  constexpr bool kYev = is_yev<T>::value;
  using MT = typename yev_y<T>::type;
  const bool median = a.median != 0;
  const double *pp = a.params + (long long)b * param_stride<R, 0>(n);  // candidate 0's row
  const double *Cm = pp + ParamLayout<R, 0>::C, *off = Cm + (long long)n * R;
  const MT *ob = kYev ? (const MT *)a.obs : (const MT *)a.obs + (long long)b * a.sb;
  const double *evp = (const double *)p.evsrc;
  double *wbuf = (double *)(a.ws + p.w_off);
  double *swbuf = (double *)(a.ws + p.sw_off);
  double *kbuf = (double *)(a.ws + p.kap_off);
  const long long s = c * p.L, e = min(TT, s + p.L);
  bool exact = false;
  int count = 0;
  for (long long t = s; t < e; ++t) {
    double W[R][R], w[R], kappa;
    gp_step_sums<R, T, E>(ob, evp, t, B, b, n, a.st, a.se, a.sj, a.E, median, Cm, off, W, w, kappa,
                          count, exact);
    pv_store_sym<R>(wbuf, t * S, B, b, W);
    gp_store_vec<R>(swbuf, t * R, B, b, w);
    pl(kbuf, t, B, b) = kappa;
  }
  pl((int32_t *)(a.ws + p.cnt_off), c, B, b) = count;
  if (exact)
    for (long long k = 0; k < a.K; ++k) flag(a.status, k * B + b, EKS_STATUS_SCAN);
}

// ===========================================================================
// k_gs_elem: the chunk's filtering element of every row
// ===========================================================================
template <int R, bool UNI>
__global__ __launch_bounds__(kBlock) void k_gs_elem(GsArgs a, GsPlan p) {
  const long long B = a.B, KB = a.K * a.B, TT = a.T;
  Lane<UNI> ln;
  if (!ln.init(KB, p.NC)) return;
  const long long c = ln.c;
  const unsigned row = ln.b;
  const unsigned b = row % (unsigned)B;
  constexpr int S = Sym<R>::len;
  using L = ParamLayout<R, 0>;
  const double *pp = a.params + (long long)row * param_stride<R, 0>(a.n);
  double A[R][R], Q[R][R];
  gs_load_model<R>(pp, A, Q);
  const double *wbuf = (const double *)(a.ws + p.w_off);
  const double *swbuf = (const double *)(a.ws + p.sw_off);
  const long long s = c * p.L, e = min(TT, s + p.L);
  Elem<R> El;
  El.set_identity();
  if (c == 0) {  // the prior as a constant element: the run below is the plain filter
    if (row >= B && !sw_same_obs_model<R>(a.params, row, b, a.n))
      flag(a.status, row, EKS_STATUS_BAD_MODEL);
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
  bool ok = true;
  for (long long t = s; t < e; ++t) {
    double W[R][R], w[R];
    pv_load_sym<R>(wbuf, t * S, B, b, W);
    gp_load_vec<R>(swbuf, t * R, B, b, w);
    ok = gp_absorb<R>(El, t > 0, A, Q, W, w) && ok;
  }
  El.store(&pl((double *)(a.ws + p.elem_off), c * Elem<R>::len, KB, row), KB);
  if (!ok) flag(a.status, row, EKS_STATUS_SINGULAR);
}

// ===========================================================================
// k_gs_fscan: (m, P) entering every chunk of every row.  One lane per row ...
// ===========================================================================
template <int R>
__global__ __launch_bounds__(64) void k_gs_fscan(GsArgs a, GsPlan p) {
  const long long row = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long KB = a.K * a.B;
  if (row >= KB) return;
  const bool ok = gp_fscan_lane<R>((const double *)(a.ws + p.elem_off),
                                   (double *)(a.ws + p.sin_off), KB, p.NC, (unsigned)row);
  if (!ok) flag(a.status, row, EKS_STATUS_SINGULAR);
}

// ... or one wave per row
template <int R>
__global__ __launch_bounds__(64) void k_gs_fscan_w(GsArgs a, GsPlan p) {
  const unsigned row = blockIdx.x;
  const bool ok = gp_fscan_wave<R>((const double *)(a.ws + p.elem_off),
                                   (double *)(a.ws + p.sin_off), a.K * a.B, p.NC, row,
                                   threadIdx.x);
  if (!ok) flag(a.status, row, EKS_STATUS_SINGULAR);
}

// ===========================================================================
// k_gs_share: the chunk's NLL share of every row from its entering state
// ===========================================================================
template <int R, bool UNI>
__global__ __launch_bounds__(kBlock) void k_gs_share(GsArgs a, GsPlan p) {
  const long long B = a.B, KB = a.K * a.B, TT = a.T;
  Lane<UNI> ln;
  if (!ln.init(KB, p.NC)) return;
  const long long c = ln.c;
  const unsigned row = ln.b;
  const unsigned b = row % (unsigned)B;
  constexpr int SL = R + Sym<R>::len;
  using L = ParamLayout<R, 0>;
  const double *pp = a.params + (long long)row * param_stride<R, 0>(a.n);
  double A[R][R], Q[R][R], m[R], P[R][R];
  gs_load_model<R>(pp, A, Q);
  if (c == 0) {
    load_vec<R>(pp + L::m0, m);
    load_mat<R, R>(pp + L::S0, P);
  } else {
    const double *sin = (const double *)(a.ws + p.sin_off);
    gp_load_vec<R>(sin, c * SL, KB, row, m);
    pv_load_sym<R>(sin, c * SL + R, KB, row, P);
  }
  const long long s = c * p.L, e = min(TT, s + p.L);
  double nll = 0.0;
  const bool ok = gs_filter_run<R>(a.ws, p, s, e, B, b, A, Q, m, P, nll);
  pl((double *)(a.ws + p.nll_off), c, KB, row) = nll;
  if (!ok) flag(a.status, row, EKS_STATUS_SINGULAR);
}

// ===========================================================================
// k_gs_sum: nll[row], the shares in ascending chunk order; nobs[b].  One lane
// per row ...
// ===========================================================================
static __global__ __launch_bounds__(64) void k_gs_sum(GsArgs a, GsPlan p) {
  const long long row = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long B = a.B, KB = a.K * a.B;
  if (row >= KB) return;
  const double *nb = (const double *)(a.ws + p.nll_off);
  double nll = 0.0;
  for (long long c = 0; c < p.NC; ++c) nll += pl(nb, c, KB, (unsigned)row);
  a.nll[row] = nll;
  if (row < B && a.nobs) {
    const int32_t *cb = (const int32_t *)(a.ws + p.cnt_off);
    int cnt = 0;
    for (long long c = 0; c < p.NC; ++c) cnt += pl(cb, c, B, (unsigned)row);
    a.nobs[row] = cnt;
  }
}

// ... or one wave per row (the chunk counts of the wave scans): lane l adds its
// contiguous run of ceil(NC / 64) chunks in ascending order, then the lanes'
// sums are added in ascending lane order (the runs ascend with the lane), as
// k_gp_bscan_w adds them
static __global__ __launch_bounds__(64) void k_gs_sum_w(GsArgs a, GsPlan p) {
  const unsigned row = blockIdx.x;
  const int lane = threadIdx.x;
  const long long B = a.B, KB = a.K * a.B, NC = p.NC;
  const double *nb = (const double *)(a.ws + p.nll_off);
  const int32_t *cb = (const int32_t *)(a.ws + p.cnt_off);
  const long long q = (NC + 63) / 64;
  const long long c0 = min(NC, lane * q), c1 = min(NC, c0 + q);
  const bool counts = row < B && a.nobs;
  double nll = 0.0;
  int cnt = 0;
  for (long long c = c0; c < c1; ++c) {
    nll += pl(nb, c, KB, row);
    if (counts) cnt += pl(cb, c, B, row);
  }
  double tn = 0.0;
  int tc = 0;
#pragma unroll 1
  for (int l = 0; l < 64; ++l) {
    tn += __shfl(nll, l, 64);
    tc += __shfl(cnt, l, 64);
  }
  if (lane == 0) {
    a.nll[row] = tn;
    if (counts) a.nobs[row] = tc;
  }
}

// ===========================================================================
// the sequential form (one chunk): one lane per row over the planes
// ===========================================================================
template <int R>
__global__ __launch_bounds__(64) void k_gs_seq(GsArgs a, GsPlan p) {
  const long long row = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long B = a.B, KB = a.K * a.B;
  if (row >= KB) return;
  const unsigned b = (unsigned)(row % B);
  using L = ParamLayout<R, 0>;
  const double *pp = a.params + row * param_stride<R, 0>(a.n);
  double A[R][R], Q[R][R], m[R], P[R][R];
  gs_load_model<R>(pp, A, Q);
  load_vec<R>(pp + L::m0, m);
  load_mat<R, R>(pp + L::S0, P);
  if (row >= B && !sw_same_obs_model<R>(a.params, row, b, a.n))
    flag(a.status, row, EKS_STATUS_BAD_MODEL);
  double nll = 0.0;
  const bool ok = gs_filter_run<R>(a.ws, p, 0, a.T, B, b, A, Q, m, P, nll);
  a.nll[row] = nll;
  if (row < B && a.nobs) a.nobs[row] = pl((const int32_t *)(a.ws + p.cnt_off), 0, B, b);
  if (!ok) flag(a.status, row, EKS_STATUS_SINGULAR);
}

// ===========================================================================
// host launcher
// ===========================================================================
template <int R>
int launch_gs(const GsArgs &a, GsPlan p) {
  const long long KB = a.K * a.B;
  const bool uni = uniform_lanes(a.B), uni_e = uniform_lanes(KB);
  const unsigned g1 = lane_grid(p.NC, a.B), g2 = lane_grid(p.NC, KB);
  const bool wave_scan = p.NC > wave_scan_chunks();
  p.evsrc = yev_ev_planes(a.obs, a.dtype, a.B, a.T, a.n);
  int rc;
  prof_call_begin();
  prof_mark(a.stream, "k_gs_reduce");
  rc = dispatch_input(a.dtype, a.E, [&](auto ttag, auto Ec) -> int {
    using T = decltype(ttag);
    constexpr int EE = decltype(Ec)::value;
    launch_uni(uni, k_gs_reduce<R, T, EE, true>, k_gs_reduce<R, T, EE, false>, g1, a.stream, a, p);
    return check_launch("k_gs_reduce");
  });
  if (rc) return rc;
  if (p.NC == 1) {
    prof_mark(a.stream, "k_gs_seq");
    hipLaunchKernelGGL((k_gs_seq<R>), dim3(grid_for(KB, 64)), dim3(64), 0, a.stream, a, p);
    prof_call_end(a.stream);
    return check_launch("k_gs_seq");
  }
  prof_mark(a.stream, "k_gs_elem");
  launch_uni(uni_e, k_gs_elem<R, true>, k_gs_elem<R, false>, g2, a.stream, a, p);
  if ((rc = check_launch("k_gs_elem"))) return rc;
  prof_mark(a.stream, "k_gs_fscan");
  launch_scan(wave_scan, k_gs_fscan<R>, k_gs_fscan_w<R>, KB, a.stream, a, p);
  if ((rc = check_launch("k_gs_fscan"))) return rc;
  prof_mark(a.stream, "k_gs_share");
  launch_uni(uni_e, k_gs_share<R, true>, k_gs_share<R, false>, g2, a.stream, a, p);
  if ((rc = check_launch("k_gs_share"))) return rc;
  prof_mark(a.stream, "k_gs_sum");
  launch_scan(wave_scan, k_gs_sum, k_gs_sum_w, KB, a.stream, a, p);
  prof_call_end(a.stream);
  return check_launch("k_gs_sum");
}

}  // namespace eks
