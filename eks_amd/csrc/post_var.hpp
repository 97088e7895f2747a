// Posterior variances of the smoother (eks_smooth_var): the covariance
// recursions of eks/ensemble_kalman.py:59-164 alone, time-parallel.
//
// The covariances Vf, S, J, Vs do not depend on the observations y, only on
// the ensemble variances ev[t] and the model, and with R_t = diag(ev[t]) the
// data enter through W_t = C^T R_t^-1 C = sum_j c_j c_j^T / ev[t][j] alone
// (r x r symmetric).  Once W_t is formed nothing depends on n, so one set of
// kernels templated on R serves every n <= kMaxObsRt.
//
//   filter   P-_0 = S0;  P-_t = A P_{t-1} A^T + Q;  P_t = (I + P-_t W_t)^-1 P-_t
//   RTS      S_t = A P_t A^T + Q,  J_t = P_t A^T S_t^-1,  D_t = P_t - J_t S_t J_t^T,
//            Vs_{T-1} = P_{T-1},  Vs_t = J_t Vs_{t+1} J_t^T + D_t
//   output   pvar[t][j] = c_j Vs_t c_j^T
//
// Each trajectory's T steps are cut into NC chunks of L steps; one lane owns
// one (chunk, trajectory) pair (Lane<UNI>, planes as smooth_impl.hpp).  Five
// launches, launch boundaries the only synchronisation (no kernel waits on
// another block):
//
//  V1 k_pv_elem   members (or the ev planes of a y / ev hand-off) -> W_t,
//                 stored as Sym<R> planes so the members are read once; the
//                 chunk's covariance element (A_e, C_e, J_e), the covariance
//                 part of the Sarkka & Garcia-Fernandez filtering element:
//                 P_end = A_e (I + P_in J_e)^-1 P_in A_e^T + C_e
//                 (chunk 0: the plain filter from S0, element (0, P_end, 0))
//  V2 k_pv_fscan  prefix scan of the elements per trajectory: the C of the
//                 prefix up to chunk c-1 is the filtered covariance entering c
//  V3 k_pv_rerun  the Riccati recursion over the chunk from that covariance,
//                 over the W planes: P_t planes, and the chunk's RTS map
//                 Vs_first = G Vs_in G^T + Lam, built left to right
//  V4 k_pv_bscan  suffix scan of the maps: Vs entering every chunk from the right
//  V5 k_pv_final  right to left over the chunk from the P_t planes: Vs_t
//                 (stored if asked) and its projection with the n rows of C
//
// The scans run one lane per trajectory while NC <= wave_scan_chunks(), above
// that one wave per trajectory: each lane folds a contiguous run of
// ceil(NC / 64) chunks, a 64-lane shuffle scan follows, each lane rewrites
// its run.
//
// P_t is stored for every step (2 * Sym<R>::len doubles per step with W_t):
// the simple form; V5 recomputes (J_t, D_t) from P_t with rts_gain's
// expressions, so a singular S_t raises EKS_STATUS_SINGULAR where the
// smoother raises it.
//
// Exact observations (ev[t][j] == 0: one member, or identical members) make
// W_t infinite: the trajectory is flagged EKS_STATUS_SCAN, its W_t is set to
// NaN and with it every value of the trajectory.  A NaN ev propagates the same
// way and is not an error.
#pragma once
#include "host_api.hpp"

namespace eks {

extern long long g_pvar_chunk;  // forced chunk length (EKS_DBG_PVAR_CHUNK), 0: automatic

struct PvArgs {
  const void *obs;
  int dtype;
  long long B, T;
  int E, n;
  long long sb, st, se, sj;
  const double *params;
  double *pvar;
  long long vb, vt, vj;
  double *Vs;
  char *ws;
  int32_t *status;
  hipStream_t stream;
};

// workspace planes (doubles, time-major: B values per plane)
struct PvPlan {
  long long L = 0, NC = 0;
  size_t w_off = 0;     // W_t        T  x Sym<R>::len
  size_t p_off = 0;     // P_t        T  x Sym<R>::len
  size_t elem_off = 0;  // elements   NC x (R*R + 2 Sym<R>::len)
  size_t pin_off = 0;   // P entering a chunk          NC x Sym<R>::len
  size_t map_off = 0;   // (G, Lam)   NC x (R*R + Sym<R>::len)
  size_t vin_off = 0;   // Vs entering a chunk from the right   NC x Sym<R>::len
  size_t total = 0;
  const char *evsrc = nullptr;  // the caller's ev planes (y / ev input)
};

inline int pv_sym_len(int r) { return r * (r + 1) / 2; }

// Chunk length as launched: a multiple of 8; one chunk when it covers T.
// Automatic: the smoother's (call_chunk_len).  With few trajectories
// (chunk-major lanes, B <= 256) the smoother shortens its chunks to kMinChunk
// because its group-mode scans cost the same for any chunk count; the scans
// here are one wave per trajectory, T / (64 L) compositions per lane, so L
// balances them against the per-lane kernels' L steps: L = c sqrt(T), c from
// the measured optima (17 trajectories: T = 100 000, r = 2: L = 48 of 16 .. 128,
// 0.43 -> 0.25 ms; T = 50 000, r = 3, n = 8: L = 32, 0.59 -> 0.55 ms;
// tools/pvar_timing.py --chunk).
inline long long pv_chunk_len(long long B, long long T, int r) {
  return chunk_len_rule(g_pvar_chunk, call_chunk_len(B, T, r, true, 0), 0.15, 0.11, B, T, r);
}

inline PvPlan pv_make_plan(long long B, long long T, int r, long long L) {
  PvPlan p;
  p.L = L;
  p.NC = (T + L - 1) / L;
  const size_t S = (size_t)pv_sym_len(r), RR = (size_t)r * r, Bz = (size_t)B;
  Carver ws;
  auto take = [&](size_t doubles) { return ws.take(doubles * Bz * 8); };
  p.w_off = take((size_t)T * S);
  p.p_off = take((size_t)T * S);
  p.elem_off = take((size_t)p.NC * (RR + 2 * S));
  p.pin_off = take((size_t)p.NC * S);
  p.map_off = take((size_t)p.NC * (RR + S));
  p.vin_off = take((size_t)p.NC * S);
  p.total = ws.off;
  return p;
}

// ---------------------------------------------------------------------------
// small symmetric pieces; every sum an explicit fma chain in ascending k
// ---------------------------------------------------------------------------
template <int R>
EKS_DEV void pv_mirror(double (&M)[R][R]) {
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) M[i][j] = M[j][i];
}

// Z = X M X^T + add, upper triangle computed and mirrored
template <int R>
EKS_DEV void pv_congruence(const double (&X)[R][R], const double (&M)[R][R],
                           const double (&add)[R][R], double (&Z)[R][R]) {
  double XM[R][R];
  matmul<R, R, R>(X, M, XM);
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) {
      double s = add[i][j];
#pragma unroll
      for (int k = 0; k < R; ++k) s = fma(XM[i][k], X[j][k], s);
      Z[i][j] = s;
    }
  pv_mirror<R>(Z);
}

template <int R>
EKS_DEV void pv_load_sym(const double *base, long long plane0, long long B, unsigned b,
                         double (&M)[R][R]) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) M[i][j] = M[j][i] = pl(base, plane0 + (k++), B, b);
}

template <int R>
EKS_DEV void pv_store_sym(double *base, long long plane0, long long B, unsigned b,
                          const double (&M)[R][R]) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) pl(base, plane0 + (k++), B, b) = M[i][j];
}

// N = (I + X Y)^-1; false on an exactly singular I + X Y
template <int R>
EKS_DEV bool pv_inv_ipxy(const double (&X)[R][R], const double (&Y)[R][R], double (&N)[R][R]) {
  double M[R][R];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) {
      double s = (i == j) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) s = fma(X[i][k], Y[k][j], s);
      M[i][j] = s;
    }
  return small_inverse<R>(M, N);
}

// P <- A P A^T + Q (kf_predict's general-A covariance expression)
template <int R>
EKS_DEV void pv_predict(double (&P)[R][R], const double (&A)[R][R], const double (&Q)[R][R]) {
  double PAt[R][R];
  matmul_nt<R, R, R>(P, A, PAt);
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) s = fma(A[i][k], PAt[k][j], s);
      P[i][j] = s + Q[i][j];
    }
  pv_mirror<R>(P);
}

// P <- (I + P W)^-1 P, kept symmetric
template <int R>
EKS_DEV bool pv_update(double (&P)[R][R], const double (&W)[R][R]) {
  double N[R][R], Pn[R][R];
  const bool ok = pv_inv_ipxy<R>(P, W, N);
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) s = fma(N[i][k], P[k][j], s);
      Pn[i][j] = s;
    }
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) P[i][j] = P[j][i] = Pn[i][j];
  return ok;
}

// RTS gain of step t from the filtered P (rts_gain's expressions for a
// general A) and D = P - J S J^T = P - (P A^T) J^T
template <int R>
EKS_DEV bool pv_rts(const double (&P)[R][R], const double (&A)[R][R], const double (&Q)[R][R],
                    double (&J)[R][R], double (&D)[R][R]) {
  double S[R][R], PAt[R][R], Si[R][R];
  matmul_nt<R, R, R>(P, A, PAt);
  matmul<R, R, R>(A, PAt, S);
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) S[i][j] += Q[i][j];
  const bool ok = small_inverse<R>(S, Si);
  matmul<R, R, R>(PAt, Si, J);
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = i; j < R; ++j) {
      double s = P[i][j];
#pragma unroll
      for (int k = 0; k < R; ++k) s = fma(-PAt[i][k], J[j][k], s);
      D[i][j] = s;
    }
  pv_mirror<R>(D);
  return ok;
}

// ---------------------------------------------------------------------------
// The covariance part of the filtering element of a run of steps:
//   P_out = A (I + P_in J)^-1 P_in A^T + C        (C, J symmetric)
// stored as [A (row-major) | C (Sym) | J (Sym)].
// ---------------------------------------------------------------------------
template <int R>
struct CovElem {
  static constexpr int S = Sym<R>::len;
  static constexpr int len = R * R + 2 * S;
  double A[R][R], C[R][R], J[R][R];
  EKS_DEV void set_identity() {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        A[i][j] = (i == j) ? 1.0 : 0.0;
        C[i][j] = 0.0;
        J[i][j] = 0.0;
      }
  }
  // a run that starts the trajectory: P_out = P whatever enters
  EKS_DEV void set_const(const double (&P)[R][R]) {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        A[i][j] = 0.0;
        C[i][j] = P[i][j];
        J[i][j] = 0.0;
      }
  }
  template <typename Get>
  EKS_DEV void load_at(Get &&get) {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) A[i][j] = get(i * R + j);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = i; j < R; ++j) {
        C[i][j] = C[j][i] = get(R * R + Sym<R>::idx(i, j));
        J[i][j] = J[j][i] = get(R * R + S + Sym<R>::idx(i, j));
      }
  }
  template <typename Put>
  EKS_DEV void store_at(Put &&put) const {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) put(i * R + j, A[i][j]);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = i; j < R; ++j) {
        put(R * R + Sym<R>::idx(i, j), C[i][j]);
        put(R * R + S + Sym<R>::idx(i, j), J[i][j]);
      }
  }
  // one step t >= 1 absorbed on the right: predict with (Am, Q), update with W;
  // equal to then() with the step's element ((I + Q W)^-1 Am, (I + Q W)^-1 Q,
  // Am^T W (I + Q W)^-1 Am), one inverse instead of two
  EKS_DEV bool absorb(const double (&Am)[R][R], const double (&Q)[R][R],
                      const double (&W)[R][R]) {
    double Ap[R][R], Cp[R][R], N[R][R], NA[R][R], WNA[R][R], Z[R][R];
    matmul<R, R, R>(Am, A, Ap);
    pv_congruence<R>(Am, C, Q, Cp);
    const bool ok = pv_inv_ipxy<R>(Cp, W, N);
    matmul<R, R, R>(N, Ap, NA);
    matmul<R, R, R>(W, NA, WNA);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = i; j < R; ++j) {
        double s = J[i][j];
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(Ap[k][i], WNA[k][j], s);
        Z[i][j] = s;
      }
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = i; j < R; ++j) {
        J[i][j] = J[j][i] = Z[i][j];
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(N[i][k], Cp[k][j], s);
        C[i][j] = s;
      }
    pv_mirror<R>(C);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) A[i][j] = NA[i][j];
    return ok;
  }
  // this (earlier) followed by o (later), N = (I + C1 J2)^-1:
  //   A = A2 N A1,  C = A2 N C1 A2^T + C2,  J = A1^T N^T J2 A1 + J1
  // ((I + J2 C1)^-1 = N^T as C1, J2 are symmetric)
  EKS_DEV CovElem then(const CovElem &o, bool &ok) const {
    CovElem e;
    double N[R][R], X[R][R], XC[R][R], NtJ[R][R], T1[R][R];
    ok = pv_inv_ipxy<R>(C, o.J, N) && ok;
    matmul<R, R, R>(o.A, N, X);
    matmul<R, R, R>(X, A, e.A);
    matmul<R, R, R>(X, C, XC);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = i; j < R; ++j) {
        double s = o.C[i][j];
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(XC[i][k], o.A[j][k], s);
        e.C[i][j] = s;
      }
    pv_mirror<R>(e.C);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(N[k][i], o.J[k][j], s);
        NtJ[i][j] = s;
      }
    matmul<R, R, R>(NtJ, A, T1);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = i; j < R; ++j) {
        double s = J[i][j];
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(A[k][i], T1[k][j], s);
        e.J[i][j] = s;
      }
    pv_mirror<R>(e.J);
    return e;
  }
  EKS_DEV CovElem shfl_up(int delta) const {
    CovElem o;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        o.A[i][j] = __shfl_up(A[i][j], delta, 64);
        o.C[i][j] = __shfl_up(C[i][j], delta, 64);
        o.J[i][j] = __shfl_up(J[i][j], delta, 64);
      }
    return o;
  }
};

// ---------------------------------------------------------------------------
// The chunk map of the backward pass: Vs_first = G Vs_in G^T + L, stored as
// [G (row-major) | L (Sym)].
// ---------------------------------------------------------------------------
template <int R>
struct CovMap {
  static constexpr int S = Sym<R>::len;
  static constexpr int len = R * R + S;
  double G[R][R], L[R][R];
  EKS_DEV void set_identity() {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        G[i][j] = (i == j) ? 1.0 : 0.0;
        L[i][j] = 0.0;
      }
  }
  template <typename Get>
  EKS_DEV void load_at(Get &&get) {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) G[i][j] = get(i * R + j);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = i; j < R; ++j) L[i][j] = L[j][i] = get(R * R + Sym<R>::idx(i, j));
  }
  template <typename Put>
  EKS_DEV void store_at(Put &&put) const {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) put(i * R + j, G[i][j]);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = i; j < R; ++j) put(R * R + Sym<R>::idx(i, j), L[i][j]);
  }
  // one RTS step absorbed on the right: L += G D G^T, then G <- G J
  EKS_DEV void step(const double (&J)[R][R], const double (&D)[R][R]) {
    double Ln[R][R], GJ[R][R];
    pv_congruence<R>(G, D, L, Ln);
    matmul<R, R, R>(G, J, GJ);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        L[i][j] = Ln[i][j];
        G[i][j] = GJ[i][j];
      }
  }
  // the trajectory's last step, Vs[T-1] = P: the map ends in a constant
  EKS_DEV void step_const(const double (&P)[R][R]) {
    double Ln[R][R];
    pv_congruence<R>(G, P, L, Ln);
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        L[i][j] = Ln[i][j];
        G[i][j] = 0.0;
      }
  }
  // this (earlier steps) o o (later steps): (G1 G2, L1 + G1 L2 G1^T)
  EKS_DEV CovMap then(const CovMap &o) const {
    CovMap m;
    matmul<R, R, R>(G, o.G, m.G);
    pv_congruence<R>(G, o.L, L, m.L);
    return m;
  }
  EKS_DEV CovMap shfl_down(int delta) const {
    CovMap o;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        o.G[i][j] = __shfl_down(G[i][j], delta, 64);
        o.L[i][j] = __shfl_down(L[i][j], delta, 64);
      }
    return o;
  }
};

// ===========================================================================
// V1: W_t planes and the chunk's covariance element
// T: float / double members, or YevIn<.> (the caller's ev planes; E unused)
// ===========================================================================
template <int R, typename T, int E, bool UNI>
__global__ __launch_bounds__(kBlock) void k_pv_elem(PvArgs a, PvPlan p) {
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
  const double *pp = a.params + (long long)b * param_stride<R, 0>(n);
  double A[R][R], Q[R][R];
  load_mat<R, R>(pp + L::A, A);
  load_mat<R, R>(pp + L::Q, Q);
  const double *Cm = pp + L::C;
  const MT *ob = kYev ? nullptr : (const MT *)a.obs + (long long)b * a.sb;
  const double *evp = (const double *)p.evsrc;
  double *wbuf = (double *)(a.ws + p.w_off);
  const long long s = c * p.L, e = min(TT, s + p.L);
  const bool first = c == 0;
  bool ok = true, exact = false;
  CovElem<R> El;
  El.set_identity();
  double P[R][R];
  if (first) load_mat<R, R>(pp + L::S0, P);
  for (long long t = s; t < e; ++t) {
    double W[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int k = 0; k < R; ++k) W[i][k] = 0.0;
    for (int j = 0; j < n; ++j) {
      double var;
      if constexpr (kYev) {
        var = pl(evp, t * n + j, B, b);
      } else {
        double avg;
        column_reduce<E, MT>(ob + t * a.st + j * a.sj, a.se, a.E, false, avg, var);
      }
      exact = exact || (var == 0.0);
      const double inv = 1.0 / var;
      double cr[R];
#pragma unroll
      for (int i = 0; i < R; ++i) cr[i] = Cm[j * R + i];
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int k = i; k < R; ++k) W[i][k] = fma(cr[i] * cr[k], inv, W[i][k]);
    }
    if (exact) {  // an infinite W_t: the trajectory is NaN from here on, both ways
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int k = i; k < R; ++k) W[i][k] = __builtin_nan("");
    }
    pv_mirror<R>(W);
    pv_store_sym<R>(wbuf, t * S, B, b, W);
    if (first) {
      if (t > 0) pv_predict<R>(P, A, Q);
      ok = pv_update<R>(P, W) && ok;
    } else {
      ok = El.absorb(A, Q, W) && ok;
    }
  }
  if (first) El.set_const(P);
  double *eb = (double *)(a.ws + p.elem_off);
  El.store_at([&](int k, double v) { pl(eb, c * CovElem<R>::len + k, B, b) = v; });
  if (exact || !ok) flag(a.status, b, EKS_STATUS_SCAN);
}

// ===========================================================================
// V2: prefix scan of the elements.  One lane per trajectory ...
// ===========================================================================
template <int R>
__global__ __launch_bounds__(64) void k_pv_fscan(PvArgs a, PvPlan p) {
  const long long bl = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (bl >= a.B) return;
  const unsigned b = (unsigned)bl;
  const long long B = a.B;
  constexpr int EL = CovElem<R>::len, S = Sym<R>::len;
  const double *eb = (const double *)(a.ws + p.elem_off);
  double *pin = (double *)(a.ws + p.pin_off);
  bool ok = true;
  CovElem<R> X;
  X.load_at([&](int k) { return pl(eb, (long long)k, B, b); });
  for (long long c = 1; c < p.NC; ++c) {
    pv_store_sym<R>(pin, c * S, B, b, X.C);
    if (c + 1 == p.NC) break;
    CovElem<R> e;
    e.load_at([&](int k) { return pl(eb, c * EL + k, B, b); });
    X = X.then(e, ok);
  }
  if (!ok) flag(a.status, b, EKS_STATUS_SCAN);
}

// ... or one wave per trajectory: lane l folds chunks [l q, (l+1) q), a
// 64-lane shuffle scan gives the prefix before its run, and it rewrites the run
template <int R>
__global__ __launch_bounds__(64) void k_pv_fscan_w(PvArgs a, PvPlan p) {
  const unsigned b = blockIdx.x;
  const int lane = threadIdx.x;
  const long long B = a.B, NC = p.NC;
  constexpr int EL = CovElem<R>::len, S = Sym<R>::len;
  const double *eb = (const double *)(a.ws + p.elem_off);
  double *pin = (double *)(a.ws + p.pin_off);
  const long long q = (NC + 63) / 64;
  const long long c0 = min(NC, lane * q), c1 = min(NC, c0 + q);
  bool ok = true;
  CovElem<R> F;
  F.set_identity();
  for (long long c = c0; c < c1; ++c) {
    CovElem<R> e;
    e.load_at([&](int k) { return pl(eb, c * EL + k, B, b); });
    F = F.then(e, ok);
  }
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const CovElem<R> o = F.shfl_up(k);
    bool ok2 = true;
    const CovElem<R> m = o.then(F, ok2);
    if (lane >= k) {
      F = m;
      ok = ok && ok2;
    }
  }
  CovElem<R> X = F.shfl_up(1);
  if (lane == 0) X.set_identity();
  for (long long c = c0; c < c1; ++c) {
    if (c > 0) pv_store_sym<R>(pin, c * S, B, b, X.C);
    CovElem<R> e;
    e.load_at([&](int k) { return pl(eb, c * EL + k, B, b); });
    X = X.then(e, ok);
  }
  if (!ok) flag(a.status, b, EKS_STATUS_SCAN);
}

// ===========================================================================
// V3: the Riccati recursion over the chunk from its entering covariance:
// P_t planes and the chunk's RTS map
// ===========================================================================
template <int R, bool UNI>
__global__ __launch_bounds__(kBlock) void k_pv_rerun(PvArgs a, PvPlan p) {
  Lane<UNI> ln;
  if (!ln.init(a.B, p.NC)) return;
  const long long c = ln.c;
  const unsigned b = ln.b;
  const long long B = a.B, TT = a.T;
  constexpr int S = Sym<R>::len;
  using L = ParamLayout<R, 0>;
  const double *pp = a.params + (long long)b * param_stride<R, 0>(a.n);
  double A[R][R], Q[R][R], P[R][R];
  load_mat<R, R>(pp + L::A, A);
  load_mat<R, R>(pp + L::Q, Q);
  if (c == 0)
    load_mat<R, R>(pp + L::S0, P);
  else
    pv_load_sym<R>((const double *)(a.ws + p.pin_off), c * S, B, b, P);
  const double *wbuf = (const double *)(a.ws + p.w_off);
  double *pbuf = (double *)(a.ws + p.p_off);
  CovMap<R> F;
  F.set_identity();
  const long long s = c * p.L, e = min(TT, s + p.L);
  bool ok = true;
  for (long long t = s; t < e; ++t) {
    double W[R][R];
    pv_load_sym<R>(wbuf, t * S, B, b, W);
    if (t > 0) pv_predict<R>(P, A, Q);
    ok = pv_update<R>(P, W) && ok;
    pv_store_sym<R>(pbuf, t * S, B, b, P);
    if (t + 1 < TT) {
      double J[R][R], D[R][R];
      ok = pv_rts<R>(P, A, Q, J, D) && ok;
      F.step(J, D);
    } else {
      F.step_const(P);
    }
  }
  double *mb = (double *)(a.ws + p.map_off);
  F.store_at([&](int k, double v) { pl(mb, c * CovMap<R>::len + k, B, b) = v; });
  if (!ok) flag(a.status, b, EKS_STATUS_SINGULAR);
}

// ===========================================================================
// V4: suffix scan of the maps.  The suffix from chunk c+1 on ends in the
// trajectory's last step, a constant map (G = 0), so its L is the Vs
// entering chunk c from the right.
// ===========================================================================
template <int R>
__global__ __launch_bounds__(64) void k_pv_bscan(PvArgs a, PvPlan p) {
  const long long bl = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (bl >= a.B) return;
  const unsigned b = (unsigned)bl;
  const long long B = a.B;
  constexpr int ML = CovMap<R>::len, S = Sym<R>::len;
  const double *mb = (const double *)(a.ws + p.map_off);
  double *vin = (double *)(a.ws + p.vin_off);
  CovMap<R> X;
  X.load_at([&](int k) { return pl(mb, (p.NC - 1) * ML + k, B, b); });
  for (long long c = p.NC - 2; c >= 0; --c) {
    pv_store_sym<R>(vin, c * S, B, b, X.L);
    if (c == 0) break;
    CovMap<R> m;
    m.load_at([&](int k) { return pl(mb, c * ML + k, B, b); });
    X = m.then(X);
  }
}

template <int R>
__global__ __launch_bounds__(64) void k_pv_bscan_w(PvArgs a, PvPlan p) {
  const unsigned b = blockIdx.x;
  const int lane = threadIdx.x;
  const long long B = a.B, NC = p.NC;
  constexpr int ML = CovMap<R>::len, S = Sym<R>::len;
  const double *mb = (const double *)(a.ws + p.map_off);
  double *vin = (double *)(a.ws + p.vin_off);
  const long long q = (NC + 63) / 64;
  const long long c0 = min(NC, lane * q), c1 = min(NC, c0 + q);
  CovMap<R> F;
  F.set_identity();
  for (long long c = c0; c < c1; ++c) {
    CovMap<R> m;
    m.load_at([&](int k) { return pl(mb, c * ML + k, B, b); });
    F = F.then(m);
  }
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const CovMap<R> o = F.shfl_down(k);
    const CovMap<R> m = F.then(o);
    if (lane + k < 64) F = m;
  }
  CovMap<R> X = F.shfl_down(1);
  if (lane == 63) X.set_identity();
  for (long long c = c1 - 1; c >= c0; --c) {
    if (c + 1 < NC) pv_store_sym<R>(vin, c * S, B, b, X.L);
    CovMap<R> m;
    m.load_at([&](int k) { return pl(mb, c * ML + k, B, b); });
    X = m.then(X);
  }
}

// ===========================================================================
// V5: right to left over the chunk: Vs_t and pvar[t][j] = c_j Vs_t c_j^T
// ===========================================================================
template <int R, bool UNI>
__global__ __launch_bounds__(kBlock) void k_pv_final(PvArgs a, PvPlan p) {
  Lane<UNI> ln;
  if (!ln.init(a.B, p.NC)) return;
  const long long c = ln.c;
  const unsigned b = ln.b;
  const long long B = a.B, TT = a.T;
  const int n = a.n;
  constexpr int S = Sym<R>::len;
  using L = ParamLayout<R, 0>;
  const double *pp = a.params + (long long)b * param_stride<R, 0>(n);
  double A[R][R], Q[R][R], V[R][R];
  load_mat<R, R>(pp + L::A, A);
  load_mat<R, R>(pp + L::Q, Q);
  const double *Cm = pp + L::C;
  // C = I (r = n): the projection is the diagonal of Vs
  bool c_id = n == R;
  if (c_id) {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int k = 0; k < R; ++k) c_id = c_id && (Cm[i * R + k] == (i == k ? 1.0 : 0.0));
  }
  const double *pbuf = (const double *)(a.ws + p.p_off);
  const long long s = c * p.L, e = min(TT, s + p.L);
  if (e < TT) {
    pv_load_sym<R>((const double *)(a.ws + p.vin_off), c * S, B, b, V);
  } else {
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int k = 0; k < R; ++k) V[i][k] = 0.0;
  }
  double *vo = a.pvar + (long long)b * a.vb;
  bool ok = true;
  for (long long t = e - 1; t >= s; --t) {
    double P[R][R];
    pv_load_sym<R>(pbuf, t * S, B, b, P);
    if (t + 1 < TT) {
      double J[R][R], D[R][R], Vn[R][R];
      ok = pv_rts<R>(P, A, Q, J, D) && ok;
      pv_congruence<R>(J, V, D, Vn);
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int k = 0; k < R; ++k) V[i][k] = Vn[i][k];
    } else {
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int k = 0; k < R; ++k) V[i][k] = P[i][k];
    }
    if (a.Vs) store_mat<R, R>(a.Vs + ((long long)b * TT + t) * (R * R), V);
    double *o = vo + t * a.vt;
    if (c_id) {
#pragma unroll
      for (int i = 0; i < R; ++i) o[i * a.vj] = V[i][i];
    } else {
      for (int j = 0; j < n; ++j) {
        double cr[R];
#pragma unroll
        for (int i = 0; i < R; ++i) cr[i] = Cm[j * R + i];
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
          double vc = 0.0;
#pragma unroll
          for (int k = 0; k < R; ++k) vc = fma(V[i][k], cr[k], vc);
          acc = fma(cr[i], vc, acc);
        }
        o[j * a.vj] = acc;
      }
    }
  }
  // (V3 has flagged a singular S_t already; the same expressions ran here)
  (void)ok;
}

// ===========================================================================
// host launcher
// ===========================================================================
template <int R>
int launch_pv(const PvArgs &a, PvPlan p) {
  const bool uni = uniform_lanes(a.B);
  const unsigned gch = lane_grid(p.NC, a.B);
  const bool wave_scan = p.NC > wave_scan_chunks();
  p.evsrc = yev_ev_planes(a.obs, a.dtype, a.B, a.T, a.n);
  int rc;
  prof_call_begin();
  prof_mark(a.stream, "k_pv_elem");
  // (a hand-off: only the ev planes are read)
  rc = dispatch_input<false>(a.dtype, a.E, [&](auto ttag, auto Ec) -> int {
    using T = decltype(ttag);
    constexpr int EE = decltype(Ec)::value;
    launch_uni(uni, k_pv_elem<R, T, EE, true>, k_pv_elem<R, T, EE, false>, gch, a.stream, a, p);
    return check_launch("k_pv_elem");
  });
  if (rc) return rc;
  if (p.NC > 1) {
    prof_mark(a.stream, "k_pv_fscan");
    launch_scan(wave_scan, k_pv_fscan<R>, k_pv_fscan_w<R>, a.B, a.stream, a, p);
    if ((rc = check_launch("k_pv_fscan"))) return rc;
  }
  prof_mark(a.stream, "k_pv_rerun");
  launch_uni(uni, k_pv_rerun<R, true>, k_pv_rerun<R, false>, gch, a.stream, a, p);
  if ((rc = check_launch("k_pv_rerun"))) return rc;
  if (p.NC > 1) {
    prof_mark(a.stream, "k_pv_bscan");
    launch_scan(wave_scan, k_pv_bscan<R>, k_pv_bscan_w<R>, a.B, a.stream, a, p);
    if ((rc = check_launch("k_pv_bscan"))) return rc;
  }
  prof_mark(a.stream, "k_pv_final");
  launch_uni(uni, k_pv_final<R, true>, k_pv_final<R, false>, gch, a.stream, a, p);
  prof_call_end(a.stream);
  return check_launch("k_pv_final");
}

}  // namespace eks
