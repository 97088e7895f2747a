// eks_ensemble_gaps: the ensemble over the VALID (finite) members of every
// column, written as the y / ev hand-off planes eks_smooth_gaps,
// eks_nll_sweep_gaps and eks_fit_gaps read (EKS_YEV64: y and ev float64,
// time-major [t*n + j][b]).  A column is missing (y = ev = NaN) only when
// fewer than min_members of its E members are finite; the arithmetic is
// ensemble_reduce_valid's (ensemble.hpp).
//
// A streaming kernel: E n sizeof(T) bytes read and 16 n (+ n with nvalid)
// written per frame.  k_fit_worst's lanes: one lane per (trajectory, chunk of
// frames), trajectory fastest, so every plane store of a wave is one
// contiguous row segment.  n is a runtime loop (up to 64), so the lane's
// frames are flattened into one stream of columns q = (t - t0) n + j -- the
// plane index (t0 n + q) B + b is linear in q -- with the member loads of the
// next DP columns in a register ring (compiled E = 3, 4, 5, and 8: the
// runtime reduction's sums contract differently from ensemble_reduce<8>'s,
// which eks_ensemble runs, by an ulp of the variance in a few columns per
// 10^4, and complete columns must have its bits); any other E reduces
// straight from memory.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/eks_hip.h"
#include "eks_common.hpp"
#include "ensemble.hpp"

namespace eks {

namespace {

// columns of member loads in flight per lane: 8 columns of up to 32 bytes,
// else 4 (160 bytes at E = 5 float32, as k_fit_worst's ring)
template <int E, typename T>
constexpr int ens_depth() {
  return E * (int)sizeof(T) <= 32 ? 8 : 4;
}

struct EnsShape {
  long long B, T;
  long long NC;  // chunks per trajectory
  long long Lc;  // frames per chunk
};

template <int E, typename T>
__global__ __launch_bounds__(256) void k_ens_gaps(const T *__restrict__ obs, EnsShape sh, int n,
                                                  long long sb, long long st, long long se,
                                                  long long sj, int Ert, int median,
                                                  int min_members, double *__restrict__ y,
                                                  double *__restrict__ ev,
                                                  uint8_t *__restrict__ nvalid) {
  const long long lane = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (lane >= sh.B * sh.NC) return;
  const long long b = lane % sh.B;
  const long long t0 = (lane / sh.B) * sh.Lc;
  const long long t1 = t0 + sh.Lc < sh.T ? t0 + sh.Lc : sh.T;
  if (t0 >= t1) return;
  const T *pb = obs + b * sb;
  const long long Q = (t1 - t0) * n;      // the lane's columns
  long long o = t0 * n * sh.B + b;         // plane index of column q = 0; + B per column
  auto put = [&](double avg, double var, int m) {
    y[o] = avg;
    ev[o] = var;
    if (nvalid) nvalid[o] = (uint8_t)m;
    o += sh.B;
  };
  long long q = 0;
  if constexpr (E > 0) {
    constexpr int DP = ens_depth<E, T>();
    T ring[DP][E];
    long long tf = t0;  // next column to fetch: (tf, jf), clamped to the lane's last one
    int jf = 0;
    auto fetch_next = [&](int k) {
      const T *pc = pb + tf * st + jf * sj;
#pragma unroll
      for (int u = 0; u < E; ++u) ring[k][u] = pc[u * se];
      if (++jf == n) {
        jf = 0;
        ++tf;
      }
      if (tf >= t1) {  // past the end: re-read the last column (a cache hit)
        tf = t1 - 1;
        jf = n - 1;
      }
    };
#pragma unroll
    for (int k = 0; k < DP; ++k) fetch_next(k);
    // whole blocks of DP columns as straight-line code
    for (; q + DP <= Q; q += DP) {
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        T cur[E];
#pragma unroll
        for (int u = 0; u < E; ++u) cur[u] = ring[k][u];
        fetch_next(k);
        double avg, var;
        int m;
        ensemble_reduce_valid<E, T>(cur, median != 0, min_members, avg, var, m);
        put(avg, var, m);
      }
    }
  }
  // the last columns (fewer than DP), and every column of a runtime E
  if (q < Q) {
    long long t = t0 + q / n;
    int j = (int)(q % n);
    for (; q < Q; ++q) {
      const T *pc = pb + t * st + j * sj;
      double avg, var;
      int m;
      if constexpr (E > 0) {
        T cur[E];
#pragma unroll
        for (int u = 0; u < E; ++u) cur[u] = pc[u * se];
        ensemble_reduce_valid<E, T>(cur, median != 0, min_members, avg, var, m);
      } else {
        ensemble_reduce_valid_rt<T>(pc, se, Ert, median != 0, min_members, avg, var, m);
      }
      put(avg, var, m);
      if (++j == n) {
        j = 0;
        ++t;
      }
    }
  }
}

// chunks per trajectory: enough lanes to fill the chip (~256k), whole frames
void ens_chunks(long long B, long long T, long long &nc, long long &lc) {
  long long nn = (262144 + B - 1) / B;
  if (nn > T) nn = T;
  if (nn < 1) nn = 1;
  lc = (T + nn - 1) / nn;
  nc = (T + lc - 1) / lc;
}

}  // namespace

}  // namespace eks

using namespace eks;

extern "C" int eks_ensemble_gaps(const void *obs, int obs_dtype, int64_t B, int64_t T, int E,
                                 int n, int64_t sb, int64_t st, int64_t se, int64_t sj, int mode,
                                 int min_members, void *yev, uint8_t *nvalid, void *stream) {
  clear_err();
  if (!obs || !yev) return set_err(EKS_ERR_ARG, "eks_ensemble_gaps: NULL pointer");
  if (B < 0 || T < 1 || E < 1) return set_err(EKS_ERR_ARG, "eks_ensemble_gaps: bad sizes");
  if (n < 1 || n > kMaxObsRt)
    return set_err(EKS_ERR_UNSUPPORTED, "eks_ensemble_gaps: n=%d not supported (1..%d)", n,
                   kMaxObsRt);
  if (E > kMaxMembers)
    return set_err(EKS_ERR_UNSUPPORTED, "eks_ensemble_gaps: E=%d > %d", E, kMaxMembers);
  if (obs_dtype != EKS_F32 && obs_dtype != EKS_F64)
    return set_err(EKS_ERR_ARG, "eks_ensemble_gaps: bad dtype %d (EKS_F32 / EKS_F64)", obs_dtype);
  if (mode != EKS_MEDIAN && mode != EKS_MEAN)
    return set_err(EKS_ERR_ARG, "eks_ensemble_gaps: %d averaging not supported", mode);
  if (min_members < 1 || min_members > E)
    return set_err(EKS_ERR_ARG, "eks_ensemble_gaps: min_members=%d outside 1..E=%d", min_members,
                   E);
  if (B == 0) return EKS_OK;
  hipStream_t s = (hipStream_t)stream;
  EnsShape sh{B, T, 0, 0};
  ens_chunks(B, T, sh.NC, sh.Lc);
  double *y = (double *)yev;
  double *ev = (double *)((char *)yev + yev_ev_offset(B, T, n, sizeof(double)));
  const unsigned grid = grid_for(B * sh.NC, 256);
  auto launch = [&](auto Ec, auto tag) -> int {
    using Tp = decltype(tag);
    constexpr int EE = decltype(Ec)::value;
    prof_call_begin();
    prof_mark(s, "k_ens_gaps");
    hipLaunchKernelGGL((k_ens_gaps<EE, Tp>), dim3(grid), dim3(256), 0, s, (const Tp *)obs, sh, n,
                       sb, st, se, sj, E, mode == EKS_MEDIAN ? 1 : 0, min_members, y, ev, nvalid);
    prof_call_end(s);
    return check_launch("k_ens_gaps");
  };
  auto by_e = [&](auto tag) -> int {
    switch (E) {
      case 3: return launch(ic<3>{}, tag);
      case 4: return launch(ic<4>{}, tag);
      case 5: return launch(ic<5>{}, tag);
      case 8: return launch(ic<8>{}, tag);
      default: return launch(ic<0>{}, tag);
    }
  };
  return obs_dtype == EKS_F32 ? by_e(float{}) : by_e(double{});
}
