// eks_fit_pupil: the statistics of the pupil model (eks/pupil_smoother.py:
// 109-172, fit.pupil_model) on the device: per trajectory the mean and the
// population variance of the pupil diameter and of the two coordinates of its
// centre, over the COMPLETE frames -- eks_fit_gaps's rule: the ensemble
// average and variance of all 8 columns are finite.  From members a column is
// missing under the all-members rule (ensemble_reduce_valid with min_members
// = E, the arithmetic and bits of eks_ensemble_gaps(min_members = E)); any
// other rule comes in through hand-off planes (EKS_YEV32 / EKS_YEV64 input).
// Only complete frames enter the statistics: the reference's nanmedian rescue
// of partly observed frames is deliberately not reproduced, which is the
// wrapper's host path under allow_missing=True, fit.pupil_model(preds[ok], A).
//
// Per complete frame: the diameter is the median of the six estimates of
// fit.pupil_diameter (the mean of the 3rd and 4th in sorted order), the centre
// the mean of the two pair midpoints per coordinate (fit.pupil_centre on
// finite inputs).
//
// Reduction (no floating-point atomics, bit-identical from run to run): a
// lane sums its frames as shifted sums S1 = sum(v - K), S2 = sum((v - K)^2)
// with K its first complete frame (k_fit_accum's idiom: no division per
// frame) and converts them to (count, mean, M2); partials are merged with
// Chan's formula in a fixed tree -- wave shuffle, then the block's waves in
// order (frames across a wave), then k_pupil_final over the partials in the
// workspace.  An empty partial is (0, 0, 0) and merges as the identity.
// The lane mappings and where the switch comes from: pupil_fit.hpp.
//
// With yev the ensemble planes are written on the way (EKS_YEV64, the layout
// and helpers of eks_ensemble_gaps.hip), so fit + sweep + smooth read the
// members once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/eks_hip.h"
#include "eks_common.hpp"
#include "ensemble.hpp"
#include "pupil_fit.hpp"

namespace eks {

namespace {

struct PStat {
  double n;      // complete frames
  double m[3];   // means of (diameter, com_x, com_y)
  double M2[3];  // sums of squared deviations from the means
};

EKS_DEV PStat pstat_empty() { return PStat{0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}; }

// Chan's pairwise merge, a before b.  With the empty partial (0, 0, 0) on
// either side the other comes back bit for bit: w is 0 or 1 and the
// cross term is multiplied by a zero count.
EKS_DEV PStat pstat_merge(const PStat &a, const PStat &b) {
  PStat r;
  r.n = a.n + b.n;
  const double w = r.n > 0.0 ? b.n / r.n : 0.0;
  const double c = a.n * w;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double d = b.m[k] - a.m[k];
    r.m[k] = a.m[k] + d * w;
    r.M2[k] = a.M2[k] + b.M2[k] + d * d * c;
  }
  return r;
}

EKS_DEV PStat pstat_shfl_down(const PStat &s, int o) {
  PStat r;
  r.n = __shfl_down(s.n, o, 64);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.m[k] = __shfl_down(s.m[k], o, 64);
    r.M2[k] = __shfl_down(s.M2[k], o, 64);
  }
  return r;
}

// lane 0 of the wave: the merge of its 64 lanes in a fixed tree
EKS_DEV PStat pstat_wave(PStat s) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s = pstat_merge(s, pstat_shfl_down(s, o));
  return s;
}

EKS_DEV bool finite64(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// (diameter, com_x, com_y) of one frame; columns in fit.PUPIL_KEYS order:
// top (0, 1), bottom (2, 3), right (4, 5), left (6, 7)
EKS_DEV void pupil_frame(const double (&y)[kPupilN], double (&v)[3]) {
  // np.linalg.norm's sqrt(dx dx + dy dy) with both products rounded (no fused
  // multiply-add): a trajectory with one complete frame reports that frame's
  // numpy diameter bit for bit
  auto dist = [](double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    return sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
  };
  constexpr double kRoot2 = 1.4142135623730951;  // 2 ** 0.5
  double e[6] = {dist(y[0], y[1], y[2], y[3]),
                 dist(y[6], y[7], y[4], y[5]),
                 dist(y[0], y[1], y[6], y[7]) * kRoot2,
                 dist(y[0], y[1], y[4], y[5]) * kRoot2,
                 dist(y[2], y[3], y[6], y[7]) * kRoot2,
                 dist(y[2], y[3], y[4], y[5]) * kRoot2};
  sort_net<6, double>(e);
  v[0] = (e[2] + e[3]) / 2.0;
  v[1] = ((y[0] + y[2]) / 2.0 + (y[4] + y[6]) / 2.0) / 2.0;
  v[2] = ((y[1] + y[3]) / 2.0 + (y[5] + y[7]) / 2.0) / 2.0;
}

struct PupilShape {
  long long B, T;
  long long seg;  // frames per partial
  long long NP;   // partials per trajectory
};

// ---------------------------------------------------------------------------
// Frame sources: fetch(ring, b, t) starts the loads of frame t, reduce(ring,
// b, t, y) turns the fetched frame into the 8 ensemble averages and says
// whether the frame is complete.  The accumulation fetches the lane's next
// frame before it reduces the current one.
// ---------------------------------------------------------------------------

// Members.  PACKED: a frame is E * 8 consecutive, 16-byte aligned values
// (sj = 1, se = 8: the time-major layout at B = 1, or (B, T, E, n)
// contiguous), read as 16-byte loads.  E = 0: a runtime member count, reduced
// straight from memory (no ring).
template <int E, typename T, bool PACKED>
struct MemberSrc {
  const T *obs;
  long long sb, st, se, sj;
  int Ert, median;
  double *y, *ev;  // the planes to write, or null
  long long B;
  int row1;  // B = 1 and 16-byte aligned planes: a frame's 8 values are one 64-byte row

  // one frame ahead in registers while it fits ~64 VGPRs
  static constexpr bool kRing = E > 0 && E * kPupilN * (int)sizeof(T) <= 256;
  struct Ring {
    T v[kRing ? kPupilN : 1][kRing ? E : 1];
  };

  template <typename R>
  EKS_DEV void load_frame(R &dst, long long b, long long t) const {
    if constexpr (E > 0) {
      if constexpr (PACKED) {
        const T *p = (const T *)__builtin_assume_aligned(obs + b * sb + t * st, 16);
#pragma unroll
        for (int e = 0; e < E; ++e)
#pragma unroll
          for (int j = 0; j < kPupilN; ++j) dst[j][e] = p[e * kPupilN + j];
      } else {
        const T *p = obs + b * sb + t * st;
#pragma unroll
        for (int j = 0; j < kPupilN; ++j)
#pragma unroll
          for (int e = 0; e < E; ++e) dst[j][e] = p[j * sj + e * se];
      }
    }
  }

  EKS_DEV void fetch(Ring &ring, long long b, long long t) const {
    if constexpr (kRing) load_frame(ring.v, b, t);
  }

  // consumes the ring (the caller fetches the next frame after `taken`)
  template <typename Next>
  EKS_DEV bool reduce(Ring &ring, long long b, long long t, double (&yy)[kPupilN],
                      Next &&fetch_next) const {
    constexpr int RE = E > 0 ? E : 1;
    T cur[kPupilN][RE];
    if constexpr (kRing) {
#pragma unroll
      for (int j = 0; j < kPupilN; ++j)
#pragma unroll
        for (int e = 0; e < RE; ++e) cur[j][e] = ring.v[j][e];
    } else {
      load_frame(cur, b, t);
    }
    fetch_next();
    double vv[kPupilN];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kPupilN; ++j) {
      int m;
      if constexpr (E > 0)
        ensemble_reduce_valid<E, T>(cur[j], median != 0, E, yy[j], vv[j], m);
      else
        ensemble_reduce_valid_rt<T>(obs + b * sb + t * st + j * sj, se, Ert, median != 0, Ert,
                                    yy[j], vv[j], m);
      ok = ok && finite64(yy[j]) && finite64(vv[j]);
    }
    if (y) {
      if (row1) {
        double *py = (double *)__builtin_assume_aligned(y + t * kPupilN, 16);
        double *pe = (double *)__builtin_assume_aligned(ev + t * kPupilN, 16);
#pragma unroll
        for (int j = 0; j < kPupilN; ++j) {
          py[j] = yy[j];
          pe[j] = vv[j];
        }
      } else {
        const long long o = t * kPupilN * B + b;
#pragma unroll
        for (int j = 0; j < kPupilN; ++j) {
          y[o + j * B] = yy[j];
          ev[o + j * B] = vv[j];
        }
      }
    }
    return ok;
  }
};

// Hand-off planes [t * 8 + j][b]: y of type YT, ev float64
template <typename YT>
struct PlaneSrc {
  const YT *y;
  const double *ev;
  long long B;
  struct Ring {
    YT y[kPupilN];
    double ev[kPupilN];
  };
  EKS_DEV void fetch(Ring &ring, long long b, long long t) const {
    const long long o = t * kPupilN * B + b;
#pragma unroll
    for (int j = 0; j < kPupilN; ++j) {
      ring.y[j] = y[o + j * B];
      ring.ev[j] = ev[o + j * B];
    }
  }
  template <typename Next>
  EKS_DEV bool reduce(Ring &ring, long long, long long, double (&yy)[kPupilN],
                      Next &&fetch_next) const {
    double vv[kPupilN];
#pragma unroll
    for (int j = 0; j < kPupilN; ++j) {
      yy[j] = (double)ring.y[j];
      vv[j] = ring.ev[j];
    }
    fetch_next();
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kPupilN; ++j) ok = ok && finite64(yy[j]) && finite64(vv[j]);
    return ok;
  }
};

// the frames t0, t0 + step, ... < tend of trajectory b as one partial
template <class Src>
EKS_DEV PStat lane_accumulate(const Src &src, long long b, long long t0, long long step,
                              long long tend) {
  double K[3] = {0.0, 0.0, 0.0}, S1[3] = {0.0, 0.0, 0.0}, S2[3] = {0.0, 0.0, 0.0};
  double cnt = 0.0;
  typename Src::Ring ring;
  if (t0 < tend) src.fetch(ring, b, t0);
  for (long long t = t0; t < tend; t += step) {
    double y[kPupilN];
    const bool ok = src.reduce(ring, b, t, y, [&] {
      if (t + step < tend) src.fetch(ring, b, t + step);
    });
    if (ok) {
      double v[3];
      pupil_frame(y, v);
      const bool first = cnt == 0.0;
      cnt += 1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        K[k] = first ? v[k] : K[k];  // the shift: the lane's first complete frame
        const double d = v[k] - K[k];
        S1[k] += d;
        S2[k] += d * d;
      }
    }
  }
  PStat s = pstat_empty();
  if (cnt > 0.0) {
    s.n = cnt;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s.m[k] = K[k] + S1[k] / cnt;
      const double m2 = S2[k] - S1[k] * S1[k] / cnt;
      s.M2[k] = m2 > 0.0 ? m2 : 0.0;
    }
  }
  return s;
}

// partials: [(p * kPupilPartW + k) * B + b]
EKS_DEV void part_store(double *part, const PupilShape &sh, long long p, long long b,
                        const PStat &s) {
  double *q = part + p * kPupilPartW * sh.B + b;
  q[0] = s.n;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    q[(1 + k) * sh.B] = s.m[k];
    q[(4 + k) * sh.B] = s.M2[k];
  }
}

EKS_DEV PStat part_load(const double *part, long long B, long long p, long long b) {
  const double *q = part + p * kPupilPartW * B + b;
  PStat s;
  s.n = q[0];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s.m[k] = q[(1 + k) * B];
    s.M2[k] = q[(4 + k) * B];
  }
  return s;
}

// FRAMES = false: trajectory-fastest lanes, one partial per lane.
// FRAMES = true: block (segment p = blockIdx.x, trajectory blockIdx.y),
// consecutive frames across the threads, one partial per block.
template <bool FRAMES, class Src>
__global__ __launch_bounds__(kPupilBlk) void k_pupil_accum(Src src, PupilShape sh,
                                                           double *__restrict__ part) {
  if constexpr (!FRAMES) {
    const long long lane = blockIdx.x * (long long)kPupilBlk + threadIdx.x;
    if (lane >= sh.B * sh.NP) return;
    const long long b = lane % sh.B, p = lane / sh.B;
    const long long t0 = p * sh.seg;
    const long long t1 = t0 + sh.seg < sh.T ? t0 + sh.seg : sh.T;
    part_store(part, sh, p, b, lane_accumulate(src, b, t0, 1, t1));
  } else {
    __shared__ PStat wave_part[kPupilBlk / 64];
    const long long b = blockIdx.y, p = blockIdx.x;
    const long long s0 = p * sh.seg;
    const long long t1 = s0 + sh.seg < sh.T ? s0 + sh.seg : sh.T;
    const PStat s = pstat_wave(lane_accumulate(src, b, s0 + threadIdx.x, kPupilBlk, t1));
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      PStat a = wave_part[0];
#pragma unroll
      for (int w = 1; w < kPupilBlk / 64; ++w) a = pstat_merge(a, wave_part[w]);
      part_store(part, sh, p, b, a);
    }
  }
}

// one wave per trajectory: lane l merges the partials l, l + 64, ... in
// order, then the wave's tree
__global__ __launch_bounds__(64) void k_pupil_final(const double *__restrict__ part, long long B,
                                                    long long NP, double *__restrict__ stats,
                                                    int32_t *__restrict__ ncomplete,
                                                    int32_t *__restrict__ status) {
  const long long b = blockIdx.x;
  PStat s = pstat_empty();
  for (long long p = threadIdx.x; p < NP; p += 64) s = pstat_merge(s, part_load(part, B, p, b));
  s = pstat_wave(s);
  if (threadIdx.x != 0) return;
  double *o = stats + b * 6;
  ncomplete[b] = (int32_t)s.n;
  if (s.n > 0.0) {
    status[b] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      o[k] = s.m[k];
      o[3 + k] = s.M2[k] / s.n;
    }
  } else {
    status[b] = EKS_STATUS_SINGULAR;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = __builtin_nan("");
  }
}

template <bool FRAMES, class Src>
int launch_accum(const Src &src, const PupilPlan &pl, double *part, hipStream_t s) {
  const PupilShape sh{pl.B, pl.T, pl.seg, pl.NP};
  prof_mark(s, "k_pupil_accum");
  hipLaunchKernelGGL((k_pupil_accum<FRAMES, Src>), dim3((unsigned)pl.gx, (unsigned)pl.gy),
                     dim3(kPupilBlk), 0, s, src, sh, part);
  return check_launch("k_pupil_accum");
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

}  // namespace eks

using namespace eks;

extern "C" size_t eks_fit_pupil_workspace_bytes(int64_t B, int64_t T) {
  const PupilPlan pl = pupil_plan(B, T);
  return pl.ok ? pl.part_bytes : 0;
}

extern "C" int eks_fit_pupil(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n,
                             int64_t sb, int64_t st, int64_t se, int64_t sj, int mode,
                             double *stats, int32_t *ncomplete, void *workspace,
                             size_t workspace_bytes, int32_t *status, void *yev, void *stream) {
  clear_err();
  if (!obs || !stats || !ncomplete || !workspace || !status)
    return set_err(EKS_ERR_ARG, "eks_fit_pupil: NULL pointer");
  const bool planes = obs_dtype == EKS_YEV32 || obs_dtype == EKS_YEV64;
  if (!planes && obs_dtype != EKS_F32 && obs_dtype != EKS_F64)
    return set_err(EKS_ERR_ARG,
                   "eks_fit_pupil: bad dtype %d (EKS_F32 / EKS_F64 / EKS_YEV32 / EKS_YEV64)",
                   obs_dtype);
  if (planes) {
    if (yev)
      return set_err(EKS_ERR_ARG,
                     "eks_fit_pupil: with hand-off planes as input yev must be NULL");
    E = 1;  // (ignored, as the strides and mode)
    mode = EKS_MEDIAN;
  }
  if (n != kPupilN)
    return set_err(EKS_ERR_UNSUPPORTED, "eks_fit_pupil: n=%d not supported (the pupil model has %d)",
                   n, kPupilN);
  if (B < 0 || T < 2 || E < 1) return set_err(EKS_ERR_ARG, "eks_fit_pupil: bad sizes");
  if (E > kMaxMembers)
    return set_err(EKS_ERR_UNSUPPORTED, "eks_fit_pupil: E=%d > %d", E, kMaxMembers);
  if (mode != EKS_MEDIAN && mode != EKS_MEAN)
    return set_err(EKS_ERR_ARG, "eks_fit_pupil: %d averaging not supported", mode);
  if (B == 0) return EKS_OK;
  const PupilPlan pl = pupil_plan(B, T);
  if (!pl.ok)
    return set_err(EKS_ERR_UNSUPPORTED, "eks_fit_pupil: B=%lld T=%lld is beyond one launch",
                   (long long)B, (long long)T);
  if (workspace_bytes < pl.part_bytes)
    return set_err(EKS_ERR_ARG, "eks_fit_pupil: workspace too small (%zu < %zu)", workspace_bytes,
                   pl.part_bytes);
  hipStream_t s = (hipStream_t)stream;
  double *part = (double *)workspace;
  prof_call_begin();
  int rc;
  if (planes) {
    const double *evp =
        (const double *)((const char *)obs +
                         yev_ev_offset(B, T, n, obs_dtype == EKS_YEV32 ? 4 : sizeof(double)));
    auto run = [&](auto tag) -> int {
      using YT = decltype(tag);
      const PlaneSrc<YT> src{(const YT *)obs, evp, B};
      return pl.frames_map ? launch_accum<true>(src, pl, part, s)
                           : launch_accum<false>(src, pl, part, s);
    };
    rc = obs_dtype == EKS_YEV32 ? run(float{}) : run(double{});
  } else {
    double *y = (double *)yev;
    double *ev = yev ? (double *)((char *)yev + yev_ev_offset(B, T, n, sizeof(double))) : nullptr;
    const int row1 = B == 1 && yev && aligned16(y) && aligned16(ev) ? 1 : 0;
    const int median = mode == EKS_MEDIAN ? 1 : 0;
    auto run = [&](auto Ec, auto tag) -> int {
      using Tp = decltype(tag);
      constexpr int EE = decltype(Ec)::value;
      const size_t ts = sizeof(Tp);
      // whole frames of consecutive, 16-byte aligned member values
      const bool packed = EE > 0 && pl.frames_map && sj == 1 && se == kPupilN &&
                          aligned16(obs) && (st * ts) % 16 == 0 && (B == 1 || (sb * ts) % 16 == 0);
      if constexpr (EE > 0) {
        if (packed) {
          const MemberSrc<EE, Tp, true> src{(const Tp *)obs, sb, st, se, sj, E, median, y, ev, B, row1};
          return launch_accum<true>(src, pl, part, s);
        }
      }
      const MemberSrc<EE, Tp, false> src{(const Tp *)obs, sb, st, se, sj, E, median, y, ev, B, row1};
      return pl.frames_map ? launch_accum<true>(src, pl, part, s)
                           : launch_accum<false>(src, pl, part, s);
    };
    auto by_e = [&](auto tag) -> int {
      switch (E) {  // eks_ensemble_gaps's compiled member counts (its bits)
        case 3: return run(ic<3>{}, tag);
        case 4: return run(ic<4>{}, tag);
        case 5: return run(ic<5>{}, tag);
        case 8: return run(ic<8>{}, tag);
        default: return run(ic<0>{}, tag);
      }
    };
    rc = obs_dtype == EKS_F32 ? by_e(float{}) : by_e(double{});
  }
  if (rc != EKS_OK) {
    prof_call_end(s);
    return rc;
  }
  prof_mark(s, "k_pupil_final");
  hipLaunchKernelGGL(k_pupil_final, dim3((unsigned)B), dim3(64), 0, s, (const double *)part,
                     (long long)B, pl.NP, stats, ncomplete, status);
  prof_call_end(s);
  return check_launch("k_pupil_final");
}
