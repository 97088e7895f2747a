// C ABI of the joint posterior draws through missing observations:
// eks_draws_gaps, eks_draws_gaps_workspace_bytes, eks_draws_gaps_chunk_len,
// eks_draws_noise (include/eks_hip.h).  Validates arguments, zeroes the status
// array, runs the five kernels of gap_smooth.hpp and then the draw stage of
// gap_draws.hpp for r = 2 or 3.
#include "gap_draws.hpp"

using namespace eks;

namespace eks {
long long g_draws_raw = 0;
}

namespace {
bool dr_shape_ok(int n, int r) { return (r == 2 || r == 3) && n >= 1 && n <= kMaxObsRt; }
constexpr long long kMaxDrawLanes = 1LL << 28;  // B * S: the 32-bit lane byte offset of a plane
constexpr long long kMaxDrawT = 1LL << 40;      // the counter's time field
}  // namespace

extern "C" {

size_t eks_draws_gaps_workspace_bytes(int64_t B, int64_t S, int64_t T, int n, int r) {
  if (B <= 0 || S < 0 || T <= 0 || !dr_shape_ok(n, r)) return 0;
  if (S > 0 && B > kMaxDrawLanes / S) return 0;
  const GpPlan g = gp_make_plan(B, T, r, gp_chunk_len(B, T, r));
  return dr_make_plan(g, B, S, T, n, r).total;
}

int64_t eks_draws_gaps_chunk_len(int64_t B, int64_t T, int r) {
  if (B <= 0 || T <= 0 || (r != 2 && r != 3)) return 0;
  return gp_chunk_len(B, T, r);
}

int eks_draws_gaps(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                   int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, const double *params,
                   int64_t S, const double *noise, int64_t zb, int64_t zs, int64_t zt,
                   uint64_t seed, double *draws, int64_t db, int64_t ds, int64_t dt, int64_t dj,
                   double *xdraws, double *out, int64_t ob, int64_t ot, int64_t oj, double *pvar,
                   void *workspace, size_t workspace_bytes, int32_t *status, void *stream) {
  clear_err();
  if (!obs || !params || !draws || !status)
    return set_err(EKS_ERR_ARG, "eks_draws_gaps: NULL pointer");
  if (B < 0 || T < 1 || E < 1 || n < 1)
    return set_err(EKS_ERR_ARG, "eks_draws_gaps: need B>=0, T>=1, E>=1, n>=1");
  if (S < 0) return set_err(EKS_ERR_ARG, "eks_draws_gaps: need S>=0");
  if (pvar && !out) return set_err(EKS_ERR_ARG, "eks_draws_gaps: pvar has out's strides, pass out");
  if (obs_dtype != EKS_F32 && obs_dtype != EKS_F64 && obs_dtype != EKS_YEV32 &&
      obs_dtype != EKS_YEV64)
    return set_err(EKS_ERR_ARG, "eks_draws_gaps: bad dtype");
  if (mode != EKS_MEDIAN && mode != EKS_MEAN)
    return set_err(EKS_ERR_ARG, "eks_draws_gaps: bad mode");
  if (E > kMaxMembers)
    return set_err(EKS_ERR_UNSUPPORTED, "eks_draws_gaps: E=%d > %d", E, kMaxMembers);
  if (!dr_shape_ok(n, r))
    return set_err(EKS_ERR_UNSUPPORTED,
                   "eks_draws_gaps: (r=%d, n=%d) not supported (r = 2 or 3, n <= %d)", r, n,
                   kMaxObsRt);
  if (T > kMaxDrawT || (S > 0 && B > kMaxDrawLanes / S))
    return set_err(EKS_ERR_UNSUPPORTED, "eks_draws_gaps: need B * S <= 2^28 and T <= 2^40");
  if (B == 0) return EKS_OK;
  const GpPlan p = gp_make_plan(B, T, r, gp_chunk_len(B, T, r));
  const DrPlan d = dr_make_plan(p, B, S, T, n, r);
  if (!workspace || workspace_bytes < d.total)
    return set_err(EKS_ERR_ARG, "eks_draws_gaps: workspace of %zu bytes needed", d.total);
  hipStream_t s = (hipStream_t)stream;
  char *ws = (char *)workspace;
  if (hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(ws + d.bad_off, 0, (size_t)B * sizeof(int32_t), s) != hipSuccess)
    return set_err(EKS_ERR_HIP, "eks_draws_gaps: hipMemsetAsync(status) failed");
  // the smoother as eks_smooth_gaps runs it; ms_t stays in the workspace, and
  // out goes to workspace planes when the caller wants none
  GpArgs a{obs, obs_dtype, B,  T,  E,    n,   sb,      st,      se,      sj, mode == EKS_MEDIAN,
           params, out,    ob, ot, oj,   pvar, (double *)(ws + d.ms_off), nullptr, nullptr,
           nullptr, ws,    status, s};
  if (!out) {
    a.out = (double *)(ws + d.out_off);
    a.ob = n;
    a.ot = (long long)B * n;
    a.oj = 1;
  }
  const int rc = r == 2 ? launch_gp<2>(a, p) : launch_gp<3>(a, p);
  if (rc || S == 0) return rc;
  const DrArgs da{B, S, T, n, params, noise, zb, zs, zt, seed, draws, db, ds, dt, dj, xdraws,
                  ws, status, s};
  return r == 2 ? launch_dr<2>(da, p, d) : launch_dr<3>(da, p, d);
}

int eks_draws_noise(int64_t B, int64_t S, int64_t T, int r, uint64_t seed, double *noise,
                    int64_t zb, int64_t zs, int64_t zt, void *stream) {
  clear_err();
  if (B < 0 || S < 0 || T < 0) return set_err(EKS_ERR_ARG, "eks_draws_noise: need B, S, T >= 0");
  if (r != 2 && r != 3) return set_err(EKS_ERR_UNSUPPORTED, "eks_draws_noise: r = 2 or 3");
  if (T > kMaxDrawT || (S > 0 && B > kMaxDrawLanes / S))
    return set_err(EKS_ERR_UNSUPPORTED, "eks_draws_noise: need B * S <= 2^28 and T <= 2^40");
  if (B == 0 || S == 0 || T == 0) return EKS_OK;
  if (T > (1LL << 62) / (B * S))
    return set_err(EKS_ERR_UNSUPPORTED, "eks_draws_noise: B * S * T overflows");
  if (!noise) return set_err(EKS_ERR_ARG, "eks_draws_noise: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)std::min<long long>((B * S * T + kBlock - 1) / kBlock, 1 << 16);
  const int raw = g_draws_raw != 0;
  if (r == 2)
    hipLaunchKernelGGL((k_dr_noise<2>), dim3(grid), dim3(kBlock), 0, s, B, S, T, seed, raw, noise,
                       zb, zs, zt);
  else
    hipLaunchKernelGGL((k_dr_noise<3>), dim3(grid), dim3(kBlock), 0, s, B, S, T, seed, raw, noise,
                       zb, zs, zt);
  return check_launch("k_dr_noise");
}

}  // extern "C"
