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
constexpr long long kMaxDrawLanes = 1LL << 28;  // B * S: the 32-bit lane byte offset of a plane
constexpr long long kMaxDrawT = 1LL << 40;      // the counter's time field
}  // namespace

extern "C" {

size_t eks_draws_gaps_workspace_bytes(int64_t B, int64_t S, int64_t T, int n, int r) {
  if (B <= 0 || S < 0 || T <= 0 || !chunked_shape_ok(n, r)) return 0;
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
  const char *fn = "eks_draws_gaps";
  const char *own = S < 0 ? "need S>=0" : pvar && !out ? "pvar has out's strides, pass out" : nullptr;
  if (int rc = check_member_args(fn, obs && params && draws && status, B, T, E, n, r, obs_dtype,
                                 mode, own))
    return rc;
  if (T > kMaxDrawT || (S > 0 && B > kMaxDrawLanes / S))
    return set_err(EKS_ERR_UNSUPPORTED, "eks_draws_gaps: need B * S <= 2^28 and T <= 2^40");
  if (B == 0) return EKS_OK;
  const GpPlan p = gp_make_plan(B, T, r, gp_chunk_len(B, T, r));
  const DrPlan d = dr_make_plan(p, B, S, T, n, r);
  if (int rc = check_workspace(fn, workspace, workspace_bytes, d.total)) return rc;
  hipStream_t s = (hipStream_t)stream;
  char *ws = (char *)workspace;
  if (int rc = zero_status(fn, status, B, s)) return rc;
  if (int rc = zero_status(fn, (int32_t *)(ws + d.bad_off), B, s)) return rc;
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
