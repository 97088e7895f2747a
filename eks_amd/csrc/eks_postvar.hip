// C ABI of the posterior-variance pass: eks_smooth_var,
// eks_smooth_var_workspace_bytes, eks_smooth_var_chunk_len (include/eks_hip.h).
// Validates arguments, zeroes the status array and launches the five kernels
// of post_var.hpp for r = 2 or 3.
#include "post_var.hpp"

using namespace eks;

namespace eks {
long long g_pvar_chunk = 0;
}

namespace {
bool pv_shape_ok(int n, int r) { return (r == 2 || r == 3) && n >= 1 && n <= kMaxObsRt; }
}  // namespace

extern "C" {

size_t eks_smooth_var_workspace_bytes(int64_t B, int64_t T, int n, int r) {
  if (B <= 0 || T <= 0 || !pv_shape_ok(n, r)) return 0;
  return pv_make_plan(B, T, r, pv_chunk_len(B, T, r)).total;
}

int64_t eks_smooth_var_chunk_len(int64_t B, int64_t T, int r) {
  if (B <= 0 || T <= 0 || (r != 2 && r != 3)) return 0;
  return pv_chunk_len(B, T, r);
}

int eks_smooth_var(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                   int64_t sb, int64_t st, int64_t se, int64_t sj, const double *params,
                   double *pvar, int64_t vb, int64_t vt, int64_t vj, double *Vs, void *workspace,
                   size_t workspace_bytes, int32_t *status, void *stream) {
  clear_err();
  if (!obs || !params || !pvar || !status)
    return set_err(EKS_ERR_ARG, "eks_smooth_var: NULL pointer");
  if (B < 0 || T < 1 || E < 1 || n < 1)
    return set_err(EKS_ERR_ARG, "eks_smooth_var: need B>=0, T>=1, E>=1, n>=1");
  if (obs_dtype != EKS_F32 && obs_dtype != EKS_F64 && obs_dtype != EKS_YEV32 &&
      obs_dtype != EKS_YEV64)
    return set_err(EKS_ERR_ARG, "eks_smooth_var: bad dtype");
  if (E > kMaxMembers)
    return set_err(EKS_ERR_UNSUPPORTED, "eks_smooth_var: E=%d > %d", E, kMaxMembers);
  if (!pv_shape_ok(n, r))
    return set_err(EKS_ERR_UNSUPPORTED,
                   "eks_smooth_var: (r=%d, n=%d) not supported (r = 2 or 3, n <= %d)", r, n,
                   kMaxObsRt);
  if (B == 0) return EKS_OK;
  const PvPlan p = pv_make_plan(B, T, r, pv_chunk_len(B, T, r));
  if (!workspace || workspace_bytes < p.total)
    return set_err(EKS_ERR_ARG, "eks_smooth_var: workspace of %zu bytes needed", p.total);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), s) != hipSuccess)
    return set_err(EKS_ERR_HIP, "eks_smooth_var: hipMemsetAsync(status) failed");
  const PvArgs a{obs, obs_dtype, B, T, E, n, sb, st, se, sj, params, pvar, vb, vt, vj, Vs,
                 (char *)workspace, status, s};
  return r == 2 ? launch_pv<2>(a, p) : launch_pv<3>(a, p);
}

}  // extern "C"
