// C ABI of the posterior-variance pass: eks_smooth_var,
// eks_smooth_var_workspace_bytes, eks_smooth_var_chunk_len (include/eks_hip.h).
// Validates arguments, zeroes the status array and launches the five kernels
// of post_var.hpp for r = 2 or 3.
#include "post_var.hpp"

using namespace eks;

namespace eks {
long long g_pvar_chunk = 0;
}

extern "C" {

size_t eks_smooth_var_workspace_bytes(int64_t B, int64_t T, int n, int r) {
  if (B <= 0 || T <= 0 || !chunked_shape_ok(n, r)) return 0;
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
  const char *fn = "eks_smooth_var";
  // (no averaging mode: the variances of the members are read in either)
  if (int rc = check_member_args(fn, obs && params && pvar && status, B, T, E, n, r, obs_dtype,
                                 EKS_MEDIAN))
    return rc;
  if (B == 0) return EKS_OK;
  const PvPlan p = pv_make_plan(B, T, r, pv_chunk_len(B, T, r));
  if (int rc = check_workspace(fn, workspace, workspace_bytes, p.total)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = zero_status(fn, status, B, s)) return rc;
  const PvArgs a{obs, obs_dtype, B, T, E, n, sb, st, se, sj, params, pvar, vb, vt, vj, Vs,
                 (char *)workspace, status, s};
  return r == 2 ? launch_pv<2>(a, p) : launch_pv<3>(a, p);
}

}  // extern "C"
