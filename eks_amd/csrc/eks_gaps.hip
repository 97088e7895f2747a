// C ABI of smoothing through missing observations: eks_smooth_gaps,
// eks_smooth_gaps_workspace_bytes, eks_smooth_gaps_chunk_len
// (include/eks_hip.h).  Validates arguments, zeroes the status array and
// launches the five kernels of gap_smooth.hpp for r = 2 or 3.
#include "gap_smooth.hpp"

using namespace eks;

namespace eks {
long long g_gaps_chunk = 0;
}

extern "C" {

size_t eks_smooth_gaps_workspace_bytes(int64_t B, int64_t T, int n, int r) {
  if (B <= 0 || T <= 0 || !chunked_shape_ok(n, r)) return 0;
  return gp_make_plan(B, T, r, gp_chunk_len(B, T, r)).total;
}

int64_t eks_smooth_gaps_chunk_len(int64_t B, int64_t T, int r) {
  if (B <= 0 || T <= 0 || (r != 2 && r != 3)) return 0;
  return gp_chunk_len(B, T, r);
}

int eks_smooth_gaps(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                    int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, const double *params,
                    double *out, int64_t ob, int64_t ot, int64_t oj, double *pvar, double *ms,
                    double *Vs, double *nll, int32_t *nobs, void *workspace,
                    size_t workspace_bytes, int32_t *status, void *stream) {
  clear_err();
  const char *fn = "eks_smooth_gaps";
  if (int rc = check_member_args(fn, obs && params && out && status, B, T, E, n, r, obs_dtype, mode))
    return rc;
  if (B == 0) return EKS_OK;
  const GpPlan p = gp_make_plan(B, T, r, gp_chunk_len(B, T, r));
  if (int rc = check_workspace(fn, workspace, workspace_bytes, p.total)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = zero_status(fn, status, B, s)) return rc;
  const GpArgs a{obs, obs_dtype, B,  T,  E,    n,   sb,   st,  se,   sj,     mode == EKS_MEDIAN,
                 params, out,    ob, ot, oj,   pvar, ms,  Vs,  nll,  nobs,   (char *)workspace,
                 status, s};
  return r == 2 ? launch_gp<2>(a, p) : launch_gp<3>(a, p);
}

}  // extern "C"
