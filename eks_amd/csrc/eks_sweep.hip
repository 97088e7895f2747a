// C ABI of the likelihood sweep: eks_nll_sweep, eks_nll_sweep_workspace_bytes,
// eks_nll_sweep_chunk_len (include/eks_hip.h).  Validates arguments, zeroes
// the status array and launches the kernels of nll_sweep.hpp for r = 2 or 3.
#include "nll_sweep.hpp"

using namespace eks;

namespace eks {
long long g_sweep_chunk = 0;
}

extern "C" {

size_t eks_nll_sweep_workspace_bytes(int64_t B, int64_t K, int64_t T, int n, int r) {
  if (B <= 0 || K <= 0 || T <= 0 || !chunked_shape_ok(n, r) || !sweep_rows_ok(B, K)) return 0;
  return sw_make_plan(B, K, T, r, sw_chunk_len(B, T, r)).total;
}

int64_t eks_nll_sweep_chunk_len(int64_t B, int64_t K, int64_t T, int r) {
  if (B <= 0 || K <= 0 || T <= 0 || (r != 2 && r != 3) || !sweep_rows_ok(B, K)) return 0;
  return sw_chunk_len(B, T, r);
}

int eks_nll_sweep(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                  int64_t sb, int64_t st, int64_t se, int64_t sj, int mode, const double *params,
                  int64_t K, double *nll, void *workspace, size_t workspace_bytes, int32_t *status,
                  void *stream) {
  clear_err();
  const char *fn = "eks_nll_sweep";
  if (int rc = check_member_args(fn, obs && params && nll && status, B, T, E, n, r, obs_dtype, mode,
                                 K < 0 ? "need K>=0" : nullptr))
    return rc;
  if (B == 0 || K == 0) return EKS_OK;
  if (!sweep_rows_ok(B, K))
    return set_err(EKS_ERR_UNSUPPORTED, "%s: K * B = %lld rows > 2^28", fn, (long long)(K * B));
  const SwPlan p = sw_make_plan(B, K, T, r, sw_chunk_len(B, T, r));
  if (int rc = check_workspace(fn, workspace, workspace_bytes, p.total)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = zero_status(fn, status, K * B, s)) return rc;
  const SwArgs a{obs, obs_dtype, B, T, E, n, sb, st, se, sj, mode == EKS_MEDIAN ? 1 : 0,
                 params, K, nll, (char *)workspace, status, s};
  return r == 2 ? launch_sw<2>(a, p) : launch_sw<3>(a, p);
}

}  // extern "C"
