// C ABI of the likelihood sweep through missing observations:
// eks_nll_sweep_gaps, eks_nll_sweep_gaps_workspace_bytes,
// eks_nll_sweep_gaps_chunk_len (include/eks_hip.h).  Validates arguments,
// zeroes the status array and launches the kernels of gap_sweep.hpp for
// r = 2 or 3.
#include "gap_sweep.hpp"

using namespace eks;

namespace eks {
long long g_gaps_sweep_chunk = 0;
}

namespace {
bool gs_shape_ok(int n, int r) { return (r == 2 || r == 3) && n >= 1 && n <= kMaxObsRt; }
// rows are addressed by 32-bit byte offsets within a plane
bool gs_rows_ok(long long B, long long K) { return B <= (1LL << 28) / (K > 0 ? K : 1); }
}  // namespace

extern "C" {

size_t eks_nll_sweep_gaps_workspace_bytes(int64_t B, int64_t K, int64_t T, int n, int r) {
  if (B <= 0 || K <= 0 || T <= 0 || !gs_shape_ok(n, r) || !gs_rows_ok(B, K)) return 0;
  return gs_make_plan(B, K, T, r, gs_chunk_len(B, T, r)).total;
}

int64_t eks_nll_sweep_gaps_chunk_len(int64_t B, int64_t K, int64_t T, int r) {
  if (B <= 0 || K <= 0 || T <= 0 || (r != 2 && r != 3) || !gs_rows_ok(B, K)) return 0;
  return gs_chunk_len(B, T, r);
}

int eks_nll_sweep_gaps(const void *obs, int obs_dtype, int64_t B, int64_t T, int E, int n, int r,
                       int64_t sb, int64_t st, int64_t se, int64_t sj, int mode,
                       const double *params, int64_t K, double *nll, int32_t *nobs,
                       void *workspace, size_t workspace_bytes, int32_t *status, void *stream) {
  clear_err();
  if (!obs || !params || !nll || !status)
    return set_err(EKS_ERR_ARG, "eks_nll_sweep_gaps: NULL pointer");
  if (B < 0 || K < 0 || T < 1 || E < 1 || n < 1)
    return set_err(EKS_ERR_ARG, "eks_nll_sweep_gaps: need B>=0, K>=0, T>=1, E>=1, n>=1");
  if (obs_dtype != EKS_F32 && obs_dtype != EKS_F64 && obs_dtype != EKS_YEV32 &&
      obs_dtype != EKS_YEV64)
    return set_err(EKS_ERR_ARG, "eks_nll_sweep_gaps: bad dtype");
  if (mode != EKS_MEDIAN && mode != EKS_MEAN)
    return set_err(EKS_ERR_ARG, "eks_nll_sweep_gaps: bad averaging mode");
  if (E > kMaxMembers)
    return set_err(EKS_ERR_UNSUPPORTED, "eks_nll_sweep_gaps: E=%d > %d", E, kMaxMembers);
  if (!gs_shape_ok(n, r))
    return set_err(EKS_ERR_UNSUPPORTED,
                   "eks_nll_sweep_gaps: (r=%d, n=%d) not supported (r = 2 or 3, n <= %d)", r, n,
                   kMaxObsRt);
  if (B == 0 || K == 0) return EKS_OK;
  if (!gs_rows_ok(B, K))
    return set_err(EKS_ERR_UNSUPPORTED, "eks_nll_sweep_gaps: K * B = %lld rows > 2^28",
                   (long long)(K * B));
  const GsPlan p = gs_make_plan(B, K, T, r, gs_chunk_len(B, T, r));
  if (!workspace || workspace_bytes < p.total)
    return set_err(EKS_ERR_ARG, "eks_nll_sweep_gaps: workspace of %zu bytes needed", p.total);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(status, 0, (size_t)(K * B) * sizeof(int32_t), s) != hipSuccess)
    return set_err(EKS_ERR_HIP, "eks_nll_sweep_gaps: hipMemsetAsync(status) failed");
  const GsArgs a{obs, obs_dtype, B, T, E, n, sb, st, se, sj, mode == EKS_MEDIAN ? 1 : 0,
                 params, K, nll, nobs, (char *)workspace, status, s};
  return r == 2 ? launch_gs<2>(a, p) : launch_gs<3>(a, p);
}

}  // extern "C"
