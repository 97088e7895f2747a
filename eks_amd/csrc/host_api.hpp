// Host-side helpers of the chunked-scan entry points (eks_smooth_var,
// eks_smooth_gaps, eks_nll_sweep, eks_nll_sweep_gaps, eks_draws_gaps): the
// argument check, the workspace check, the status memset, the chunk-length
// rule, the workspace carver, the input dispatch and the launch pairs their
// launchers share.
// Plain functions and small templates, host only: no kernel and no EKS_DEV
// function lives here, and nothing here is a kernel argument.
#pragma once
#include "smooth_impl.hpp"

namespace eks {

// the shapes the chunked-scan kernels serve: R is a template argument, n a loop bound
inline bool chunked_shape_ok(int n, int r) { return (r == 2 || r == 3) && n >= 1 && n <= kMaxObsRt; }

// K * B rows of a sweep are addressed by 32-bit byte offsets within a plane
inline bool sweep_rows_ok(long long B, long long K) { return B <= (1LL << 28) / (K > 0 ? K : 1); }

// The arguments every entry point of the family takes, checked in the order
// the return codes document: a NULL pointer, the sizes, `own` (the message of
// the entry point's own failed size check, NULL if none: K, S, pvar without
// out), the input code, the averaging mode, the member cap and the shape.
// `fn` starts every message.  An entry point without a mode passes EKS_MEDIAN.
inline int check_member_args(const char *fn, bool pointers_ok, long long B, long long T, int E,
                             int n, int r, int dtype, int mode, const char *own = nullptr) {
  if (!pointers_ok) return set_err(EKS_ERR_ARG, "%s: NULL pointer", fn);
  if (B < 0 || T < 1 || E < 1 || n < 1)
    return set_err(EKS_ERR_ARG, "%s: need B>=0, T>=1, E>=1, n>=1", fn);
  if (own) return set_err(EKS_ERR_ARG, "%s: %s", fn, own);
  if (dtype != EKS_F32 && dtype != EKS_F64 && dtype != EKS_YEV32 && dtype != EKS_YEV64)
    return set_err(EKS_ERR_ARG, "%s: bad dtype", fn);
  if (mode != EKS_MEDIAN && mode != EKS_MEAN)
    return set_err(EKS_ERR_ARG, "%s: bad averaging mode", fn);
  if (E > kMaxMembers) return set_err(EKS_ERR_UNSUPPORTED, "%s: E=%d > %d", fn, E, kMaxMembers);
  if (!chunked_shape_ok(n, r))
    return set_err(EKS_ERR_UNSUPPORTED, "%s: (r=%d, n=%d) not supported (r = 2 or 3, n <= %d)", fn,
                   r, n, kMaxObsRt);
  return EKS_OK;
}

inline int check_workspace(const char *fn, const void *workspace, size_t have, size_t need) {
  if (!workspace || have < need)
    return set_err(EKS_ERR_ARG, "%s: workspace of %zu bytes needed", fn, need);
  return EKS_OK;
}

// zeroes `words` status words (or another int32 array the kernels OR into)
inline int zero_status(const char *fn, int32_t *status, long long words, hipStream_t s) {
  if (hipMemsetAsync(status, 0, (size_t)words * sizeof(int32_t), s) != hipSuccess)
    return set_err(EKS_ERR_HIP, "%s: hipMemsetAsync(status) failed", fn);
  return EKS_OK;
}

// Chunk length as launched: a multiple of 8, one chunk when it covers T.
// `forced` > 0 (a debug key) is taken as it is; else `base`, and with few
// trajectories (chunk-major lanes, B <= 256) not less than c sqrt(T), c = c2 at
// r = 2 and c3 at r = 3 (0: no such floor).  The callers hold the measurements
// behind their base and constants (base is a call_chunk_len value: pure
// arithmetic, so it costs nothing to have it at hand when a key forces L).
inline long long chunk_len_rule(long long forced, long long base, double c2, double c3, long long B,
                                long long T, int r) {
  long long L = forced > 0 ? round_up(forced, 8) : base;
  const double c = r <= 2 ? c2 : c3;
  if (forced <= 0 && c > 0 && !uniform_lanes(B) && B <= 256)
    L = std::max(L, round_up(std::llround(c * std::sqrt((double)T)), 8));
  if (L >= T) L = round_up(T, 8);
  return L;
}

// carves 256-byte aligned arrays out of a workspace, in the order of the calls
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off = align256(off + bytes);
    return o;
  }
};

// the ev planes of the caller's buffer when `dtype` is a y / ev hand-off, else NULL
inline const char *yev_ev_planes(const void *obs, int dtype, long long B, long long T, int n) {
  if (dtype != EKS_YEV32 && dtype != EKS_YEV64) return nullptr;
  return (const char *)obs + yev_ev_offset(B, T, n, dtype == EKS_YEV32 ? 4 : 8);
}

// k(input tag, member count) for the input code: YevIn<float> / YevIn<double>
// with ic<0> (the members are not read), float / double with the compiled
// member count.  YEV_TYPED = false: the kernel reads only the ev planes, which
// are doubles in both hand-off forms, so both run k(YevIn<double>).
template <bool YEV_TYPED = true, typename F>
int dispatch_input(int dtype, int E, F &&k) {
  if constexpr (YEV_TYPED)
    if (dtype == EKS_YEV32) return k(YevIn<float>{}, ic<0>{});
  if (dtype == EKS_YEV32 || dtype == EKS_YEV64) return k(YevIn<double>{}, ic<0>{});
  if (dtype == EKS_F32) return dispatch_members_c(E, [&](auto Ec) { return k(float{}, Ec); });
  return dispatch_members_c(E, [&](auto Ec) { return k(double{}, Ec); });
}

// grid of a per-lane kernel over NC chunks of `rows` trajectories (or rows)
inline unsigned lane_grid(long long NC, long long rows) {
  return uniform_lanes(rows) ? (unsigned)(NC * blocks_per_chunk(rows)) : grid_for(NC * rows, kBlock);
}

// a per-lane kernel: its <.., true> instantiation when every block lies in
// one chunk (uniform_lanes), else its <.., false> one
template <typename... KArgs, typename... Args>
void launch_uni(bool uni, void (*k_uni)(KArgs...), void (*k_mixed)(KArgs...), unsigned grid,
                hipStream_t s, const Args &...args) {
  hipLaunchKernelGGL(uni ? k_uni : k_mixed, dim3(grid), dim3(kBlock), 0, s, args...);
}

// a scan over the chunks of `rows` trajectories (or rows): one lane per row
// while NC <= wave_scan_chunks(), above that one wave per row
template <typename... KArgs, typename... Args>
void launch_scan(bool wave_scan, void (*k_lane)(KArgs...), void (*k_wave)(KArgs...),
                 long long rows, hipStream_t s, const Args &...args) {
  if (!wave_scan)
    hipLaunchKernelGGL(k_lane, dim3(grid_for(rows, 64)), dim3(64), 0, s, args...);
  else
    hipLaunchKernelGGL(k_wave, dim3((unsigned)rows), dim3(64), 0, s, args...);
}

}  // namespace eks
