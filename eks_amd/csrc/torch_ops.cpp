// torch.ops.eks.*: the C ABI of libeks_hip.so registered as PyTorch operators
// in C++ ("the torch extension wraps the same functions as
// torch.ops.eks.*"; BASELINE north star: ensemble() / forward_pass() /
// backward_pass() / compute_nll() as a PyTorch-ROCm C++/HIP extension).
//
// Built by eks_amd/build.py into eks_amd/lib/libeks_torch.so (linked against
// libtorch and libeks_hip.so) and loaded by eks_amd/ops.py with
// torch.ops.load_library: the operators' dispatch has no Python frame.  Each
// operator has a CUDA-key kernel (the HIP device: on ROCm builds of PyTorch
// the GPU dispatch key is CUDA) that launches on the current stream, and a
// Meta kernel that only computes shapes (FakeTensor / torch.compile tracing).
// The two are one function, X_op, so the output shapes are written once: it
// checks the shapes, allocates the outputs from its first argument's options
// (meta tensors for a meta input) and, unless that argument is a meta tensor,
// requires GPU tensors and goes on to the device work.  X_gpu and X_meta name
// it for the two keys.
// There is no CPU kernel: a CPU tensor is a dispatch error.
//
//   eks::ensemble(obs, mode)                       eks/ensemble_kalman.py:4-57
//   eks::forward(y, ev, m0, S0, A, Q, C)           :59-117  (filtering_pass)
//   eks::backward(mf, Vf, S, A)                    :120-164 (smooth_backward)
//   eks::nll(obs, params, n, r, mode, flags)       compute_nll
//   eks::smooth(obs, params, n, r, mode, flags, algo)  the fused hot path
//   eks::smooth_var(obs, params, n, r)             posterior variances of smooth's output
//   eks::smooth_gaps(obs, params, n, r, mode)      the smoother through missing observations
//   eks::draws_gaps(obs, params, noise, n, r, mode)  joint posterior draws from given noise
//   eks::draws_noise(like, B, S, T, r, seed)       the noise of a seeded draws call
//   eks::nll_sweep(obs, params, K, n, r, mode)     the NLL of K candidate models per trajectory
//   eks::nll_sweep_gaps(obs, params, K, n, r, mode)  the same through missing observations
//   eks::fit(obs, kind, n, r, s, q, mode)          eks/multiview_pca_smoother.py:684-731
//   eks::fit_gaps(obs, kind, n, r, s, q, mode)     the same through missing observations
//   eks::ensemble_gaps(obs, mode, min_members)     the ensemble over the valid members
//   eks::fit_pupil(obs, mode)                      the pupil model's statistics (complete frames)
//   eks::newton_filter(y, ev, mu0, S0, A, Bm, E, max_iter)  eks/newton_eks.py:115-148
//   eks::interp1d(x, y, xq)                        eks/multiview_pca_smoother.py:86-96
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <initializer_list>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/eks_hip.h"

namespace {

using at::Tensor;
using T2 = std::tuple<Tensor, Tensor>;
using T3 = std::tuple<Tensor, Tensor, Tensor>;
using T4 = std::tuple<Tensor, Tensor, Tensor, Tensor>;
using T5 = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor>;

// (ROCm PyTorch: the HIP device is the "cuda" device type; its streams and
// guard are the masquerading ones)
void* cur_stream(const Tensor& t) {
  return (void*)at::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

void check(int rc, const char* what) {
  TORCH_CHECK(rc == EKS_OK, what, " failed (code ", rc, "): ", eks_last_error());
}

int mode_code(const std::string& mode) {
  TORCH_CHECK(mode == "median" || mode == "mean", mode, " averaging not supported");
  return mode == "median" ? EKS_MEDIAN : EKS_MEAN;
}

int fit_kind(const std::string& kind) {
  TORCH_CHECK(kind == "singleview" || kind == "multicam", "kind must be singleview or multicam");
  return kind == "singleview" ? EKS_FIT_SINGLEVIEW : EKS_FIT_MULTICAM;
}

int obs_dtype(const Tensor& obs) {
  TORCH_CHECK(obs.scalar_type() == at::kFloat || obs.scalar_type() == at::kDouble,
              "obs must be float32 or float64");
  return obs.scalar_type() == at::kFloat ? EKS_F32 : EKS_F64;
}

void need_gpu(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "eks ops run on the GPU only (no CPU fallback): ", name,
              " is a ", t.device().str(), " tensor");
}

at::TensorOptions f64(const Tensor& like) { return like.options().dtype(at::kDouble); }
at::TensorOptions i32(const Tensor& like) { return like.options().dtype(at::kInt); }

Tensor contiguous_f64(const Tensor& t) { return t.to(at::kDouble).contiguous(); }

// an argument of the call's device: moved there (float64, contiguous) when it
// is a host / numpy-derived tensor, so no host pointer reaches a kernel
Tensor on_dev_f64(const Tensor& t, const Tensor& like) {
  return t.to(like.device(), at::kDouble).contiguous();
}

// model argument `t` must be lead + shp: per trajectory (lead = {B}) or
// shared by every trajectory (lead = {}), as the Python shims check
// (eks_amd/newton_eks.py: newton_filter_batch)
void check_shape(const Tensor& t, const char* name, bool shared, int64_t B,
                 std::initializer_list<int64_t> shp) {
  std::vector<int64_t> want;
  if (!shared) want.push_back(B);
  want.insert(want.end(), shp.begin(), shp.end());
  TORCH_CHECK(t.sizes().vec() == want, name, " has shape ", t.sizes(), ", expected ",
              at::IntArrayRef(want));
}

// The member input of an operator: obs viewed as (B, T, E, n) with the
// operator's n (want_n < 0: any n) and a supported dtype (`code`).  Off the
// Meta key obs is a GPU tensor, and its device is current while this lives.
struct MemberIn {
  int64_t B, T;
  int E, n, code;
  bool meta;
  c10::OptionalDeviceGuard guard;
  explicit MemberIn(const Tensor& obs, int64_t want_n = -1) : meta(obs.is_meta()) {
    if (!meta) need_gpu(obs, "obs");
    TORCH_CHECK(obs.dim() == 4, "obs must be viewed as (B, T, E, n)");
    TORCH_CHECK(want_n < 0 || obs.size(3) == want_n,
                "obs must be viewed as (B, T, E, n) with n=", want_n);
    B = obs.size(0), T = obs.size(1), E = (int)obs.size(2), n = (int)obs.size(3);
    code = obs_dtype(obs);
    if (!meta) guard.reset_device(obs.device());
  }
};

// the model rows of `rows` trajectories (or candidates), on obs's device
Tensor param_rows(const Tensor& params, const Tensor& obs, int64_t rows, int n, int64_t r) {
  need_gpu(params, "params");
  TORCH_CHECK(params.device() == obs.device(), "params is on ", params.device().str(),
              ", obs on ", obs.device().str());
  Tensor prm = params.contiguous();
  const int64_t P = eks_param_len(n, (int)r);
  TORCH_CHECK(prm.scalar_type() == at::kDouble && prm.dim() == 2 && prm.size(0) == rows &&
                  prm.size(1) == P,
              "params must be a (", rows, ", ", P, ") float64 tensor");
  return prm;
}

// byte buffers from PyTorch's caching allocator (stream ordered on the current
// stream, so reuse across calls is free); a workspace is never empty
Tensor bytes(const Tensor& like, size_t n) {
  return at::empty({(int64_t)n}, like.options().dtype(at::kByte));
}
Tensor workspace(const Tensor& like, size_t n) { return bytes(like, std::max<size_t>(n, 1)); }

// a (B, T, n) result is written time-major (coalesced stores) and returned contiguous
Tensor time_major(const Tensor& like, const MemberIn& in) {
  return at::empty({in.T, in.B, (int64_t)in.n}, f64(like));
}
Tensor batch_major(const Tensor& tm) { return tm.permute({1, 0, 2}).contiguous(); }

// ---------------------------------------------------------------- ensemble
T2 ensemble_op(const Tensor& obs, const std::string& mode) {
  const MemberIn in(obs);
  Tensor preds = at::empty({in.B, in.T, in.n}, f64(obs));
  Tensor vars = at::empty({in.B, in.T, in.n}, f64(obs));
  if (!in.meta)
    check(eks_ensemble(obs.data_ptr(), in.code, in.B, in.T, in.E, in.n, obs.stride(0),
                       obs.stride(1), obs.stride(2), obs.stride(3), mode_code(mode),
                       preds.data_ptr<double>(), vars.data_ptr<double>(), cur_stream(obs)),
          "eks_ensemble");
  return {preds, vars};
}
constexpr auto &ensemble_gpu = ensemble_op, &ensemble_meta = ensemble_op;

// ----------------------------------------------------------------- forward
// y, ev (B, T, n); m0 (B, r); S0, A, Q (B, r, r); C (B, n, r) -- or, with no
// leading B, one model shared by every trajectory.  R is diagonal = ev[t]
// (the reference overwrites R's diagonal every step and never reads the rest
// unless the caller's R has off-diagonal entries: the Python shim passes R).
T5 forward_op(const Tensor& y, const Tensor& ev, const Tensor& m0, const Tensor& S0,
              const Tensor& A, const Tensor& Q, const Tensor& C) {
  if (!y.is_meta()) need_gpu(y, "y");
  TORCH_CHECK(y.dim() == 3 && ev.sizes() == y.sizes(), "y and ev must both be (B, T, n)");
  TORCH_CHECK(m0.dim() == 1 || m0.dim() == 2, "m0 must be (r,) or (B, r)");
  const int64_t B = y.size(0), T = y.size(1), n = y.size(2), r = m0.size(-1);
  Tensor mf = at::empty({B, T, r}, f64(y));
  Tensor Vf = at::empty({B, T, r, r}, f64(y));
  Tensor S = at::empty({B, T, r, r}, f64(y));
  Tensor nll = at::empty({B}, f64(y));
  Tensor status = at::zeros({B}, i32(y));
  if (y.is_meta()) return {mf, Vf, S, nll, status};
  const c10::DeviceGuard g(y.device());
  const bool sh = m0.dim() == 1;
  check_shape(m0, "m0", sh, B, {r});
  check_shape(S0, "S0", sh, B, {r, r});
  check_shape(A, "A", sh, B, {r, r});
  check_shape(Q, "Q", sh, B, {r, r});
  check_shape(C, "C", sh, B, {n, r});
  Tensor y_ = contiguous_f64(y), ev_ = on_dev_f64(ev, y);
  Tensor m0_ = on_dev_f64(m0, y), S0_ = on_dev_f64(S0, y), A_ = on_dev_f64(A, y);
  Tensor Q_ = on_dev_f64(Q, y), C_ = on_dev_f64(C, y);
  check(eks_forward(B, T, (int)n, (int)r, y_.data_ptr<double>(), ev_.data_ptr<double>(),
                    m0_.data_ptr<double>(), S0_.data_ptr<double>(), A_.data_ptr<double>(),
                    Q_.data_ptr<double>(), C_.data_ptr<double>(), nullptr, sh ? 1 : 0,
                    mf.data_ptr<double>(), Vf.data_ptr<double>(), S.data_ptr<double>(),
                    nll.data_ptr<double>(), status.data_ptr<int32_t>(), cur_stream(y)),
        "eks_forward");
  return {mf, Vf, S, nll, status};
}
constexpr auto &forward_gpu = forward_op, &forward_meta = forward_op;

// ---------------------------------------------------------------- backward
T4 backward_op(const Tensor& mf, const Tensor& Vf, const Tensor& S, const Tensor& A) {
  if (!mf.is_meta()) need_gpu(mf, "mf");
  TORCH_CHECK(mf.dim() == 3, "mf must be (B, T, r)");
  TORCH_CHECK(A.dim() == 2 || A.dim() == 3, "A must be (r, r) or (B, r, r)");
  const int64_t B = mf.size(0), T = mf.size(1), r = mf.size(2);
  Tensor ms = at::empty({B, T, r}, f64(mf));
  Tensor Vs = at::empty({B, T, r, r}, f64(mf));
  Tensor CV = at::empty({B, T > 1 ? T - 1 : 0, r, r}, f64(mf));
  Tensor status = at::zeros({B}, i32(mf));
  if (mf.is_meta()) return {ms, Vs, CV, status};
  const c10::DeviceGuard g(mf.device());
  const bool sh = A.dim() == 2;
  TORCH_CHECK(Vf.sizes() == at::IntArrayRef({B, T, r, r}), "Vf has shape ", Vf.sizes(),
              ", expected (", B, ", ", T, ", ", r, ", ", r, ")");
  TORCH_CHECK(S.sizes() == at::IntArrayRef({B, T, r, r}), "S has shape ", S.sizes(),
              ", expected (", B, ", ", T, ", ", r, ", ", r, ")");
  check_shape(A, "A", sh, B, {r, r});
  Tensor mf_ = contiguous_f64(mf), Vf_ = on_dev_f64(Vf, mf), S_ = on_dev_f64(S, mf);
  Tensor A_ = on_dev_f64(A, mf);
  check(eks_backward(B, T, (int)r, mf_.data_ptr<double>(), Vf_.data_ptr<double>(),
                     S_.data_ptr<double>(), A_.data_ptr<double>(), sh ? 1 : 0,
                     ms.data_ptr<double>(), Vs.data_ptr<double>(),
                     T > 1 ? CV.data_ptr<double>() : nullptr, status.data_ptr<int32_t>(),
                     cur_stream(mf)),
        "eks_backward");
  return {ms, Vs, CV, status};
}
constexpr auto &backward_gpu = backward_op, &backward_meta = backward_op;

// --------------------------------------------------------- smooth / nll
// (out (B, T, n) or, filter only, nll (B); status (B))
T3 smooth_call(const Tensor& obs, const Tensor& params, int64_t n, int64_t r,
               const std::string& mode, int64_t flags, int64_t algo, bool want_out) {
  const MemberIn in(obs, n);
  const int64_t B = in.B, T = in.T;
  Tensor out_tm = want_out ? time_major(obs, in) : Tensor();
  Tensor nll = want_out ? Tensor() : at::empty({B}, f64(obs));
  Tensor status = at::empty({B}, i32(obs));
  if (!in.meta) {
    Tensor prm = param_rows(params, obs, B, in.n, r);
    Tensor ws = workspace(obs, eks_smooth_workspace_bytes(B, T, in.n, (int)r, in.E, (int)algo));
    check(eks_smooth(obs.data_ptr(), in.code, B, T, in.E, in.n, (int)r, obs.stride(0),
                     obs.stride(1), obs.stride(2), obs.stride(3), mode_code(mode),
                     prm.data_ptr<double>(), want_out ? out_tm.data_ptr<double>() : nullptr,
                     want_out ? n : 0, want_out ? B * n : 0, 1, nullptr,
                     want_out ? nullptr : nll.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel(),
                     (int)flags, (int)algo, status.data_ptr<int32_t>(), cur_stream(obs)),
          "eks_smooth");
  }
  return {want_out ? batch_major(out_tm) : Tensor(), nll, status};
}
T2 smooth_op(const Tensor& obs, const Tensor& params, int64_t n, int64_t r, const std::string& mode,
             int64_t flags, int64_t algo) {
  auto res = smooth_call(obs, params, n, r, mode, flags, algo, true);
  return {std::get<0>(res), std::get<2>(res)};
}
constexpr auto &smooth_gpu = smooth_op, &smooth_meta = smooth_op;

// compute_nll: the filter-only pass; raises where the reference's solve would
// (singular system) or when a model promise does not hold
Tensor nll_op(const Tensor& obs, const Tensor& params, int64_t n, int64_t r,
              const std::string& mode, int64_t flags) {
  auto res = smooth_call(obs, params, n, r, mode, flags, 0, false);
  if (obs.is_meta()) return std::get<1>(res);
  Tensor st = std::get<2>(res);
  const int64_t bad = st.ne(0).sum().item<int64_t>();
  if (bad) {
    // a chain breakdown (EKS_STATUS_SCAN) is retried with the sequential algorithm
    if (st.bitwise_and(EKS_STATUS_SCAN).ne(0).any().item<bool>())
      res = smooth_call(obs, params, n, r, mode, flags, 1, false);
    st = std::get<2>(res);
    TORCH_CHECK(!st.bitwise_and(EKS_STATUS_BAD_MODEL).ne(0).any().item<bool>(),
                "eks::nll: a model_flags promise does not hold");
    TORCH_CHECK(!st.ne(0).any().item<bool>(), "eks::nll: singular system (LinAlgError)");
  }
  return std::get<1>(res);
}
constexpr auto &nll_gpu = nll_op, &nll_meta = nll_op;

// posterior variances of smooth's output: var (B, T, n), Vs (B, T, r, r), status (B)
T3 smooth_var_op(const Tensor& obs, const Tensor& params, int64_t n, int64_t r) {
  const MemberIn in(obs, n);
  const int64_t B = in.B, T = in.T;
  Tensor var_tm = time_major(obs, in);
  Tensor Vs = at::empty({B, T, r, r}, f64(obs));
  Tensor status = at::empty({B}, i32(obs));
  if (!in.meta) {
    Tensor prm = param_rows(params, obs, B, in.n, r);
    Tensor ws = workspace(obs, eks_smooth_var_workspace_bytes(B, T, in.n, (int)r));
    check(eks_smooth_var(obs.data_ptr(), in.code, B, T, in.E, in.n, (int)r, obs.stride(0),
                         obs.stride(1), obs.stride(2), obs.stride(3), prm.data_ptr<double>(),
                         var_tm.data_ptr<double>(), n, B * n, 1, Vs.data_ptr<double>(),
                         ws.data_ptr(), (size_t)ws.numel(), status.data_ptr<int32_t>(),
                         cur_stream(obs)),
          "eks_smooth_var");
  }
  return {batch_major(var_tm), Vs, status};
}
constexpr auto &smooth_var_gpu = smooth_var_op, &smooth_var_meta = smooth_var_op;

// smoothing through missing observations (a non-finite ensemble average or
// variance): out, var (B, T, n), nll (B), nobs (B) int32, status (B)
T5 smooth_gaps_op(const Tensor& obs, const Tensor& params, int64_t n, int64_t r,
                  const std::string& mode) {
  const MemberIn in(obs, n);
  const int64_t B = in.B, T = in.T;
  Tensor out_tm = time_major(obs, in), var_tm = time_major(obs, in);
  Tensor nll = at::empty({B}, f64(obs));
  Tensor nobs = at::empty({B}, i32(obs));
  Tensor status = at::empty({B}, i32(obs));
  if (!in.meta) {
    Tensor prm = param_rows(params, obs, B, in.n, r);
    Tensor ws = workspace(obs, eks_smooth_gaps_workspace_bytes(B, T, in.n, (int)r));
    check(eks_smooth_gaps(obs.data_ptr(), in.code, B, T, in.E, in.n, (int)r, obs.stride(0),
                          obs.stride(1), obs.stride(2), obs.stride(3), mode_code(mode),
                          prm.data_ptr<double>(), out_tm.data_ptr<double>(), n, B * n, 1,
                          var_tm.data_ptr<double>(), nullptr, nullptr, nll.data_ptr<double>(),
                          nobs.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(),
                          status.data_ptr<int32_t>(), cur_stream(obs)),
          "eks_smooth_gaps");
  }
  return {batch_major(out_tm), batch_major(var_tm), nll, nobs, status};
}
constexpr auto &smooth_gaps_gpu = smooth_gaps_op, &smooth_gaps_meta = smooth_gaps_op;

// joint posterior draws through missing observations from the caller's noise
// (B, S, T, r): draws (B, S, T, n), latent (B, S, T, r), out (B, T, n), status (B)
T4 draws_gaps_op(const Tensor& obs, const Tensor& params, const Tensor& noise, int64_t n,
                 int64_t r, const std::string& mode) {
  const MemberIn in(obs, n);
  const int64_t B = in.B, T = in.T;
  if (!in.meta) {
    need_gpu(params, "params");
    need_gpu(noise, "noise");
    TORCH_CHECK(params.device() == obs.device() && noise.device() == obs.device(),
                "obs, params and noise must be on one device");
  }
  TORCH_CHECK(noise.dim() == 4 && noise.size(0) == B && noise.size(2) == T && noise.size(3) == r &&
                  noise.scalar_type() == at::kDouble,
              "noise must be a (", B, ", S, ", T, ", ", r, ") float64 tensor");
  const int64_t S = noise.size(1);
  Tensor draws_tm = at::empty({T, B, S, n}, f64(obs));  // time-major: coalesced stores
  Tensor latent = at::empty({B, S, T, r}, f64(obs));
  Tensor out_tm = time_major(obs, in);
  Tensor status = at::empty({B}, i32(obs));
  if (!in.meta) {
    Tensor z = noise.stride(3) == 1 ? noise : noise.contiguous();
    Tensor prm = param_rows(params, obs, B, in.n, r);
    Tensor ws = workspace(obs, eks_draws_gaps_workspace_bytes(B, S, T, in.n, (int)r));
    check(eks_draws_gaps(obs.data_ptr(), in.code, B, T, in.E, in.n, (int)r, obs.stride(0),
                         obs.stride(1), obs.stride(2), obs.stride(3), mode_code(mode),
                         prm.data_ptr<double>(), S, z.data_ptr<double>(), z.stride(0), z.stride(1),
                         z.stride(2), 0, draws_tm.data_ptr<double>(), S * n, n, B * S * n, 1,
                         latent.data_ptr<double>(), out_tm.data_ptr<double>(), n, B * n, 1, nullptr,
                         ws.data_ptr(), (size_t)ws.numel(), status.data_ptr<int32_t>(),
                         cur_stream(obs)),
          "eks_draws_gaps");
  }
  return {draws_tm.permute({1, 2, 0, 3}).contiguous(), latent, batch_major(out_tm), status};
}
constexpr auto &draws_gaps_gpu = draws_gaps_op, &draws_gaps_meta = draws_gaps_op;

// the noise a seeded eks_draws_gaps call generates, on `like`'s device: (B, S, T, r)
Tensor draws_noise_op(const Tensor& like, int64_t B, int64_t S, int64_t T, int64_t r,
                      int64_t seed) {
  if (!like.is_meta()) need_gpu(like, "like");
  TORCH_CHECK(B >= 0 && S >= 0 && T >= 0, "B, S, T must be >= 0");
  Tensor z = at::empty({B, S, T, r}, f64(like));
  if (like.is_meta()) return z;
  const c10::DeviceGuard g(like.device());
  check(eks_draws_noise(B, S, T, (int)r, (uint64_t)seed, z.data_ptr<double>(), S * T * r, T * r,
                        r, cur_stream(like)),
        "eks_draws_noise");
  return z;
}
constexpr auto &draws_noise_gpu = draws_noise_op, &draws_noise_meta = draws_noise_op;

// the NLL of K candidate models per trajectory: params (K * B, P), row
// k * B + b = candidate k of trajectory b -> nll (K, B), status (K, B)
T2 nll_sweep_op(const Tensor& obs, const Tensor& params, int64_t K, int64_t n, int64_t r,
                const std::string& mode) {
  const MemberIn in(obs, n);
  TORCH_CHECK(K >= 0, "K must be >= 0");
  const int64_t B = in.B, T = in.T;
  Tensor nll = at::empty({K, B}, f64(obs));
  Tensor status = at::zeros({K, B}, i32(obs));
  if (!in.meta) {
    Tensor prm = param_rows(params, obs, K * B, in.n, r);
    Tensor ws = workspace(obs, eks_nll_sweep_workspace_bytes(B, K, T, in.n, (int)r));
    check(eks_nll_sweep(obs.data_ptr(), in.code, B, T, in.E, in.n, (int)r, obs.stride(0),
                        obs.stride(1), obs.stride(2), obs.stride(3), mode_code(mode),
                        prm.data_ptr<double>(), K, nll.data_ptr<double>(), ws.data_ptr(),
                        (size_t)ws.numel(), status.data_ptr<int32_t>(), cur_stream(obs)),
          "eks_nll_sweep");
  }
  return {nll, status};
}
constexpr auto &nll_sweep_gpu = nll_sweep_op, &nll_sweep_meta = nll_sweep_op;

// nll_sweep through missing observations (eks_nll_sweep_gaps): the NLL over
// the observed entries -> nll (K, B), nobs (B), status (K, B)
T3 nll_sweep_gaps_op(const Tensor& obs, const Tensor& params, int64_t K, int64_t n, int64_t r,
                     const std::string& mode) {
  const MemberIn in(obs, n);
  TORCH_CHECK(K >= 0, "K must be >= 0");
  const int64_t B = in.B, T = in.T;
  Tensor nll = at::empty({K, B}, f64(obs));
  Tensor nobs = at::zeros({B}, i32(obs));
  Tensor status = at::zeros({K, B}, i32(obs));
  if (!in.meta) {
    Tensor prm = param_rows(params, obs, K * B, in.n, r);
    Tensor ws = workspace(obs, eks_nll_sweep_gaps_workspace_bytes(B, K, T, in.n, (int)r));
    check(eks_nll_sweep_gaps(obs.data_ptr(), in.code, B, T, in.E, in.n, (int)r, obs.stride(0),
                             obs.stride(1), obs.stride(2), obs.stride(3), mode_code(mode),
                             prm.data_ptr<double>(), K, nll.data_ptr<double>(),
                             nobs.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(),
                             status.data_ptr<int32_t>(), cur_stream(obs)),
          "eks_nll_sweep_gaps");
  }
  return {nll, nobs, status};
}
constexpr auto &nll_sweep_gaps_gpu = nll_sweep_gaps_op, &nll_sweep_gaps_meta = nll_sweep_gaps_op;

// --------------------------------------------------------------------- fit
T2 fit_op(const Tensor& obs, const std::string& kind, int64_t n, int64_t r, double smooth_param,
          double quantile_keep, const std::string& mode) {
  const MemberIn in(obs, n);
  const int64_t B = in.B, T = in.T;
  Tensor params = at::empty({B, eks_param_len(in.n, (int)r)}, f64(obs));
  Tensor status = at::empty({B}, i32(obs));
  if (!in.meta) {
    const int k = fit_kind(kind);
    Tensor ws = workspace(obs, eks_fit_workspace_bytes(B, T, in.n));
    check(eks_fit(obs.data_ptr(), in.code, B, T, in.E, in.n, (int)r, obs.stride(0), obs.stride(1),
                  obs.stride(2), obs.stride(3), mode_code(mode), k, smooth_param, quantile_keep,
                  params.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel(),
                  status.data_ptr<int32_t>(), nullptr, cur_stream(obs)),
          "eks_fit");
  }
  return {params, status};
}
constexpr auto &fit_gpu = fit_op, &fit_meta = fit_op;

// ---------------------------------------------------------------- fit_gaps
// (params, status, yev bytes, ncomplete, nkept); the planes in yev have the
// type eks_yev_dtype(obs dtype, E, mode) names
T5 fit_gaps_op(const Tensor& obs, const std::string& kind, int64_t n, int64_t r,
               double smooth_param, double quantile_keep, const std::string& mode) {
  const MemberIn in(obs, n);
  const int64_t B = in.B, T = in.T;
  const int m = mode_code(mode);
  Tensor params = at::empty({B, eks_param_len(in.n, (int)r)}, f64(obs));
  Tensor status = at::empty({B}, i32(obs));
  Tensor ncomplete = at::empty({B}, i32(obs));
  Tensor nkept = at::empty({B}, i32(obs));
  Tensor yev = bytes(obs, eks_yev_bytes(B, T, in.n, in.code, in.E, m));
  if (!in.meta && B > 0) {  // (an empty batch has no planes to point at)
    const int k = fit_kind(kind);
    Tensor ws = workspace(obs, eks_fit_gaps_workspace_bytes(B, T, in.n));
    check(eks_fit_gaps(obs.data_ptr(), in.code, B, T, in.E, in.n, (int)r, obs.stride(0),
                       obs.stride(1), obs.stride(2), obs.stride(3), m, k, smooth_param,
                       quantile_keep, params.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel(),
                       status.data_ptr<int32_t>(), yev.data_ptr(), ncomplete.data_ptr<int32_t>(),
                       nkept.data_ptr<int32_t>(), cur_stream(obs)),
          "eks_fit_gaps");
  }
  return {params, status, yev, ncomplete, nkept};
}
constexpr auto &fit_gaps_gpu = fit_gaps_op, &fit_gaps_meta = fit_gaps_op;

// ----------------------------------------------------------- ensemble_gaps
// (yev bytes: EKS_YEV64 planes; nvalid (T, n, B) uint8, the valid members of
// every column in the planes' layout)
T2 ensemble_gaps_op(const Tensor& obs, const std::string& mode, int64_t min_members) {
  const MemberIn in(obs);
  const int64_t B = in.B, T = in.T;
  const int m = mode_code(mode);
  Tensor yev = bytes(obs, eks_yev_bytes(B, T, in.n, EKS_F64, in.E, m));
  Tensor nvalid = at::empty({T, in.n, B}, obs.options().dtype(at::kByte));
  if (!in.meta) {
    TORCH_CHECK(min_members >= 1 && min_members <= in.E, "min_members must be in 1..E=", in.E);
    if (B > 0)  // (an empty batch has no planes to point at)
      check(eks_ensemble_gaps(obs.data_ptr(), in.code, B, T, in.E, in.n, obs.stride(0),
                              obs.stride(1), obs.stride(2), obs.stride(3), m, (int)min_members,
                              yev.data_ptr(), nvalid.data_ptr<uint8_t>(), cur_stream(obs)),
            "eks_ensemble_gaps");
  }
  return {yev, nvalid};
}
constexpr auto &ensemble_gaps_gpu = ensemble_gaps_op, &ensemble_gaps_meta = ensemble_gaps_op;

// --------------------------------------------------------------- fit_pupil
// (stats (B, 6), ncomplete, status, yev bytes: the EKS_YEV64 planes of
// eks_ensemble_gaps(min_members = E))
T4 fit_pupil_op(const Tensor& obs, const std::string& mode) {
  const MemberIn in(obs, 8);
  const int64_t B = in.B, T = in.T;
  const int m = mode_code(mode);
  Tensor stats = at::empty({B, 6}, f64(obs));
  Tensor ncomplete = at::empty({B}, i32(obs));
  Tensor status = at::empty({B}, i32(obs));
  Tensor yev = bytes(obs, eks_yev_bytes(B, T, 8, EKS_F64, in.E, m));
  if (!in.meta && B > 0) {  // (an empty batch has no planes to point at)
    Tensor ws = workspace(obs, eks_fit_pupil_workspace_bytes(B, T));
    check(eks_fit_pupil(obs.data_ptr(), in.code, B, T, in.E, 8, obs.stride(0), obs.stride(1),
                        obs.stride(2), obs.stride(3), m, stats.data_ptr<double>(),
                        ncomplete.data_ptr<int32_t>(), ws.data_ptr(), (size_t)ws.numel(),
                        status.data_ptr<int32_t>(), yev.data_ptr(), cur_stream(obs)),
          "eks_fit_pupil");
  }
  return {stats, ncomplete, status, yev};
}
constexpr auto &fit_pupil_gpu = fit_pupil_op, &fit_pupil_meta = fit_pupil_op;

// ---------------------------------------------------------- newton_filter
T2 newton_op(const Tensor& y, const Tensor& ev, const Tensor& mu0, const Tensor& S0,
             const Tensor& A, const Tensor& Bm, const Tensor& E, int64_t max_iter) {
  if (!y.is_meta()) need_gpu(y, "y");
  TORCH_CHECK(y.dim() == 3 && ev.sizes() == y.sizes(), "y and ev must both be (B, T, n)");
  TORCH_CHECK(mu0.dim() == 1 || mu0.dim() == 2, "mu0 must be (r,) or (B, r)");
  const int64_t B = y.size(0), T = y.size(1), n = y.size(2), r = mu0.size(-1);
  Tensor q = at::empty({B, T, r}, f64(y));
  Tensor status = at::zeros({B}, i32(y));
  if (y.is_meta()) return {q, status};
  const c10::DeviceGuard g(y.device());
  const bool sh = mu0.dim() == 1;
  check_shape(mu0, "mu0", sh, B, {r});
  check_shape(S0, "S0", sh, B, {r, r});
  check_shape(A, "A", sh, B, {r, r});
  check_shape(Bm, "B", sh, B, {n, r});
  check_shape(E, "E", sh, B, {r, r});
  Tensor y_ = contiguous_f64(y), ev_ = on_dev_f64(ev, y), mu0_ = on_dev_f64(mu0, y);
  Tensor S0_ = on_dev_f64(S0, y), A_ = on_dev_f64(A, y), B_ = on_dev_f64(Bm, y),
         E_ = on_dev_f64(E, y);
  check(eks_newton_filter(B, T, (int)n, (int)r, y_.data_ptr<double>(), ev_.data_ptr<double>(),
                          mu0_.data_ptr<double>(), S0_.data_ptr<double>(), A_.data_ptr<double>(),
                          B_.data_ptr<double>(), E_.data_ptr<double>(), sh ? 1 : 0, (int)max_iter,
                          q.data_ptr<double>(), status.data_ptr<int32_t>(), cur_stream(y)),
        "eks_newton_filter");
  return {q, status};
}
constexpr auto &newton_gpu = newton_op, &newton_meta = newton_op;

// --------------------------------------------------------------- interp1d
Tensor interp_op(const Tensor& x, const Tensor& y, const Tensor& xq) {
  if (!x.is_meta()) need_gpu(x, "x");
  TORCH_CHECK(y.dim() == 2 && x.dim() == 1 && xq.dim() == 1 && y.size(0) == x.size(0),
              "x (n,), y (n, C), xq (q,)");
  const int64_t n = x.size(0), C = y.size(1), q = xq.size(0);
  Tensor out = at::empty({q, C}, f64(x));
  if (x.is_meta()) return out;
  const c10::DeviceGuard g(x.device());
  Tensor x_ = contiguous_f64(x), y_ = y.to(x.device(), at::kDouble), xq_ = on_dev_f64(xq, x);
  Tensor status = at::zeros({q}, i32(x));
  check(eks_interp1d(x_.data_ptr<double>(), n, y_.data_ptr<double>(), C, y_.stride(0),
                     y_.stride(1), xq_.data_ptr<double>(), q, out.data_ptr<double>(), out.stride(0),
                     out.stride(1), status.data_ptr<int32_t>(), cur_stream(x)),
        "eks_interp1d");
  TORCH_CHECK(!status.ne(0).any().item<bool>(),
              "A value in x_new is outside the interpolation range.");
  return out;
}
constexpr auto &interp_gpu = interp_op, &interp_meta = interp_op;

}  // namespace

TORCH_LIBRARY(eks, m) {
  m.def("ensemble(Tensor obs, str mode) -> (Tensor, Tensor)");
  m.def("forward(Tensor y, Tensor ev, Tensor m0, Tensor S0, Tensor A, Tensor Q, Tensor C) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("backward(Tensor mf, Tensor Vf, Tensor S, Tensor A) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("smooth(Tensor obs, Tensor params, int n, int r, str mode, int flags, int algo) -> "
        "(Tensor, Tensor)");
  m.def("smooth_var(Tensor obs, Tensor params, int n, int r) -> (Tensor, Tensor, Tensor)");
  m.def("smooth_gaps(Tensor obs, Tensor params, int n, int r, str mode) -> "
        "(Tensor out, Tensor var, Tensor nll, Tensor nobs, Tensor status)");
  m.def("draws_gaps(Tensor obs, Tensor params, Tensor noise, int n, int r, str mode) -> "
        "(Tensor draws, Tensor latent, Tensor out, Tensor status)");
  m.def("draws_noise(Tensor like, int B, int S, int T, int r, int seed) -> Tensor");
  m.def("nll(Tensor obs, Tensor params, int n, int r, str mode, int flags) -> Tensor");
  m.def("nll_sweep(Tensor obs, Tensor params, int K, int n, int r, str mode) -> (Tensor, Tensor)");
  m.def("nll_sweep_gaps(Tensor obs, Tensor params, int K, int n, int r, str mode) -> "
        "(Tensor, Tensor, Tensor)");
  m.def("fit(Tensor obs, str kind, int n, int r, float smooth_param, float quantile_keep, "
        "str mode) -> (Tensor, Tensor)");
  m.def("fit_gaps(Tensor obs, str kind, int n, int r, float smooth_param, float quantile_keep, "
        "str mode) -> (Tensor params, Tensor status, Tensor yev, Tensor ncomplete, Tensor nkept)");
  m.def("ensemble_gaps(Tensor obs, str mode, int min_members) -> (Tensor, Tensor)");
  m.def("fit_pupil(Tensor obs, str mode) -> "
        "(Tensor stats, Tensor ncomplete, Tensor status, Tensor yev)");
  m.def("newton_filter(Tensor y, Tensor ev, Tensor mu0, Tensor S0, Tensor A, Tensor Bm, "
        "Tensor E, int max_iter) -> (Tensor, Tensor)");
  m.def("interp1d(Tensor x, Tensor y, Tensor xq) -> Tensor");
}

TORCH_LIBRARY_IMPL(eks, CUDA, m) {
  m.impl("ensemble", &ensemble_gpu);
  m.impl("forward", &forward_gpu);
  m.impl("backward", &backward_gpu);
  m.impl("smooth", &smooth_gpu);
  m.impl("smooth_var", &smooth_var_gpu);
  m.impl("smooth_gaps", &smooth_gaps_gpu);
  m.impl("draws_gaps", &draws_gaps_gpu);
  m.impl("draws_noise", &draws_noise_gpu);
  m.impl("nll", &nll_gpu);
  m.impl("nll_sweep", &nll_sweep_gpu);
  m.impl("nll_sweep_gaps", &nll_sweep_gaps_gpu);
  m.impl("fit", &fit_gpu);
  m.impl("fit_gaps", &fit_gaps_gpu);
  m.impl("ensemble_gaps", &ensemble_gaps_gpu);
  m.impl("fit_pupil", &fit_pupil_gpu);
  m.impl("newton_filter", &newton_gpu);
  m.impl("interp1d", &interp_gpu);
}

TORCH_LIBRARY_IMPL(eks, Meta, m) {
  m.impl("ensemble", &ensemble_meta);
  m.impl("forward", &forward_meta);
  m.impl("backward", &backward_meta);
  m.impl("smooth", &smooth_meta);
  m.impl("smooth_var", &smooth_var_meta);
  m.impl("smooth_gaps", &smooth_gaps_meta);
  m.impl("draws_gaps", &draws_gaps_meta);
  m.impl("draws_noise", &draws_noise_meta);
  m.impl("nll", &nll_meta);
  m.impl("nll_sweep", &nll_sweep_meta);
  m.impl("nll_sweep_gaps", &nll_sweep_gaps_meta);
  m.impl("fit", &fit_meta);
  m.impl("fit_gaps", &fit_gaps_meta);
  m.impl("ensemble_gaps", &ensemble_gaps_meta);
  m.impl("fit_pupil", &fit_pupil_meta);
  m.impl("newton_filter", &newton_meta);
  m.impl("interp1d", &interp_meta);
}
