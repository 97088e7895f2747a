// Host-only check of eks_fit_pupil's launch geometry and workspace arithmetic
// (eks_amd/csrc/pupil_fit.hpp): over B in {0, 1, 63, 64, 65, 1023} and T in
// {2, 63, 64, 65, 1 000 003} every frame belongs to exactly one (lane or
// block, partial), the grid covers every partial, the last partial a kernel
// writes or k_pupil_final reads lies inside the workspace, the plan's size is
// what eks_fit_pupil_workspace_bytes reports, and a workspace one byte short
// is refused before any launch.  No kernel is launched.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/pupil_fit_plan_check.hip eks_amd/csrc/eks_fit_pupil.hip \
//         -o pupil_fit_plan_check && ./pupil_fit_plan_check
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../eks_amd/csrc/eks_common.hpp"
#include "../eks_amd/csrc/pupil_fit.hpp"
#include "../include/eks_hip.h"

// the library's error text and launch bookkeeping (eks_kernels.hip), so that
// eks_fit_pupil.hip links alone: the checks below never reach a launch
namespace eks {
static std::string g_err;
int set_err(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
void clear_err() { g_err.clear(); }
int check_launch(const char *what) { return set_err(EKS_ERR_HIP, "%s: launched", what); }
void prof_mark(hipStream_t, const char *) {}
void prof_call_begin() {}
void prof_call_end(hipStream_t) {}
}  // namespace eks
extern "C" const char *eks_last_error(void) { return eks::g_err.c_str(); }

using namespace eks;

static int fails = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      ++fails;                                                            \
      std::printf("FAIL %s (B=%lld T=%lld)\n", #c, B, T);                 \
    }                                                                     \
  } while (0)

int main() {
  const long long Bs[] = {0, 1, 63, 64, 65, 1023};
  const long long Ts[] = {2, 63, 64, 65, 1000003};
  long long n_plans = 0;
  for (long long B : Bs)
    for (long long T : Ts) {
      const PupilPlan p = pupil_plan(B, T);
      const size_t reported = eks_fit_pupil_workspace_bytes(B, T);
      ++n_plans;
      if (B == 0) {
        CHECK(!p.ok && reported == 0);
        // no trajectories: EKS_OK, nothing launched, nothing dereferenced
        double dummy[8];
        int32_t idummy[2];
        CHECK(eks_fit_pupil(dummy, EKS_F32, 0, T, 5, 8, 0, 0, 0, 0, EKS_MEDIAN, dummy, idummy, dummy,
                            0, idummy, nullptr, nullptr) == EKS_OK);
        continue;
      }
      CHECK(p.ok);
      CHECK(reported == p.part_bytes && reported > 0);
      CHECK(p.frames_map == (B < kPupilFramesBelowB));
      CHECK(p.seg >= 1 && p.NP >= 1);
      CHECK(p.NP * p.seg >= T && (p.NP - 1) * p.seg < T);  // the partials tile [0, T)
      // every frame is summed exactly once
      std::vector<unsigned char> seen((size_t)T, 0);
      long long partials_written = 0, last_index = -1;
      if (p.frames_map) {
        CHECK(p.seg % kPupilBlk == 0 && p.seg / kPupilBlk <= kPupilMaxLaneFrames);
        CHECK(p.gx == p.NP && p.gy == B);
        for (long long blk = 0; blk < p.gx; ++blk) {
          const long long s0 = blk * p.seg, t1 = s0 + p.seg < T ? s0 + p.seg : T;
          for (int tid = 0; tid < kPupilBlk; ++tid)
            for (long long t = s0 + tid; t < t1; t += kPupilBlk) ++seen[(size_t)t];
          ++partials_written;
        }
        // the last value thread 0 of the last block stores
        last_index = ((p.NP - 1) * kPupilPartW + (kPupilPartW - 2)) * B + (B - 1);
      } else {
        CHECK(p.seg == kPupilLaneFrames && p.gy == 1);
        const long long lanes = p.gx * kPupilBlk;
        CHECK(lanes >= B * p.NP && lanes - kPupilBlk < B * p.NP);
        for (long long lane = 0; lane < lanes; lane += B) {  // (trajectory 0 of every chunk)
          if (lane >= B * p.NP) break;
          const long long pp = lane / B, t0 = pp * p.seg, t1 = t0 + p.seg < T ? t0 + p.seg : T;
          CHECK(lane % B == 0 && t0 < T);
          for (long long t = t0; t < t1; ++t) ++seen[(size_t)t];
          ++partials_written;
        }
        const long long lane = B * p.NP - 1;  // the last active lane
        last_index = ((lane / B) * kPupilPartW + (kPupilPartW - 2)) * B + lane % B;
      }
      bool once = true;
      for (long long t = 0; t < T; ++t) once = once && seen[(size_t)t] == 1;
      CHECK(once);
      CHECK(partials_written == p.NP);
      // the partials fit the workspace the query reports
      CHECK((size_t)(last_index + 1) * sizeof(double) <= reported);
      CHECK((size_t)p.NP * (size_t)B * kPupilPartW * sizeof(double) == reported);
      // a workspace one byte short (and the other argument errors) never reach a launch
      double dummy[8];
      int32_t idummy[2];
      CHECK(eks_fit_pupil(dummy, EKS_F32, B, T, 5, 8, 0, 0, 0, 0, EKS_MEDIAN, dummy, idummy, dummy,
                          reported - 1, idummy, nullptr, nullptr) == EKS_ERR_ARG);
      CHECK(std::strstr(eks_last_error(), "eks_fit_pupil") != nullptr);
      CHECK(eks_fit_pupil(dummy, EKS_F32, B, T, 5, 2, 0, 0, 0, 0, EKS_MEDIAN, dummy, idummy, dummy,
                          reported, idummy, nullptr, nullptr) == EKS_ERR_UNSUPPORTED);
      CHECK(eks_fit_pupil(dummy, EKS_YEV64, B, T, 5, 8, 0, 0, 0, 0, EKS_MEDIAN, dummy, idummy,
                          dummy, reported, idummy, dummy, nullptr) == EKS_ERR_ARG);
    }
  // below T = 2 there is nothing to fit
  {
    const long long B = 3, T = 1;
    CHECK(eks_fit_pupil_workspace_bytes(B, T) == 0 && !pupil_plan(B, T).ok);
  }
  std::printf("%lld plans checked, %d failure(s)\n", n_plans, fails);
  return fails ? 1 : 0;
}
