// Host-only check of eks_nll_sweep_gaps's workspace plan (gap_sweep.hpp): over
// a sweep of (B, T, r), K in {1, 7, 64} and forced chunk lengths, every
// array's offset plus extent lies inside the reported workspace size, the
// arrays are 256-byte aligned and do not overlap, their sizes sum to the
// reported total, the chunk grid covers T, and the last index each kernel
// touches (the last plane of the last trajectory or row) is inside its array.
// No kernel is launched.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/gaps_sweep_plan_check.hip -o gaps_sweep_plan_check && ./gaps_sweep_plan_check
#include <cstdio>

#include "../eks_amd/csrc/gap_sweep.hpp"

namespace eks {
long long g_pvar_chunk = 0;
long long g_gaps_chunk = 0;
long long g_sweep_chunk = 0;
long long g_gaps_sweep_chunk = 0;
}  // namespace eks

using namespace eks;

static int fails = 0;
#define CHECK(c)                                                                        \
  do {                                                                                  \
    if (!(c)) {                                                                         \
      ++fails;                                                                          \
      std::printf("FAIL %s (B=%lld K=%lld T=%lld r=%d forced=%lld)\n", #c, B, K, T, r,  \
                  forced);                                                              \
    }                                                                                   \
  } while (0)

int main() {
  const long long Bs[] = {1, 2, 3, 17, 63, 64, 65, 255, 256, 257, 300, 480, 2176, 17408};
  const long long Ts[] = {1, 2, 7, 8, 9, 64, 131, 2100, 10000, 100000, 1000000};
  const long long Ks[] = {1, 7, 64};
  const long long forceds[] = {0, 1, 8, 13, 136, 1 << 20};
  long long n_plans = 0;
  for (long long forced : forceds)
    for (long long K : Ks)
      for (long long B : Bs)
        for (long long T : Ts)
          for (int r = 2; r <= 3; ++r) {
            if ((double)B * (double)T > 4e9) continue;
            g_gaps_sweep_chunk = forced;
            const long long L = gs_chunk_len(B, T, r);
            const GsPlan p = gs_make_plan(B, K, T, r, L);
            ++n_plans;
            const size_t S = (size_t)pv_sym_len(r), R = (size_t)r, Bz = (size_t)B;
            const size_t KB = (size_t)(K * B), NC = (size_t)p.NC, Tz = (size_t)T;
            const size_t EL = (size_t)elem_len(r);
            CHECK(EL == (r == 2 ? (size_t)Elem<2>::len : (size_t)Elem<3>::len));
            CHECK(S == (r == 2 ? (size_t)Sym<2>::len : (size_t)Sym<3>::len));
            CHECK(L >= 8 && L % 8 == 0);
            CHECK(p.L == L && p.NC >= 1 && p.NC * L >= T && (p.NC - 1) * L < T);
            if (forced >= 8 && forced % 8 == 0 && forced < T) CHECK(L == forced);
            // offset, planes, values per plane and bytes per value, in the plan's order
            const size_t off[] = {p.w_off,   p.sw_off,  p.kap_off, p.elem_off,
                                  p.sin_off, p.nll_off, p.cnt_off};
            const size_t planes[] = {Tz * S, Tz * R, Tz, NC * EL, NC * (R + S), NC, NC};
            const size_t width[] = {Bz, Bz, Bz, KB, KB, KB, Bz};
            const size_t bytes[] = {8, 8, 8, 8, 8, 8, 4};
            size_t end = 0, sum = 0, per_step = 0;
            for (int i = 0; i < 7; ++i) {
              CHECK(off[i] % 256 == 0);
              CHECK(off[i] >= end);  // no overlap with the array before
              // the last value a kernel addresses: the last plane, the last trajectory / row
              const size_t last = (planes[i] - 1) * width[i] + (width[i] - 1);
              end = off[i] + planes[i] * width[i] * bytes[i];
              CHECK(off[i] + (last + 1) * bytes[i] == end);
              CHECK(end <= p.total);
              CHECK(end <= (i + 1 < 7 ? off[i + 1] : p.total));
              sum += align256(planes[i] * width[i] * bytes[i]);
              if (i < 3) per_step += planes[i] / Tz;
            }
            CHECK(sum == p.total);
            CHECK(per_step == S + R + 1);  // T (Sym + r + 1) doubles per trajectory
            CHECK(p.total >= Tz * Bz * per_step * 8);
            // 32-bit per-lane byte offsets within a plane of K * B rows
            CHECK(KB * 8 < (1ull << 32));
          }
  g_gaps_sweep_chunk = 0;
  std::printf("%lld plans checked, %d failure(s)\n", n_plans, fails);
  return fails ? 1 : 0;
}
