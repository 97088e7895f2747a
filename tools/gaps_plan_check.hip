// Host-only check of eks_smooth_gaps's workspace plan (gap_smooth.hpp): over a
// sweep of (B, T, r) and forced chunk lengths, every array's offset plus
// extent lies inside the reported workspace size, the arrays do not overlap,
// the total is the documented formula, the chunk grid covers T, and the last
// index each kernel touches (the last step's last plane of the last
// trajectory; the last chunk's last plane) is inside its array.  No kernel is
// launched.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/gaps_plan_check.hip -o gaps_plan_check && ./gaps_plan_check
#include <cstdio>

#include "../eks_amd/csrc/gap_smooth.hpp"

namespace eks {
long long g_pvar_chunk = 0;
long long g_gaps_chunk = 0;
}  // namespace eks

using namespace eks;

static int fails = 0;
#define CHECK(c)                                                                      \
  do {                                                                                \
    if (!(c)) {                                                                       \
      ++fails;                                                                        \
      std::printf("FAIL %s (B=%lld T=%lld r=%d forced=%lld)\n", #c, B, T, r, forced); \
    }                                                                                 \
  } while (0)

int main() {
  const long long Bs[] = {1, 2, 3, 17, 63, 64, 65, 255, 256, 257, 300, 480, 2176, 17408};
  const long long Ts[] = {1, 2, 7, 8, 9, 64, 131, 2100, 10000, 100000, 1000000};
  const long long forceds[] = {0, 1, 8, 13, 136, 1 << 20};
  long long n_plans = 0;
  for (long long forced : forceds)
    for (long long B : Bs)
      for (long long T : Ts)
        for (int r = 2; r <= 3; ++r) {
          if ((double)B * (double)T > 4e9) continue;
          g_gaps_chunk = forced;
          const long long L = gp_chunk_len(B, T, r);
          const GpPlan p = gp_make_plan(B, T, r, L);
          ++n_plans;
          const size_t S = (size_t)pv_sym_len(r), R = (size_t)r, Bz = (size_t)B;
          const size_t NC = (size_t)p.NC, Tz = (size_t)T;
          const size_t EL = (size_t)elem_len(r), ML = (size_t)gp_map_len(r);
          CHECK(EL == (r == 2 ? 14u : 27u) && ML == (r == 2 ? 13u : 27u));
          CHECK(EL == (r == 2 ? (size_t)Elem<2>::len : (size_t)Elem<3>::len));
          CHECK(ML == (r == 2 ? (size_t)GapMap<2>::len : (size_t)GapMap<3>::len));
          CHECK(L >= 8 && L % 8 == 0);
          CHECK(p.NC >= 1 && p.NC * L >= T && (p.NC - 1) * L < T);
          if (forced >= 8 && forced % 8 == 0 && forced < T) CHECK(L == forced);
          // offset, planes and bytes per value, in the order the plan lays them out
          const size_t off[] = {p.w_off,   p.sw_off,  p.kap_off, p.m_off,   p.p_off,  p.elem_off,
                                p.sin_off, p.map_off, p.bin_off, p.nll_off, p.cnt_off};
          const size_t planes[] = {Tz * S,  Tz * R,  Tz,           Tz * R, Tz * S, NC * EL,
                                   NC * (R + S), NC * ML, NC * (R + S), NC,     NC};
          const size_t bytes[] = {8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 4};
          size_t end = 0, sum = 0, per_step = 0;
          for (int i = 0; i < 11; ++i) {
            CHECK(off[i] % 256 == 0);
            CHECK(off[i] >= end);  // no overlap with the array before
            // the last value a kernel addresses: the last plane, the last trajectory
            const size_t last = (planes[i] - 1) * Bz + (Bz - 1);
            end = off[i] + planes[i] * Bz * bytes[i];
            CHECK(off[i] + (last + 1) * bytes[i] == end);
            CHECK(end <= p.total);
            CHECK(end <= (i + 1 < 11 ? off[i + 1] : p.total));
            sum += align256(planes[i] * Bz * bytes[i]);
            if (i < 5) per_step += planes[i] / Tz;
          }
          CHECK(sum == p.total);
          CHECK(per_step == 2 * S + 2 * R + 1);  // T (2 Sym + 2 r + 1) doubles per trajectory
          CHECK(p.total >= Tz * Bz * per_step * 8);
          // 32-bit per-lane byte offsets within a plane
          CHECK(Bz * 8 < (1ull << 32));
        }
  g_gaps_chunk = 0;
  std::printf("%lld plans checked, %d failure(s)\n", n_plans, fails);
  return fails ? 1 : 0;
}
