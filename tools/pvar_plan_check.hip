// Host-only check of eks_smooth_var's workspace plan (post_var.hpp): over a
// sweep of (B, T, r) and forced chunk lengths, every plane array's offset
// plus extent lies inside the reported workspace size, the arrays do not
// overlap, and the chunk grid covers T.  No kernel is launched.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/pvar_plan_check.hip -o pvar_plan_check && ./pvar_plan_check
#include <cstdio>

#include "../eks_amd/csrc/post_var.hpp"

namespace eks {
long long g_pvar_chunk = 0;
}

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
  const long long Bs[] = {1, 2, 3, 17, 63, 64, 65, 255, 256, 257, 300, 480, 2176, 17408, 1 << 20};
  const long long Ts[] = {1, 2, 7, 8, 9, 64, 131, 2100, 10000, 100000, 1000000};
  const long long forceds[] = {0, 1, 8, 13, 136, 1 << 20};
  long long n_plans = 0;
  for (long long forced : forceds)
    for (long long B : Bs)
      for (long long T : Ts)
        for (int r = 2; r <= 3; ++r) {
          if ((double)B * (double)T > 4e9) continue;
          g_pvar_chunk = forced;
          const long long L = pv_chunk_len(B, T, r);
          const PvPlan p = pv_make_plan(B, T, r, L);
          ++n_plans;
          const size_t S = (size_t)pv_sym_len(r), RR = (size_t)r * r, Bz = (size_t)B;
          CHECK(L >= 8 && L % 8 == 0);
          CHECK(p.NC >= 1 && p.NC * L >= T && (p.NC - 1) * L < T);
          if (forced >= 8 && forced % 8 == 0 && forced < T) CHECK(L == forced);
          // offset, doubles per trajectory: in the order the plan lays them out
          const size_t off[] = {p.w_off, p.p_off, p.elem_off, p.pin_off, p.map_off, p.vin_off};
          const size_t ext[] = {(size_t)T * S,        (size_t)T * S,       (size_t)p.NC * (RR + 2 * S),
                                (size_t)p.NC * S,     (size_t)p.NC * (RR + S), (size_t)p.NC * S};
          size_t end = 0;
          for (int i = 0; i < 6; ++i) {
            CHECK(off[i] % 256 == 0);
            CHECK(off[i] >= end);  // no overlap with the array before
            end = off[i] + ext[i] * Bz * 8;
            CHECK(end <= p.total);
          }
        }
  std::printf("%lld plans checked, %d failure(s)\n", n_plans, fails);
  return fails ? 1 : 0;
}
