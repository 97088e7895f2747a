// Host-only check of eks_nll_sweep's workspace plan (nll_sweep.hpp): over a
// sweep of (B, K, T, r) and forced chunk lengths, every array's offset plus
// extent lies inside the reported workspace size, the arrays do not overlap,
// the total is the documented formula, the chunk grid covers T, and the last
// index each kernel touches (the last step's last plane of the last
// trajectory; the last chunk's constant of the last row) is inside its array.
// No kernel is launched.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/sweep_plan_check.hip -o sweep_plan_check && ./sweep_plan_check
#include <cstdio>

#include "../eks_amd/csrc/nll_sweep.hpp"

namespace eks {
long long g_sweep_chunk = 0;
}

using namespace eks;

static int fails = 0;
#define CHECK(c)                                                                          \
  do {                                                                                    \
    if (!(c)) {                                                                           \
      ++fails;                                                                            \
      std::printf("FAIL %s (B=%lld K=%lld T=%lld r=%d forced=%lld)\n", #c, B, K, T, r, forced); \
    }                                                                                     \
  } while (0)

int main() {
  const long long Bs[] = {1, 2, 3, 17, 63, 64, 65, 255, 256, 257, 300, 480, 2176, 17408};
  const long long Ks[] = {1, 2, 7, 9, 16, 100};
  const long long Ts[] = {1, 2, 7, 8, 9, 64, 131, 2100, 10000, 100000, 1000000};
  const long long forceds[] = {0, 1, 8, 13, 136, 1 << 20};
  long long n_plans = 0;
  for (long long forced : forceds)
    for (long long B : Bs)
      for (long long K : Ks)
        for (long long T : Ts)
          for (int r = 2; r <= 3; ++r) {
            if ((double)B * (double)K * (double)T > 4e9) continue;
            g_sweep_chunk = forced;
            const long long L = sw_chunk_len(B, T, r);
            const SwPlan p = sw_make_plan(B, K, T, r, L);
            ++n_plans;
            const size_t NP = (size_t)sw_row_len(r), EL1 = (size_t)elem_len(r) + 1;
            const size_t Bz = (size_t)B, KB = (size_t)(K * B);
            CHECK(NP == (r == 2 ? 5u : 9u) && EL1 == (r == 2 ? 15u : 28u));
            CHECK(L >= 8 && L % 8 == 0);
            CHECK(p.NC >= 1 && p.NC * L >= T && (p.NC - 1) * L < T);
            if (forced >= 8 && forced % 8 == 0 && forced < T) CHECK(L == forced);
            // offset and extent in doubles, in the order the plan lays them out
            const size_t off[] = {p.row_off, p.elem_off, p.kap_off};
            const size_t ext[] = {(size_t)T * NP * Bz, (size_t)p.NC * EL1 * KB, (size_t)p.NC * Bz};
            size_t end = 0, sum = 0;
            for (int i = 0; i < 3; ++i) {
              CHECK(off[i] % 256 == 0);
              CHECK(off[i] >= end);  // no overlap with the array before
              end = off[i] + ext[i] * 8;
              CHECK(end <= p.total);
              sum += align256(ext[i] * 8);
            }
            CHECK(sum == p.total);
            // the last elements the kernels address
            const size_t last_row = ((size_t)(T - 1) * NP + (NP - 1)) * Bz + (Bz - 1);
            const size_t last_elem = ((size_t)(p.NC - 1) * EL1 + (EL1 - 1)) * KB + (KB - 1);
            const size_t last_kap = (size_t)(p.NC - 1) * Bz + (Bz - 1);
            CHECK(p.row_off + (last_row + 1) * 8 <= p.elem_off);
            CHECK(p.elem_off + (last_elem + 1) * 8 <= p.kap_off);
            CHECK(p.kap_off + (last_kap + 1) * 8 <= p.total);
            // 32-bit per-lane byte offsets within a plane
            CHECK(KB * 8 < (1ull << 32));
          }
  std::printf("%lld plans checked, %d failure(s)\n", n_plans, fails);
  return fails ? 1 : 0;
}
