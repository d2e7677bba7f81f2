// sanitize_given_main.cpp -- a stand-alone program over the host DEBUGGING build of champ_given (the title odds by
// finishing position of mcgp_run_championship_live), for the host's sanitizers (not product code).  Compiled together
// with the standings driver of this directory:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
//       -static-libubsan -pthread -Itools/emu tools/emu/sanitize_given_main.cpp tools/emu/emu_champ.cpp -o san_given
//
// emu_champ_given_run (champ_accumulate and champ_given in blocks of 256 real threads) on seasons of every field size,
// the given race first, middle and last, with the table in LDS and by global atomics, in buffers of exactly their size
// (the kept orders of a chunk, the dynamic LDS and the output table), through one block and several, one chunk and three,
// and a key stride above the simulation count.  Exit status 0 and "ok" when every call returned MCGP_OK, every table sums
// to simulations x n and the sanitizers found nothing.  tests/test_champ_given_sanitize.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/mcgp.h"

extern "C" int emu_champ_given_run(uint32_t n_races, uint32_t n, uint64_t n_sims, uint64_t cap, const uint8_t *orders,
                                   const int32_t *points, const uint8_t *countback, const int32_t *init_points,
                                   const int32_t *init_counts, const int32_t *team, uint32_t n_teams, uint32_t given_race,
                                   uint32_t table_in_lds, uint32_t acc_grid, uint32_t given_grid,
                                   unsigned long long *given_out, uint32_t *info_out, const char **err);
extern "C" void emu_champ_shutdown();

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

}  // namespace

int main()
{
    const uint32_t R = 3;
    for (uint32_t n = 1; n <= 32; ++n) {
        for (int shape = 0; shape < 4; ++shape) {
            const uint64_t sims = shape == 0 ? 1 : shape == 1 ? 300 : shape == 2 ? 641 : 65;
            const uint64_t cap = shape == 2 ? 256 : shape == 3 ? 100 : sims;
            const uint32_t grid = shape == 1 ? 1 : 1u << 20;
            const uint32_t given = (n + (uint32_t)shape) % R, in_lds = (n + (uint32_t)shape / 2) & 1u;
            // every buffer on the heap at exactly its size
            std::unique_ptr<uint8_t[]> orders(new uint8_t[R * sims * n]);
            for (uint32_t r = 0; r < R; ++r)
                for (uint64_t s = 0; s < sims; ++s) {
                    uint8_t *o = orders.get() + (r * sims + s) * n;
                    for (uint32_t p = 0; p < n; ++p) o[p] = (uint8_t)p;
                    for (uint32_t p = n; p-- > 1;) std::swap(o[p], o[next_u32() % (p + 1)]);
                }
            std::vector<int32_t> points(R * n, 0), ip(n), ic((size_t)n * n, 29), team(n, 0);
            for (uint32_t r = 0; r < R; ++r)
                for (uint32_t p = 0; p < n && p < 3; ++p) points[r * n + p] = 5 - 2 * (int32_t)p;
            for (uint32_t d = 0; d < n; ++d) ip[d] = 65535 - 15 - (int32_t)(next_u32() % 3);   // the champion may end on 65 535
            const uint8_t cb[R] = {1, 0, 1};
            std::unique_ptr<unsigned long long[]> table(new unsigned long long[(size_t)n * n * n]());
            const char *err = "";
            const int rc = emu_champ_given_run(R, n, sims, cap, orders.get(), points.data(), cb, ip.data(), ic.data(),
                                               team.data(), 1, given, in_lds, grid, grid, table.get(), nullptr, &err);
            if (rc != MCGP_OK) {
                std::fprintf(stderr, "n = %u, shape %d: rc %d: %s\n", n, shape, rc, err);
                return 1;
            }
            unsigned long long total = 0;
            for (size_t i = 0; i < (size_t)n * n * n; ++i) total += table[i];
            if (total != sims * n) {
                std::fprintf(stderr, "n = %u, shape %d: the table sums to %llu, not %llu\n", n, shape, total,
                             (unsigned long long)(sims * n));
                return 1;
            }
        }
    }
    emu_champ_shutdown();
    std::puts("ok");
    return 0;
}
