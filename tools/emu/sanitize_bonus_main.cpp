// sanitize_bonus_main.cpp -- a stand-alone program over the host DEBUGGING builds of the fastest-lap bonus kernels, for
// the host's sanitizers (not product code).  Compiled together with one of the two drivers of this directory:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
//       -static-libubsan -pthread -Itools/emu \
//       -DSANITIZE_CHAMP tools/emu/sanitize_bonus_main.cpp tools/emu/emu_champ.cpp -o san_champ
//   g++ ... -fno-sanitize=alignment -ffp-contract=off -DSANITIZE_FASTEST tools/emu/sanitize_bonus_main.cpp \
//       tools/emu/emu_generic.cpp -o san_fastest
//
// (-fno-sanitize=alignment for the second only: emu_generic.cpp runs a block of ONE thread, and the lane's u16 `out` row
// follows n x blockDim.x bytes of `ord` in LDS, which is odd for an odd field there and a multiple of 64 on the device.)
// SANITIZE_CHAMP: emu_champ_bonus_run (champ_accumulate and champ_bonus in blocks of 256 real threads) on seasons of
// every field size, in buffers of exactly the chunk's size, through one block and several, one chunk and three.
// SANITIZE_FASTEST: emu_fastest_run (race_fastest_kernel) on fields of 1, 2, 20 and 32 cars and a race of one lap, the
// outputs in buffers of exactly n_sims entries.  Exit status 0 and "ok" when every call returned MCGP_OK and the
// sanitizers found nothing.  tests/test_fastest_sanitize.py builds and runs both.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/mcgp.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

}  // namespace

#ifdef SANITIZE_CHAMP
extern "C" int emu_champ_bonus_run(uint32_t n_races, uint32_t n, uint64_t n_sims, uint64_t cap, const uint8_t *orders,
                                   const int32_t *points, const uint8_t *countback, const int32_t *init_points,
                                   const int32_t *init_counts, const int32_t *team, uint32_t n_teams,
                                   const int32_t *bonus_points, const int32_t *bonus_within, const uint8_t *fl_driver,
                                   const uint8_t *fl_pos, uint32_t acc_grid, uint64_t *keys_out,
                                   unsigned long long *bonus_hist, unsigned long long *fastest_hist, uint32_t *info_out,
                                   const char **err);
extern "C" void emu_champ_shutdown();

int main()
{
    const uint32_t R = 3;
    for (uint32_t n = 1; n <= 32; ++n) {
        for (int shape = 0; shape < 3; ++shape) {
            const uint64_t sims = shape == 0 ? 1 : shape == 1 ? 300 : 641;
            const uint64_t cap = shape == 2 ? 256 : sims;
            const uint32_t grid = shape == 1 ? 1 : 1u << 20;
            const uint32_t T = n < 3 ? n : 3, words = (16 + 5 * n + 63) / 64;
            // every buffer on the heap at exactly its size
            std::unique_ptr<uint8_t[]> orders(new uint8_t[R * sims * n]), fd(new uint8_t[R * sims]), fp(new uint8_t[R * sims]);
            for (uint32_t r = 0; r < R; ++r)
                for (uint64_t s = 0; s < sims; ++s) {
                    uint8_t *o = orders.get() + (r * sims + s) * n;
                    for (uint32_t p = 0; p < n; ++p) o[p] = (uint8_t)p;
                    for (uint32_t p = n; p-- > 1;) std::swap(o[p], o[next_u32() % (p + 1)]);
                    const bool none = next_u32() % 8 == 0;
                    const uint32_t pos = next_u32() % n;
                    fd[r * sims + s] = none ? 0xFF : o[pos];
                    fp[r * sims + s] = none ? 0xFF : (uint8_t)pos;
                }
            std::vector<int32_t> points(R * n, 0), ip(n), ic((size_t)n * n, 28), team(n);
            for (uint32_t r = 0; r < R; ++r)
                for (uint32_t p = 0; p < n && p < 3; ++p) points[r * n + p] = 5 - 2 * (int32_t)p;
            for (uint32_t d = 0; d < n; ++d) {
                ip[d] = 65535 - 15 - 60 - (int32_t)(next_u32() % 5);        // the leader may end on exactly 65 535
                team[d] = (int32_t)(d % T);
            }
            const uint8_t cb[R] = {1, 0, 1};
            const int32_t bonus[R] = {20, 0, 40}, within[R] = {(int32_t)((n + 1) / 2), 1, (int32_t)n};
            std::unique_ptr<uint64_t[]> keys(new uint64_t[(size_t)words * n * cap]);
            std::unique_ptr<unsigned long long[]> bh(new unsigned long long[R * n]()), fh(new unsigned long long[R * n]());
            const char *err = "";
            const int rc = emu_champ_bonus_run(R, n, sims, cap, orders.get(), points.data(), cb, ip.data(), ic.data(),
                                               team.data(), T, bonus, within, fd.get(), fp.get(), grid, keys.get(), bh.get(),
                                               fh.get(), nullptr, &err);
            if (rc != MCGP_OK) {
                std::fprintf(stderr, "n = %u, shape %d: rc %d: %s\n", n, shape, rc, err);
                return 1;
            }
            unsigned long long fastest = 0, none = 0;
            for (uint32_t d = 0; d < n; ++d) fastest += fh[d] + fh[2 * n + d];
            for (uint64_t s = 0; s < sims; ++s) none += (fd[s] == 0xFF) + (fd[2 * sims + s] == 0xFF);
            if (fastest + none != 2 * sims) {
                std::fprintf(stderr, "n = %u, shape %d: %llu fastest laps + %llu without, of %llu\n", n, shape, fastest, none,
                             (unsigned long long)(2 * sims));
                return 1;
            }
        }
    }
    emu_champ_shutdown();
    std::puts("ok");
    return 0;
}
#endif

#ifdef SANITIZE_FASTEST
extern "C" int emu_fastest_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                               uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *orders,
                               uint8_t *fl_driver, uint8_t *fl_pos, const char **err);

int main()
{
    const struct { uint32_t n; int laps; uint64_t sims; } runs[] = {{1, 10, 40}, {2, 10, 40}, {20, 30, 64}, {32, 12, 40}, {20, 1, 40}};
    for (const auto &run : runs) {
        const uint32_t n = run.n;
        mcgp_config cfg = {};
        cfg.total_laps = run.laps;
        cfg.track_condition = MCGP_DRY;
        cfg.pit_loss = 22.0;
        cfg.overtake_delta = 0.3;
        cfg.sc_probability = 0.03;
        cfg.vsc_probability = 0.03;
        cfg.red_flag_probability = 0.01;
        cfg.drs_delta = 0.3;
        cfg.dirty_air_threshold = 2.0;
        cfg.dirty_air_penalty = 0.5;
        const double delta[5] = {-0.6, 0.0, 0.5, 2.0, 4.0}, deg[5] = {0.08, 0.05, 0.03, 0.04, 0.03};
        const int32_t opt[5] = {8, 14, 22, 20, 25};
        for (int c = 0; c < 5; ++c) {
            cfg.comp_pace_delta[c] = delta[c];
            cfg.comp_deg_rate[c] = deg[c];
            cfg.comp_optimal_laps[c] = opt[c];
        }
        cfg.pop_soft_hard = MCGP_HARD;
        cfg.pop_medium_hard = MCGP_HARD;
        cfg.deviates = MCGP_DEVIATES_32;
        std::vector<double> base(n), tdeg(n, 0.05), var(n, 0.2), dnf1(n, 0.01), dnf(n, 0.02), grid((size_t)n * n);
        for (uint32_t d = 0; d < n; ++d) base[d] = 90.0 + 0.05 * d;
        for (auto &g : grid) g = 0.05 + (double)(next_u32() % 100) / 100.0;
        const mcgp_drivers drv = {base.data(), tdeg.data(), tdeg.data(), var.data(), dnf1.data(), dnf.data()};
        std::unique_ptr<unsigned long long[]> hist(new unsigned long long[n * n]());
        std::unique_ptr<uint8_t[]> orders(new uint8_t[run.sims * n]), fd(new uint8_t[run.sims]), fp(new uint8_t[run.sims]);
        const char *err = "";
        const int rc = emu_fastest_run(&cfg, &drv, grid.data(), n, run.sims, 1000, 77, hist.get(), orders.get(), fd.get(),
                                       fp.get(), &err);
        if (rc != MCGP_OK) {
            std::fprintf(stderr, "n = %u, %d laps: rc %d: %s\n", n, run.laps, rc, err);
            return 1;
        }
        for (uint64_t s = 0; s < run.sims; ++s) {
            // the position byte names the place of the fastest-lap driver in the finishing order; one lap: none
            const bool none = fd[s] == 0xFF;
            const bool ok = none ? fp[s] == 0xFF : fp[s] < n && orders[s * n + fp[s]] == fd[s];
            if (!ok || (run.laps == 1 && !none)) {
                std::fprintf(stderr, "n = %u, %d laps, simulation %llu: bytes %u / %u\n", n, run.laps, (unsigned long long)s,
                             fd[s], fp[s]);
                return 1;
            }
        }
    }
    std::puts("ok");
    return 0;
}
#endif
