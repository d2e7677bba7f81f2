// sanitize_penalties_main.cpp -- a stand-alone program over the host DEBUGGING build of the penalties kernels and their
// packer (csrc/penalty_pack.h), for the host's sanitizers (not product code).  Compiled together with emu_generic.cpp:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
//       -static-libubsan -pthread -fno-sanitize=alignment -ffp-contract=off -Itools/emu \
//       tools/emu/sanitize_penalties_main.cpp tools/emu/emu_generic.cpp -o san_penalties
//
// (-fno-sanitize=alignment for the reason given in sanitize_bonus_main.cpp: a block of one thread.)  It runs
// emu_penalties_run (race_scenario_kernel<false, kRulePenalties>, then penalties_count as blocks of one thread) on fields of 1, 2, 20
// and 32 cars and a race of two laps, under scenarios that hold every kind of penalty, the most penalties a scenario
// takes (256), a planned stop that serves a penalty, and driver n - 1 (mask bit 31 at 32 cars); every buffer on the heap
// at exactly its size.  It checks that every staged row is a permutation with fate bits that agree with the scenario,
// and that the counted fates are the staged ones.  Exit status 0 and "ok" when every call returned MCGP_OK and the
// sanitizers found nothing.  tests/test_penalties_sanitize.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/mcgp.h"

extern "C" int emu_penalties_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                                 const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                                 const mcgp_pit_plan *plans, const uint32_t *penalty_count, const mcgp_time_penalty *penalties,
                                 uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage,
                                 unsigned long long *delta, unsigned long long *fate, uint32_t grid_x, const char **err);

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
    const struct { uint32_t n; int laps; uint64_t sims; } runs[] = {{1, 10, 40}, {2, 10, 40}, {20, 30, 64}, {32, 12, 40}, {20, 2, 40}};
    for (const auto &run : runs) {
        const uint32_t n = run.n;
        const int L = run.laps;
        mcgp_config cfg = {};
        cfg.total_laps = L;
        cfg.track_condition = MCGP_DRY;
        cfg.pit_loss = 22.0;
        cfg.overtake_delta = 0.3;
        cfg.sc_probability = 0.03;
        cfg.vsc_probability = 0.03;
        cfg.red_flag_probability = 0.01;
        cfg.drs_delta = 0.3;
        cfg.dirty_air_threshold = 2.0;
        cfg.dirty_air_penalty = 0.5;
        const double cdelta[5] = {-0.6, 0.0, 0.5, 2.0, 4.0}, deg[5] = {0.08, 0.05, 0.03, 0.04, 0.03};
        const int32_t opt[5] = {8, 14, 22, 20, 25};
        for (int c = 0; c < 5; ++c) {
            cfg.comp_pace_delta[c] = cdelta[c];
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

        // scenarios: none | every kind on driver n - 1 | a planned stop on lap L that serves driver 0's penalty |
        // as many lap additions as a scenario takes
        const uint32_t S = 4, last = n - 1;
        std::vector<mcgp_time_penalty> pens;
        std::vector<uint32_t> pen_count(S, 0), plan_count(S, 0);
        pens.push_back({(int32_t)last, MCGP_PEN_SERVE_AT_STOP, 2, 5.0});
        pens.push_back({(int32_t)last, MCGP_PEN_AT_FLAG, 0, 10.0});
        pens.push_back({(int32_t)last, MCGP_PEN_ON_LAP, L, 20.0});
        pen_count[1] = 3;
        pens.push_back({0, MCGP_PEN_SERVE_AT_STOP, L, 1e6});
        pen_count[2] = 1;
        for (int lap = 2; lap <= L && pen_count[3] < MCGP_MAX_SCENARIO_PENALTIES; ++lap)
            for (uint32_t d = 0; d < n && pen_count[3] < MCGP_MAX_SCENARIO_PENALTIES; ++d, ++pen_count[3])
                pens.push_back({(int32_t)(n - 1 - d), MCGP_PEN_ON_LAP, lap, 0.25 + d});
        mcgp_pit_plan plan = {};
        plan.driver = 0;
        plan.start_compound = -1;
        plan.n_stops = 1;
        plan.stop_lap[0] = (int16_t)L;
        plan.stop_compound[0] = MCGP_SOFT;
        plan_count[2] = 1;

        const uint64_t m = run.sims;
        const size_t w = 2 * (size_t)n - 1;
        std::unique_ptr<unsigned long long[]> hist(new unsigned long long[S * n * n]()), delta(new unsigned long long[S * n * w]()),
            fate(new unsigned long long[S * n * 4]());
        std::unique_ptr<uint8_t[]> stage(new uint8_t[S * m * n]);
        const char *err = "";
        const int rc = emu_penalties_run(&cfg, &drv, grid.data(), nullptr, n, S, plan_count.data(), &plan, pen_count.data(),
                                         pens.data(), m, 1000, 77, hist.get(), stage.get(), delta.get(), fate.get(), 3, &err);
        if (rc != MCGP_OK) {
            std::fprintf(stderr, "n = %u, %d laps: rc %d: %s\n", n, L, rc, err);
            return 1;
        }
        std::vector<unsigned long long> seen_fate(S * n * 4, 0);
        for (uint32_t s = 0; s < S; ++s)
            for (uint64_t i = 0; i < m; ++i) {
                const uint8_t *row = stage.get() + (s * m + i) * n;
                uint32_t seen = 0;
                for (uint32_t d = 0; d < n; ++d) {
                    const uint32_t pos = row[d] & 31u, f = (row[d] >> 5) & 3u;
                    const bool has_serve = (s == 1 && d == last) || (s == 2 && d == 0);
                    // a penalty pending from lap L with a planned stop on lap L is served or its car retired
                    const bool ok = pos < n && !(row[d] & 0x80u) && (f != 0u) == has_serve && !(s == 2 && f == 2u);
                    if (!ok) {
                        std::fprintf(stderr, "n = %u, %d laps, scenario %u, simulation %llu, driver %u: byte %u\n", n, L, s,
                                     (unsigned long long)i, d, row[d]);
                        return 1;
                    }
                    seen |= 1u << pos;
                    seen_fate[(s * n + d) * 4 + f] += 1;
                }
                if (seen != (n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u)) {
                    std::fprintf(stderr, "n = %u, scenario %u, simulation %llu: not a permutation\n", n, s, (unsigned long long)i);
                    return 1;
                }
            }
        for (size_t k = 0; k < (size_t)S * n * 4; ++k)
            if (k % 4 != 0 && fate[k] != seen_fate[k]) {
                std::fprintf(stderr, "n = %u, %d laps: fate cell %zu: counted %llu, staged %llu\n", n, L, k, fate[k], seen_fate[k]);
                return 1;
            }
    }
    std::puts("ok");
    return 0;
}
