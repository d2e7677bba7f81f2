// sanitize_events_main.cpp -- a stand-alone program over the host DEBUGGING build of the event-scenario kernels and their
// packer (csrc/event_pack.h), for the host's sanitizers (not product code).  Compiled together with emu_generic.cpp:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
//       -static-libubsan -pthread -fno-sanitize=alignment -ffp-contract=off -Itools/emu \
//       tools/emu/sanitize_events_main.cpp tools/emu/emu_generic.cpp -o san_events
//
// (-fno-sanitize=alignment for the reason given in sanitize_bonus_main.cpp: a block of one thread.)  It runs
// emu_events_run (race_scenario_kernel<false, kRuleEvents>, then events_count as blocks of one thread) on fields of 1, 2, 20 and 32
// cars, a race of two laps and one of 1000, under scenarios that hold every kind on single laps (the first and the last
// included), a whole-race range of each kind, the most overrides a scenario takes (64) and a planned stop on a forced
// safety-car lap; every buffer on the heap at exactly its size.  It checks that every staged row is a permutation, that
// the staged event counts of the whole-race scenarios are exact, and that the counted events are the staged ones.  Exit
// status 0 and "ok" when every call returned MCGP_OK and the sanitizers found nothing.  tests/test_events_sanitize.py
// builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/mcgp.h"

extern "C" int emu_events_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                              const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                              const mcgp_pit_plan *plans, const uint32_t *event_count, const mcgp_lap_event *events,
                              uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage,
                              uint32_t *ev_stage, unsigned long long *delta, unsigned long long *events_cnt, uint32_t grid_x,
                              const char **err);

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
    const struct { uint32_t n; int laps; uint64_t sims; } runs[] = {{1, 10, 40}, {2, 10, 40}, {20, 30, 64}, {32, 12, 40},
                                                                    {20, 2, 40}, {3, 1000, 6}, {32, 70, 8}};
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
        std::vector<double> base(n), tdeg(n, 0.05), var(n, 0.2), dnf1(n, 0.01), dnf(n, L > 100 ? 0.001 : 0.02), grid((size_t)n * n);
        for (uint32_t d = 0; d < n; ++d) base[d] = 90.0 + 0.05 * d;
        for (auto &g : grid) g = 0.05 + (double)(next_u32() % 100) / 100.0;
        const mcgp_drivers drv = {base.data(), tdeg.data(), tdeg.data(), var.data(), dnf1.data(), dnf.data()};

        // scenarios: none | kinds 0..3 over the whole race (4 scenarios) | single laps: 2 and L | as many single-lap
        // overrides as a scenario takes | a safety car on lap L with a planned stop of driver n - 1 on it
        const uint32_t S = 8;
        std::vector<mcgp_lap_event> evs;
        std::vector<uint32_t> ev_count(S, 0), plan_count(S, 0);
        for (int kind = 0; kind < 4; ++kind) {
            evs.push_back({2, L, kind});
            ev_count[1 + kind] = 1;
        }
        evs.push_back({2, 2, MCGP_EVT_RED_FLAG});
        ev_count[5] = 1;
        if (L > 2) {
            evs.push_back({L, L, MCGP_EVT_VSC});
            ev_count[5] = 2;
        }
        for (int lap = 2; lap <= L && ev_count[6] < MCGP_MAX_SCENARIO_EVENTS; ++lap, ++ev_count[6])
            evs.push_back({lap, lap, (int32_t)(next_u32() % 4)});
        evs.push_back({L, L, MCGP_EVT_SAFETY_CAR});
        ev_count[7] = 1;
        mcgp_pit_plan plan = {};
        plan.driver = (int32_t)(n - 1);
        plan.start_compound = -1;
        plan.n_stops = 1;
        plan.stop_lap[0] = (int16_t)L;
        plan.stop_compound[0] = MCGP_SOFT;
        plan_count[7] = 1;

        const uint64_t m = run.sims;
        const size_t w = 2 * (size_t)n - 1, ev_cells = 3 * (size_t)(L + 1);
        std::unique_ptr<unsigned long long[]> hist(new unsigned long long[S * n * n]()), delta(new unsigned long long[S * n * w]()),
            counted(new unsigned long long[S * ev_cells]());
        std::unique_ptr<uint8_t[]> stage(new uint8_t[S * m * n]);
        std::unique_ptr<uint32_t[]> ev_stage(new uint32_t[S * m]);
        const char *err = "";
        const int rc = emu_events_run(&cfg, &drv, grid.data(), nullptr, n, S, plan_count.data(), &plan, ev_count.data(),
                                      evs.data(), m, 1000, 77, hist.get(), stage.get(), ev_stage.get(), delta.get(),
                                      counted.get(), 3, &err);
        if (rc != MCGP_OK) {
            std::fprintf(stderr, "n = %u, %d laps: rc %d: %s\n", n, L, rc, err);
            return 1;
        }
        std::vector<unsigned long long> seen_ev(S * ev_cells, 0);
        for (uint32_t s = 0; s < S; ++s)
            for (uint64_t i = 0; i < m; ++i) {
                const uint8_t *row = stage.get() + (s * m + i) * n;
                uint32_t seen = 0;
                for (uint32_t d = 0; d < n; ++d) {
                    if (row[d] >= n) {
                        std::fprintf(stderr, "n = %u, %d laps, scenario %u, simulation %llu, driver %u: byte %u\n", n, L, s,
                                     (unsigned long long)i, d, row[d]);
                        return 1;
                    }
                    seen |= 1u << row[d];
                }
                if (seen != (n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u)) {
                    std::fprintf(stderr, "n = %u, scenario %u, simulation %llu: not a permutation\n", n, s, (unsigned long long)i);
                    return 1;
                }
                const uint32_t r = ev_stage[s * m + i];
                for (uint32_t k = 0; k < 3; ++k) {
                    const uint32_t c = (r >> (10 * k)) & 1023u;
                    // a whole-race scenario of kind k + 1 has L - 1 such laps and none of the others
                    if ((r >> 30) != 0u || c > (uint32_t)(L - 1) ||
                        (s >= 1 && s <= 4 && c != (s - 1 == k + 1 ? (uint32_t)(L - 1) : 0u))) {
                        std::fprintf(stderr, "n = %u, %d laps, scenario %u, simulation %llu: event word %08x\n", n, L, s,
                                     (unsigned long long)i, r);
                        return 1;
                    }
                    seen_ev[s * ev_cells + k * (size_t)(L + 1) + c] += 1;
                }
            }
        for (size_t k = 0; k < (size_t)S * ev_cells; ++k)
            if (counted[k] != seen_ev[k]) {
                std::fprintf(stderr, "n = %u, %d laps: event cell %zu: counted %llu, staged %llu\n", n, L, k, counted[k], seen_ev[k]);
                return 1;
            }
    }
    std::puts("ok");
    return 0;
}
