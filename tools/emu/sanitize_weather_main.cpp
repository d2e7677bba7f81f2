// sanitize_weather_main.cpp -- a stand-alone program over the host DEBUGGING build of the weather-scenario kernels and
// their packer (csrc/weather_pack.h), for the host's sanitizers (not product code).  Compiled together with
// emu_generic.cpp, as sanitize_events_main.cpp documents:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
//       -static-libubsan -pthread -fno-sanitize=alignment -ffp-contract=off -Itools/emu \
//       tools/emu/sanitize_weather_main.cpp tools/emu/emu_generic.cpp -o san_weather
//
// (-fno-sanitize=alignment for the reason given in sanitize_bonus_main.cpp: a block of one thread.)  It runs
// emu_weather_run (race_scenario_kernel<false, kRuleWeather>, then weather_count as blocks of one thread) at the limits:
// fields of 1, 2, 20 and 32 cars; a race of 2 laps (one lap a change may name); 1000 laps on 2 cars that cannot retire,
// one of them on intermediates on a dry track under a plan without stops (its 1000 laps on the wrong tyres land in the
// last column); 64 scenarios of 64 single-lap changes on 20 cars over 70 laps; rain to the flag and a cross-back on 32
// cars under a table with every cell non-zero; every buffer on the heap at exactly its size.  It checks that every
// staged row is a permutation, that every staged count of laps is within [0, L], that the counted laps are the staged
// ones, and that a run without the u16 staging gives the same positions.  Exit status 0 and "ok" when every call returned
// MCGP_OK and the sanitizers found nothing.  tests/test_weather_sanitize.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/mcgp.h"

extern "C" int emu_weather_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                               const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                               const mcgp_pit_plan *plans, const uint32_t *change_count, const mcgp_track_change *changes,
                               const mcgp_weather_model *model, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                               unsigned long long *hist, uint8_t *stage, uint16_t *car_stage, unsigned long long *wrong,
                               uint32_t grid_x, const char **err);

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

struct Run {
    uint32_t n;
    int laps;
    uint64_t sims;
    bool retirements, full_table;
    std::vector<std::vector<mcgp_track_change>> scen;   // the changes of every scenario
    int planned;                                        // scenario whose driver 0 starts on intermediates and never stops, or -1
};

}  // namespace

int main()
{
    std::vector<Run> runs;
    runs.push_back({1, 2, 16, true, true, {{}, {{2, 2, MCGP_DAMP}}, {{2, 2, MCGP_WET_TRACK}}}, -1});
    runs.push_back({2, 2, 16, true, false, {{}, {{2, 2, MCGP_DRY}}, {{2, 2, MCGP_DAMP}}}, 2});
    runs.push_back({2, 1000, 2, false, false, {{}, {}, {{2, 500, MCGP_DAMP}, {501, 1000, MCGP_WET_TRACK}}, {{994, 1000, MCGP_DAMP}}}, 1});
    {   // 64 scenarios x 64 single-lap changes, 20 cars, 70 laps
        Run r = {20, 70, 2, true, true, {}, -1};
        for (int s = 0; s < 64; ++s) {
            std::vector<mcgp_track_change> c;
            for (int k = 0; k < MCGP_MAX_SCENARIO_TRACK_CHANGES; ++k) c.push_back({2 + k, 2 + k, (s + k) % 3});
            r.scen.push_back(c);
        }
        runs.push_back(r);
    }
    runs.push_back({32, 30, 24, true, true, {{}, {{12, 30, MCGP_DAMP}}, {{5, 9, MCGP_WET_TRACK}, {10, 12, MCGP_DAMP}}, {{24, 30, MCGP_DAMP}},
                                            {{25, 30, MCGP_DAMP}}}, 3});
    for (const Run &run : runs) {
        const uint32_t n = run.n, S = (uint32_t)run.scen.size();
        const int L = run.laps;
        mcgp_config cfg = {};
        cfg.total_laps = L;
        cfg.track_condition = MCGP_DRY;
        cfg.pit_loss = 22.0;
        cfg.overtake_delta = 0.3;
        cfg.sc_probability = 0.03;
        cfg.vsc_probability = 0.03;
        cfg.red_flag_probability = run.retirements ? 0.02 : 0.0;    // (a red flag would change the planned car's tyres)
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
        const double rate = run.retirements ? 0.02 : 0.0;
        std::vector<double> base(n), tdeg(n, 0.05), var(n, 0.2), dnf1(n, rate / 2), dnf(n, rate), grid((size_t)n * n);
        for (uint32_t d = 0; d < n; ++d) base[d] = 90.0 + 0.05 * d;
        for (auto &g : grid) g = 0.05 + (double)(next_u32() % 100) / 100.0;
        const mcgp_drivers drv = {base.data(), tdeg.data(), tdeg.data(), var.data(), dnf1.data(), dnf.data()};
        std::unique_ptr<mcgp_weather_model> model(new mcgp_weather_model());
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 5; ++k) model->wrong_tyre_sec[c][k] = run.full_table ? 0.2 + 0.9 * c + 0.17 * k : 0.0;

        std::vector<mcgp_track_change> changes;
        std::vector<uint32_t> change_count(S, 0), plan_count(S, 0);
        for (uint32_t s = 0; s < S; ++s) {
            change_count[s] = (uint32_t)run.scen[s].size();
            for (const mcgp_track_change &c : run.scen[s]) changes.push_back(c);
        }
        std::unique_ptr<mcgp_pit_plan> plan(new mcgp_pit_plan());
        plan->driver = 0;
        plan->start_compound = MCGP_INTERMEDIATE;
        plan->n_stops = 0;
        if (run.planned >= 0) plan_count[run.planned] = 1;

        const uint64_t m = run.sims;
        const size_t row_cells = (size_t)L + 1;
        std::unique_ptr<unsigned long long[]> hist(new unsigned long long[S * n * n]()), hist2(new unsigned long long[S * n * n]()),
            counted(new unsigned long long[S * n * row_cells]());
        std::unique_ptr<uint8_t[]> stage(new uint8_t[S * m * n]), stage2(new uint8_t[S * m * n]);
        std::unique_ptr<uint16_t[]> car(new uint16_t[S * m * n]);
        for (size_t k = 0; k < S * m * n; ++k) car[k] = 0xEEEE;
        const char *err = "";
        int rc = emu_weather_run(&cfg, &drv, grid.data(), nullptr, n, S, plan_count.data(), plan.get(), change_count.data(),
                                 changes.empty() ? nullptr : changes.data(), model.get(), m, 1000, 77, hist.get(), stage.get(),
                                 car.get(), counted.get(), 3, &err);
        if (rc == MCGP_OK)      // ... and without the u16 staging
            rc = emu_weather_run(&cfg, &drv, grid.data(), nullptr, n, S, plan_count.data(), plan.get(), change_count.data(),
                                 changes.empty() ? nullptr : changes.data(), model.get(), m, 1000, 77, hist2.get(),
                                 stage2.get(), nullptr, nullptr, 3, &err);
        if (rc != MCGP_OK) {
            std::fprintf(stderr, "n = %u, %d laps: rc %d: %s\n", n, L, rc, err);
            return 1;
        }
        if (std::memcmp(stage.get(), stage2.get(), S * m * n) != 0 ||
            std::memcmp(hist.get(), hist2.get(), sizeof(unsigned long long) * S * n * n) != 0) {
            std::fprintf(stderr, "n = %u, %d laps: the positions depend on the u16 staging\n", n, L);
            return 1;
        }
        std::vector<unsigned long long> seen_c(S * n * row_cells, 0);
        for (uint32_t s = 0; s < S; ++s)
            for (uint64_t i = 0; i < m; ++i) {
                const uint8_t *row = stage.get() + (s * m + i) * n;
                const uint16_t *crow = car.get() + (s * m + i) * n;
                uint32_t seen = 0;
                for (uint32_t d = 0; d < n; ++d) {
                    if (row[d] >= n) {
                        std::fprintf(stderr, "n = %u, %d laps, scenario %u, simulation %llu, driver %u: byte %u\n", n, L, s,
                                     (unsigned long long)i, d, row[d]);
                        return 1;
                    }
                    seen |= 1u << row[d];
                    if (crow[d] > (uint32_t)L) {
                        std::fprintf(stderr, "n = %u, %d laps, scenario %u, simulation %llu, driver %u: wrong-tyre laps %u\n", n,
                                     L, s, (unsigned long long)i, d, crow[d]);
                        return 1;
                    }
                    if (crow[d]) seen_c[((size_t)s * n + d) * row_cells + crow[d]] += 1;     // column 0 is the host's
                }
                if (seen != (n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u)) {
                    std::fprintf(stderr, "n = %u, scenario %u, simulation %llu: not a permutation\n", n, s, (unsigned long long)i);
                    return 1;
                }
                // nobody retires, the track stays dry and driver 0 never leaves its intermediates: all L laps are wrong
                if ((int)s == run.planned && !run.retirements && crow[0] != (uint32_t)L) {
                    std::fprintf(stderr, "%d laps, scenario %u, simulation %llu: %u laps on the wrong tyres, not %d\n", L, s,
                                 (unsigned long long)i, crow[0], L);
                    return 1;
                }
            }
        for (size_t k = 0; k < (size_t)S * n * row_cells; ++k)
            if (counted[k] != seen_c[k]) {
                std::fprintf(stderr, "n = %u, %d laps: wrong-tyre cell %zu: counted %llu, staged %llu\n", n, L, k, counted[k],
                             seen_c[k]);
                return 1;
            }
    }
    std::puts("ok");
    return 0;
}
