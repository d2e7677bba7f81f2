// sanitize_grids_main.cpp -- a stand-alone program over the host DEBUGGING build of the grid-scenario kernels and their
// packer (csrc/grid_pack.h), for the host's sanitizers (not product code).  Compiled together with emu_generic.cpp, as
// sanitize_events_main.cpp documents:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
//       -static-libubsan -pthread -fno-sanitize=alignment -ffp-contract=off -Itools/emu \
//       tools/emu/sanitize_grids_main.cpp tools/emu/emu_generic.cpp -o san_grids
//
// (-fno-sanitize=alignment for the reason given in sanitize_bonus_main.cpp: a block of one thread.)  It runs
// emu_grid_run (race_scenario_kernel<false, kRuleGrid>, then grid_count as blocks of one thread) on fields of 1, 2, 11
// and 32 cars under scenarios at the limits of the edit table: none; a drop of 255 of the last driver; every driver
// dropped (all keys tie-free only by the drawn slot); every driver pinned, on the reversed grid; every driver from the
// pit lane; the last driver from the pit lane behind the first one pinned on the last slot left; a drop and a pin across
// the tyre boundary at n >= 11; every buffer on the heap at exactly its size.  It checks that every staged row of
// positions and of start slots is a permutation, that a pinned driver starts from its slot and a pit-lane driver from
// one of the last slots, that the counted start slots and gains are the staged ones, that the packer refuses what the
// header says it refuses, and that a run without the u16 staging gives the same positions.  Exit status 0 and "ok" when
// every call returned what it should and the sanitizers found nothing.  tests/test_grids_sanitize.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../../include/mcgp.h"

extern "C" int emu_grid_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                            uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                            const uint32_t *edit_count, const mcgp_grid_edit *edits, uint64_t n_sims, uint64_t sim_offset,
                            uint64_t seed, unsigned long long *hist, uint8_t *stage, uint16_t *car_stage,
                            unsigned long long *start, unsigned long long *gain, uint32_t grid_x, const char **err);

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

using Scenario = std::vector<mcgp_grid_edit>;

}  // namespace

int main()
{
    const uint32_t sizes[4] = {1, 2, 11, 32};
    for (const uint32_t n : sizes) {
        const int32_t N = (int32_t)n;
        std::vector<Scenario> scen;
        scen.push_back({});
        scen.push_back({{N - 1, MCGP_GRID_DROP, 255, 0.0}});
        {
            Scenario all_drop, all_pin, all_lane;
            for (int32_t d = 0; d < N; ++d) {
                all_drop.push_back({d, MCGP_GRID_DROP, 1 + (d * 7) % 255, 0.0});
                all_pin.push_back({d, MCGP_GRID_PIN, N - d, 0.0});
                all_lane.push_back({d, MCGP_GRID_PIT_LANE, 0, d == 0 ? 1e6 : 0.5 * d});
            }
            scen.push_back(all_drop);
            scen.push_back(all_pin);
            scen.push_back(all_lane);
        }
        if (n >= 2) scen.push_back({{N - 1, MCGP_GRID_PIT_LANE, 0, 2.5}, {0, MCGP_GRID_PIN, N - 1, 0.0}});
        if (n >= 11) scen.push_back({{3, MCGP_GRID_DROP, 9, 0.0}, {N - 1, MCGP_GRID_PIN, 10, 0.0}, {0, MCGP_GRID_PIN, 11, 0.0}});
        const uint32_t S = (uint32_t)scen.size();
        const int L = 12;
        mcgp_config cfg = {};
        cfg.total_laps = L;
        cfg.track_condition = MCGP_DRY;
        cfg.pit_loss = 22.0;
        cfg.overtake_delta = 0.3;
        cfg.sc_probability = 0.03;
        cfg.vsc_probability = 0.03;
        cfg.red_flag_probability = 0.02;
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

        std::vector<mcgp_grid_edit> edits;
        std::vector<uint32_t> edit_count(S, 0), plan_count(S, 0);
        for (uint32_t s = 0; s < S; ++s) {
            edit_count[s] = (uint32_t)scen[s].size();
            for (const mcgp_grid_edit &e : scen[s]) edits.push_back(e);
        }
        // driver n - 1 starts the pit-lane scenario (4: everybody in the lane) on new hard tyres
        std::unique_ptr<mcgp_pit_plan> plan(new mcgp_pit_plan());
        plan->driver = N - 1;
        plan->start_compound = MCGP_HARD;
        plan->n_stops = 0;
        plan_count[4] = 1;

        const uint64_t m = 24;
        const uint32_t w = 2 * n - 1;
        std::unique_ptr<unsigned long long[]> hist(new unsigned long long[S * n * n]()), hist2(new unsigned long long[S * n * n]()),
            start(new unsigned long long[S * n * n]()), gain(new unsigned long long[S * n * w]());
        std::unique_ptr<uint8_t[]> stage(new uint8_t[S * m * n]), stage2(new uint8_t[S * m * n]);
        std::unique_ptr<uint16_t[]> car(new uint16_t[S * m * n]);
        for (size_t k = 0; k < S * m * n; ++k) car[k] = 0xEEEE;
        const char *err = "";
        int rc = emu_grid_run(&cfg, &drv, grid.data(), n, S, plan_count.data(), plan.get(), edit_count.data(), edits.data(), m,
                              1000, 77, hist.get(), stage.get(), car.get(), start.get(), gain.get(), 3, &err);
        if (rc == MCGP_OK)      // ... and without the u16 staging
            rc = emu_grid_run(&cfg, &drv, grid.data(), n, S, plan_count.data(), plan.get(), edit_count.data(), edits.data(), m,
                              1000, 77, hist2.get(), stage2.get(), nullptr, nullptr, nullptr, 3, &err);
        if (rc != MCGP_OK) {
            std::fprintf(stderr, "n = %u: rc %d: %s\n", n, rc, err);
            return 1;
        }
        if (std::memcmp(stage.get(), stage2.get(), S * m * n) != 0 ||
            std::memcmp(hist.get(), hist2.get(), sizeof(unsigned long long) * S * n * n) != 0) {
            std::fprintf(stderr, "n = %u: the positions depend on the u16 staging\n", n);
            return 1;
        }
        const uint32_t all = n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u;
        std::vector<unsigned long long> seen_s(S * n * n, 0), seen_g(S * n * w, 0);
        for (uint32_t s = 0; s < S; ++s)
            for (uint64_t i = 0; i < m; ++i) {
                const uint8_t *row = stage.get() + (s * m + i) * n;
                const uint16_t *crow = car.get() + (s * m + i) * n;
                uint32_t seen = 0, slots = 0;
                for (uint32_t d = 0; d < n; ++d) {
                    if (row[d] >= n || crow[d] >= n) {
                        std::fprintf(stderr, "n = %u, scenario %u, simulation %llu, driver %u: byte %u, slot %u\n", n, s,
                                     (unsigned long long)i, d, row[d], crow[d]);
                        return 1;
                    }
                    seen |= 1u << row[d];
                    slots |= 1u << crow[d];
                    seen_s[((size_t)s * n + d) * n + crow[d]] += 1;
                    seen_g[((size_t)s * n + d) * w + (crow[d] + n - 1 - row[d])] += 1;
                }
                if (seen != all || slots != all) {
                    std::fprintf(stderr, "n = %u, scenario %u, simulation %llu: not a permutation\n", n, s, (unsigned long long)i);
                    return 1;
                }
                uint32_t n_lane = 0;
                for (const mcgp_grid_edit &e : scen[s]) n_lane += e.kind == MCGP_GRID_PIT_LANE;
                for (const mcgp_grid_edit &e : scen[s]) {
                    const uint32_t slot = crow[e.driver];
                    const bool ok = e.kind == MCGP_GRID_PIN ? slot == (uint32_t)e.value - 1
                                    : e.kind == MCGP_GRID_PIT_LANE ? slot >= n - n_lane : true;
                    if (!ok) {
                        std::fprintf(stderr, "n = %u, scenario %u, simulation %llu: driver %d starts from slot %u\n", n, s,
                                     (unsigned long long)i, e.driver, slot);
                        return 1;
                    }
                }
                // the last driver, dropped 255 places, starts last
                if (s == 1 && crow[n - 1] != n - 1) {
                    std::fprintf(stderr, "n = %u, simulation %llu: the dropped driver starts from slot %u\n", n,
                                 (unsigned long long)i, crow[n - 1]);
                    return 1;
                }
            }
        for (size_t k = 0; k < (size_t)S * n * n; ++k)
            if (start[k] != seen_s[k]) {
                std::fprintf(stderr, "n = %u: start cell %zu: counted %llu, staged %llu\n", n, k, start[k], seen_s[k]);
                return 1;
            }
        for (size_t k = 0; k < (size_t)S * n * w; ++k)
            if (gain[k] != seen_g[k]) {
                std::fprintf(stderr, "n = %u: gain cell %zu: counted %llu, staged %llu\n", n, k, gain[k], seen_g[k]);
                return 1;
            }

        // what the packer refuses: every case one scenario at exactly its size on the heap
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::vector<Scenario> bad = {
            {{N, MCGP_GRID_DROP, 1, 0.0}},       {{-1, MCGP_GRID_PIN, 1, 0.0}},        {{0, 3, 1, 0.0}},
            {{0, MCGP_GRID_DROP, 0, 0.0}},       {{0, MCGP_GRID_DROP, 256, 0.0}},      {{0, MCGP_GRID_PIN, N + 1, 0.0}},
            {{0, MCGP_GRID_PIN, 0, 0.0}},        {{0, MCGP_GRID_PIT_LANE, 1, 0.0}},    {{0, MCGP_GRID_PIT_LANE, 0, nan}},
            {{0, MCGP_GRID_PIT_LANE, 0, -1.0}},  {{0, MCGP_GRID_PIT_LANE, 0, 1e6 + 1}}, {{0, MCGP_GRID_DROP, 1, 0.5}},
            {{0, MCGP_GRID_PIN, N, 0.0}, {0, MCGP_GRID_PIT_LANE, 0, 1.0}},
        };
        if (n >= 2) {
            bad.push_back({{0, MCGP_GRID_PIN, 1, 0.0}, {1, MCGP_GRID_PIN, 1, 0.0}});
            bad.push_back({{0, MCGP_GRID_PIN, N, 0.0}, {1, MCGP_GRID_PIT_LANE, 0, 1.0}});
            bad.push_back(Scenario((size_t)n + 1, mcgp_grid_edit{0, MCGP_GRID_DROP, 1, 0.0}));
        }
        for (size_t b = 0; b < bad.size(); ++b) {
            const uint32_t count = (uint32_t)bad[b].size(), none = 0;
            std::unique_ptr<mcgp_grid_edit[]> items(new mcgp_grid_edit[count]);
            for (uint32_t k = 0; k < count; ++k) items[k] = bad[b][k];
            std::unique_ptr<unsigned long long[]> h(new unsigned long long[n * n]());
            std::unique_ptr<uint8_t[]> st(new uint8_t[2 * n]);
            rc = emu_grid_run(&cfg, &drv, grid.data(), n, 1, &none, nullptr, &count, items.get(), 2, 0, 1, h.get(), st.get(),
                              nullptr, nullptr, nullptr, 1, &err);
            if (rc != MCGP_E_BAD_ARG) {
                std::fprintf(stderr, "n = %u: bad scenario %zu was not refused (rc %d)\n", n, b, rc);
                return 1;
            }
        }
    }
    std::puts("ok");
    return 0;
}
