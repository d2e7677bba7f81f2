// sanitize_paces_main.cpp -- a stand-alone program over the host DEBUGGING build of the pace-scenario kernels and their
// packer (csrc/pace_pack.h), for the host's sanitizers (not product code).  Compiled together with emu_generic.cpp:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
//       -static-libubsan -pthread -fno-sanitize=alignment -ffp-contract=off -Itools/emu \
//       tools/emu/sanitize_paces_main.cpp tools/emu/emu_generic.cpp -o san_paces
//
// (-fno-sanitize=alignment for the reason given in sanitize_bonus_main.cpp: a block of one thread.)  It runs
// emu_paces_run (race_scenario_kernel<false, kRulePaces>, then paces_count as blocks of one thread) at the limits: 64 scenarios of 64
// single-lap offsets on 3 cars over 70 laps; 1000 laps on 2 cars with an UNTIL_STOP offset from lap 1 that no stop
// clears and two LAPS ranges that meet; a race of one lap with an offset on lap 1; and 32 cars with offsets of both kinds
// on drivers 0 and 31; every buffer on the heap at exactly its size.  It checks that every staged row is a permutation,
// that the staged laps carried are within [0, L] at the drivers that have an UNTIL_STOP offset, that a car under a plan
// without stops that cannot retire carries its offset to the flag, and that the counted laps are the staged ones.  Exit
// status 0 and "ok" when every call returned MCGP_OK and the sanitizers found nothing.  tests/test_paces_sanitize.py
// builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/mcgp.h"

extern "C" int emu_paces_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                             const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                             const mcgp_pit_plan *plans, const uint32_t *pace_count, const mcgp_pace_offset *paces,
                             uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage,
                             uint16_t *car_stage, unsigned long long *delta, unsigned long long *carried, uint32_t grid_x,
                             const char **err);

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
    bool retirements;
    std::vector<std::vector<mcgp_pace_offset>> scen;    // the offsets of every scenario
    int planned;                                        // scenario whose driver 0 has a plan without stops, or -1
};

mcgp_pace_offset laps(int d, int a, int b, double s) { return {d, MCGP_PACE_LAPS, a, b, s}; }
mcgp_pace_offset until(int d, int p, double s) { return {d, MCGP_PACE_UNTIL_STOP, p, 0, s}; }

}  // namespace

int main()
{
    std::vector<Run> runs;
    {   // 64 scenarios x 64 single-lap offsets, 3 cars, 70 laps
        Run r = {3, 70, 2, true, {}, -1};
        for (int s = 0; s < 64; ++s) {
            std::vector<mcgp_pace_offset> o;
            for (int lap = 1; lap <= MCGP_MAX_SCENARIO_PACES; ++lap) o.push_back(laps((s + lap) % 3, lap, lap, 0.05 * ((s + lap) % 9 - 4)));
            r.scen.push_back(o);
        }
        runs.push_back(r);
    }
    // 1000 laps, 2 cars that cannot retire: an UNTIL_STOP offset from lap 1 under a plan without stops lands in column L
    runs.push_back({2, 1000, 2, false, {{}, {until(0, 1, 0.4), laps(1, 1, 500, 0.2), laps(1, 501, 1000, -0.2)},
                                        {until(1, 1000, -0.3), until(0, 2, 0.1)}}, 1});
    // one lap: an offset on lap 1 only
    runs.push_back({3, 1, 40, true, {{}, {laps(0, 1, 1, 1.7)}, {until(1, 1, -0.9), laps(1, 1, 1, -0.8)}}, -1});
    // 32 cars: drivers 0 and 31, both kinds on the same laps
    runs.push_back({32, 30, 24, true, {{}, {laps(0, 1, 30, 0.3), until(0, 1, 0.1), laps(31, 1, 30, 0.1), until(31, 1, 0.3)},
                                       {until(31, 30, 60.0), laps(31, 2, 2, -60.0), laps(0, 29, 30, 0.0)}}, -1});
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
        const double rate = run.retirements ? 0.02 : 0.0;
        std::vector<double> base(n), tdeg(n, 0.05), var(n, 0.2), dnf1(n, rate / 2), dnf(n, rate), grid((size_t)n * n);
        for (uint32_t d = 0; d < n; ++d) base[d] = 90.0 + 0.05 * d;
        for (auto &g : grid) g = 0.05 + (double)(next_u32() % 100) / 100.0;
        const mcgp_drivers drv = {base.data(), tdeg.data(), tdeg.data(), var.data(), dnf1.data(), dnf.data()};

        std::vector<mcgp_pace_offset> offs;
        std::vector<uint32_t> pace_count(S, 0), plan_count(S, 0), until_mask(S, 0);
        for (uint32_t s = 0; s < S; ++s) {
            pace_count[s] = (uint32_t)run.scen[s].size();
            for (const mcgp_pace_offset &o : run.scen[s]) {
                offs.push_back(o);
                if (o.kind == MCGP_PACE_UNTIL_STOP) until_mask[s] |= 1u << o.driver;
            }
        }
        mcgp_pit_plan plan = {};
        plan.driver = 0;
        plan.start_compound = -1;
        plan.n_stops = 0;
        if (run.planned >= 0) plan_count[run.planned] = 1;

        const uint64_t m = run.sims;
        const size_t w = 2 * (size_t)n - 1, row_cells = (size_t)L + 1;
        std::unique_ptr<unsigned long long[]> hist(new unsigned long long[S * n * n]()), delta(new unsigned long long[S * n * w]()),
            counted(new unsigned long long[S * n * row_cells]());
        std::unique_ptr<uint8_t[]> stage(new uint8_t[S * m * n]);
        std::unique_ptr<uint16_t[]> car(new uint16_t[S * m * n]);
        for (size_t k = 0; k < S * m * n; ++k) car[k] = 0xEEEE;
        const char *err = "";
        const int rc = emu_paces_run(&cfg, &drv, grid.data(), nullptr, n, S, plan_count.data(), &plan, pace_count.data(),
                                     offs.empty() ? nullptr : offs.data(), m, 1000, 77, hist.get(), stage.get(), car.get(),
                                     delta.get(), counted.get(), 3, &err);
        if (rc != MCGP_OK) {
            std::fprintf(stderr, "n = %u, %d laps: rc %d: %s\n", n, L, rc, err);
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
                    const bool has = (until_mask[s] >> d) & 1u;
                    if (has ? crow[d] > (uint32_t)L : crow[d] != 0xEEEE) {
                        std::fprintf(stderr, "n = %u, %d laps, scenario %u, simulation %llu, driver %u: laps carried %u\n", n, L,
                                     s, (unsigned long long)i, d, crow[d]);
                        return 1;
                    }
                    if (has && crow[d]) seen_c[((size_t)s * n + d) * row_cells + crow[d]] += 1;     // column 0 is the host's
                }
                if (seen != (n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u)) {
                    std::fprintf(stderr, "n = %u, scenario %u, simulation %llu: not a permutation\n", n, s, (unsigned long long)i);
                    return 1;
                }
                // nobody retires and driver 0's plan has no stop: its offset from lap 1 is carried on all L laps
                if ((int)s == run.planned && !run.retirements && crow[0] != (uint32_t)L) {
                    std::fprintf(stderr, "%d laps, scenario %u, simulation %llu: carried %u laps, not %d\n", L, s,
                                 (unsigned long long)i, crow[0], L);
                    return 1;
                }
            }
        for (size_t k = 0; k < (size_t)S * n * row_cells; ++k)
            if (counted[k] != seen_c[k]) {
                std::fprintf(stderr, "n = %u, %d laps: carried cell %zu: counted %llu, staged %llu\n", n, L, k, counted[k], seen_c[k]);
                return 1;
            }
    }
    std::puts("ok");
    return 0;
}
