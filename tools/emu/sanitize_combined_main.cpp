// sanitize_combined_main.cpp -- a stand-alone program over the host DEBUGGING build of the combined-scenario kernel and
// the three packers it reads through (csrc/penalty_pack.h, event_pack.h, pace_pack.h), for the host's sanitizers (not
// product code).  Compiled together with emu_generic.cpp:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
//       -static-libubsan -pthread -fno-sanitize=alignment -ffp-contract=off -Itools/emu \
//       tools/emu/sanitize_combined_main.cpp tools/emu/emu_generic.cpp -o san_combined
//
// (-fno-sanitize=alignment for the reason given in sanitize_bonus_main.cpp: a block of one thread.)  It runs
// emu_combined_run (race_scenario_kernel<false, kRuleAll>, then penalties_count, events_count and paces_count as blocks of one
// thread) at the limits: 64 scenarios on 3 cars over 70 laps, each with 64 single-lap offsets, 64 single-lap overrides
// and additions on 64 laps; 1000 laps on 2 cars that cannot retire, with a penalty to serve and an offset from lap 2
// under a plan whose only stop is on lap 1000; a race of one lap (penalties and events cannot name lap 1: only an offset
// and a post-race penalty); 32 cars with every kind on drivers 0 and 31; and a call whose three count arrays are NULL;
// every buffer on the heap at exactly its size.  It checks that every staged byte is a position below n with a fate, every
// row a permutation, the fate 0 exactly where the driver has no penalty to serve, the staged laps carried within [0, L]
// exactly at the drivers with an UNTIL_STOP offset, the packed event counts within the laps run, the stop on lap 1000
// serving and clearing (fate 1, 999 laps carried), and the counted fates, events and laps the staged ones.  Exit status 0
// and "ok" when every call returned MCGP_OK and the sanitizers found nothing.  tests/test_combined_sanitize.py builds
// and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/mcgp.h"

extern "C" int emu_combined_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                                const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                                const mcgp_pit_plan *plans, const uint32_t *penalty_count, const mcgp_time_penalty *penalties,
                                const uint32_t *event_count, const mcgp_lap_event *events, const uint32_t *pace_count,
                                const mcgp_pace_offset *paces, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                                unsigned long long *hist, uint8_t *stage, uint32_t *ev_stage, uint16_t *car_stage,
                                unsigned long long *delta, unsigned long long *fate, unsigned long long *events_cnt,
                                unsigned long long *carried, uint32_t grid_x, const char **err);

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t next_u32()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

struct Scenario {
    std::vector<mcgp_time_penalty> pens;
    std::vector<mcgp_lap_event> evs;
    std::vector<mcgp_pace_offset> offs;
};

struct Run {
    uint32_t n;
    int laps;
    uint64_t sims;
    bool retirements;
    std::vector<Scenario> scen;
    int planned;            // scenario whose driver 0 has a plan with one stop on the last lap, or -1
    bool null_counts;       // pass the three count arrays as NULL (every scenario is empty)
};

mcgp_time_penalty serve(int d, int lap, double s) { return {d, MCGP_PEN_SERVE_AT_STOP, lap, s}; }
mcgp_time_penalty flag(int d, double s) { return {d, MCGP_PEN_AT_FLAG, 0, s}; }
mcgp_time_penalty on_lap(int d, int lap, double s) { return {d, MCGP_PEN_ON_LAP, lap, s}; }
mcgp_lap_event event(int a, int b, int kind) { return {a, b, kind}; }
mcgp_pace_offset laps(int d, int a, int b, double s) { return {d, MCGP_PACE_LAPS, a, b, s}; }
mcgp_pace_offset until(int d, int p, double s) { return {d, MCGP_PACE_UNTIL_STOP, p, 0, s}; }

#define FAIL(...)                                  \
    do {                                           \
        std::fprintf(stderr, __VA_ARGS__);         \
        std::fputc('\n', stderr);                  \
        return 1;                                  \
    } while (0)

}  // namespace

int main()
{
    std::vector<Run> runs;
    {   // 64 scenarios, each at the limits of the events and the offsets, 3 cars, 70 laps
        Run r = {3, 70, 2, true, {}, -1, false};
        for (int s = 0; s < 64; ++s) {
            Scenario sc;
            for (int k = 0; k < MCGP_MAX_SCENARIO_PACES; ++k) {
                const int lap = k + 1;
                sc.offs.push_back(laps((s + lap) % 3, lap, lap, 0.05 * ((s + lap) % 9 - 4)));
                sc.evs.push_back(event(k + 2, k + 2, (s + k) % 4));
                sc.pens.push_back(on_lap((s + k) % 3, k + 2, 1.0 + 0.25 * (k % 5)));
            }
            sc.pens.push_back(serve(s % 3, 2 + s % 60, 5.0));
            sc.pens.push_back(flag((s + 1) % 3, 10.0));
            r.scen.push_back(sc);
        }
        runs.push_back(r);
    }
    // 1000 laps, 2 cars that cannot retire: driver 0's only stop is on lap 1000; it serves there and clears the offset
    runs.push_back({2, 1000, 2, false,
                    {{}, {{serve(0, 2, 5.0), on_lap(0, 1000, 2.0), flag(1, 3.0)}, {event(1000, 1000, MCGP_EVT_SAFETY_CAR)},
                          {until(0, 2, 0.4), laps(1, 1, 500, 0.2), laps(1, 501, 1000, -0.2)}}},
                    1, false});
    // one lap: only an offset and a post-race penalty can be given
    runs.push_back({3, 1, 40, true, {{}, {{flag(0, 1.0)}, {}, {laps(0, 1, 1, 1.7), until(1, 1, -0.9)}}}, -1, false});
    // 32 cars: every kind on drivers 0 and 31
    runs.push_back({32, 30, 24, true,
                    {{},
                     {{serve(0, 2, 5.0), flag(0, 5.0), on_lap(0, 30, 3.0), serve(31, 30, 5.0), flag(31, 5.0), on_lap(31, 2, 3.0)},
                      {event(2, 2, MCGP_EVT_RED_FLAG), event(3, 29, MCGP_EVT_NONE), event(30, 30, MCGP_EVT_VSC)},
                      {laps(0, 1, 30, 0.3), until(0, 1, 0.1), laps(31, 1, 30, 0.1), until(31, 30, 60.0)}}},
                    -1, false});
    // the three count arrays NULL
    runs.push_back({5, 12, 16, true, {{}, {}}, -1, true});
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

        std::vector<mcgp_time_penalty> pens;
        std::vector<mcgp_lap_event> evs;
        std::vector<mcgp_pace_offset> offs;
        std::vector<uint32_t> pen_count(S, 0), ev_count(S, 0), pace_count(S, 0), plan_count(S, 0), serve_mask(S, 0),
            until_mask(S, 0);
        for (uint32_t s = 0; s < S; ++s) {
            const Scenario &sc = run.scen[s];
            pen_count[s] = (uint32_t)sc.pens.size();
            ev_count[s] = (uint32_t)sc.evs.size();
            pace_count[s] = (uint32_t)sc.offs.size();
            for (const mcgp_time_penalty &p : sc.pens) {
                pens.push_back(p);
                if (p.kind == MCGP_PEN_SERVE_AT_STOP) serve_mask[s] |= 1u << p.driver;
            }
            for (const mcgp_lap_event &e : sc.evs) evs.push_back(e);
            for (const mcgp_pace_offset &o : sc.offs) {
                offs.push_back(o);
                if (o.kind == MCGP_PACE_UNTIL_STOP) until_mask[s] |= 1u << o.driver;
            }
        }
        mcgp_pit_plan plan = {};
        plan.driver = 0;
        plan.start_compound = -1;
        plan.n_stops = 1;
        plan.stop_lap[0] = L;
        plan.stop_compound[0] = MCGP_HARD;
        if (run.planned >= 0) plan_count[run.planned] = 1;

        const uint64_t m = run.sims;
        const size_t w = 2 * (size_t)n - 1, row_cells = (size_t)L + 1;
        std::unique_ptr<unsigned long long[]> hist(new unsigned long long[S * n * n]()), delta(new unsigned long long[S * n * w]()),
            fate(new unsigned long long[S * n * 4]()), ev_cnt(new unsigned long long[S * 3 * row_cells]()),
            counted(new unsigned long long[S * n * row_cells]());
        std::unique_ptr<uint8_t[]> stage(new uint8_t[S * m * n]);
        std::unique_ptr<uint32_t[]> ev_stage(new uint32_t[S * m]);
        std::unique_ptr<uint16_t[]> car(new uint16_t[S * m * n]);
        for (size_t k = 0; k < S * m * n; ++k) car[k] = 0xEEEE;
        const char *err = "";
        const bool nul = run.null_counts;
        const int rc = emu_combined_run(&cfg, &drv, grid.data(), nullptr, n, S, plan_count.data(), &plan,
                                        nul ? nullptr : pen_count.data(), pens.empty() ? nullptr : pens.data(),
                                        nul ? nullptr : ev_count.data(), evs.empty() ? nullptr : evs.data(),
                                        nul ? nullptr : pace_count.data(), offs.empty() ? nullptr : offs.data(), m, 1000, 77,
                                        hist.get(), stage.get(), ev_stage.get(), car.get(), delta.get(), fate.get(), ev_cnt.get(),
                                        counted.get(), 3, &err);
        if (rc != MCGP_OK) FAIL("n = %u, %d laps: rc %d: %s", n, L, rc, err);
        std::vector<unsigned long long> seen_c(S * n * row_cells, 0), seen_f(S * n * 4, 0), seen_e(S * 3 * row_cells, 0);
        for (uint32_t s = 0; s < S; ++s)
            for (uint64_t i = 0; i < m; ++i) {
                const uint8_t *row = stage.get() + (s * m + i) * n;
                const uint16_t *crow = car.get() + (s * m + i) * n;
                uint32_t seen = 0;
                for (uint32_t d = 0; d < n; ++d) {
                    const uint32_t pos = row[d] & 31u, f = row[d] >> 5;
                    const bool serves = (serve_mask[s] >> d) & 1u, has = (until_mask[s] >> d) & 1u;
                    if (pos >= n || f > 3 || (f != 0) != serves)
                        FAIL("n = %u, %d laps, scenario %u, simulation %llu, driver %u: byte %u", n, L, s, (unsigned long long)i,
                             d, row[d]);
                    seen |= 1u << pos;
                    if (f) seen_f[((size_t)s * n + d) * 4 + f] += 1;                                // column 0 is the host's
                    if (has ? crow[d] > (uint32_t)L : crow[d] != 0xEEEE)
                        FAIL("n = %u, %d laps, scenario %u, simulation %llu, driver %u: laps carried %u", n, L, s,
                             (unsigned long long)i, d, crow[d]);
                    if (has && crow[d]) seen_c[((size_t)s * n + d) * row_cells + crow[d]] += 1;     // column 0 is the host's
                }
                if (seen != (n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u))
                    FAIL("n = %u, scenario %u, simulation %llu: not a permutation", n, s, (unsigned long long)i);
                const uint32_t packed = ev_stage[s * m + i];
                uint32_t total = 0;
                for (uint32_t k = 0; k < 3; ++k) {
                    const uint32_t c = (packed >> (10 * k)) & 1023u;
                    total += c;
                    seen_e[((size_t)s * 3 + k) * row_cells + (c < (uint32_t)L ? c : (uint32_t)L)] += 1;
                }
                if ((packed >> 30) || total > (uint32_t)(L - 1))
                    FAIL("n = %u, %d laps, scenario %u, simulation %llu: event counts %08x", n, L, s, (unsigned long long)i, packed);
                // nobody retires and driver 0's only stop is on lap L: it serves there, and its offset from lap 2 clears
                if ((int)s == run.planned && !run.retirements && ((row[0] >> 5) != 1 || crow[0] != (uint32_t)(L - 1)))
                    FAIL("%d laps, scenario %u, simulation %llu: fate %u, carried %u laps", L, s, (unsigned long long)i,
                         row[0] >> 5, crow[0]);
            }
        for (size_t k = 0; k < (size_t)S * n * row_cells; ++k)
            if (counted[k] != seen_c[k]) FAIL("n = %u, %d laps: carried cell %zu: counted %llu, staged %llu", n, L, k, counted[k], seen_c[k]);
        for (size_t k = 0; k < (size_t)S * n * 4; ++k)
            if (fate[k] != seen_f[k]) FAIL("n = %u, %d laps: fate cell %zu: counted %llu, staged %llu", n, L, k, fate[k], seen_f[k]);
        for (size_t k = 0; k < (size_t)S * 3 * row_cells; ++k)
            if (ev_cnt[k] != seen_e[k]) FAIL("n = %u, %d laps: events cell %zu: counted %llu, staged %llu", n, L, k, ev_cnt[k], seen_e[k]);
    }
    std::puts("ok");
    return 0;
}
