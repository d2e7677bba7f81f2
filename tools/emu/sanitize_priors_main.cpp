// sanitize_priors_main.cpp -- a stand-alone program over the host DEBUGGING build of the pace-uncertainty kernels and
// their packer (csrc/prior_pack.h), for the host's sanitizers (not product code).  Compiled together with emu_generic.cpp:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
//       -static-libubsan -pthread -fno-sanitize=alignment -ffp-contract=off -Itools/emu \
//       tools/emu/sanitize_priors_main.cpp tools/emu/emu_generic.cpp -o san_priors
//
// (-fno-sanitize=alignment for the reason given in sanitize_bonus_main.cpp: a block of one thread.)  It runs
// emu_priors_run (race_scenario_kernel<false, kRulePriors>, then priors_count as blocks of one thread) at the limits: 64
// scenarios of 64 items on 32 cars with 15 edges; 1000 laps on 2 cars; a race of one lap without edges; one group of all
// 32 drivers; and 5 cars without the offsets staged; every buffer on the heap at exactly its size.  It checks that every
// staged row is a permutation, that every staged bin is the number of edges not above the staged offset, that a driver
// without an item has offset +0, that the members of the all-driver group share one offset, and that the counted
// [bin][position] cells are the staged ones.  Exit status 0 and "ok" when every call returned MCGP_OK and the sanitizers
// found nothing.  tests/test_priors_sanitize.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/mcgp.h"

extern "C" int emu_priors_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                              const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                              const mcgp_pit_plan *plans, const uint32_t *prior_count, const mcgp_pace_prior *priors,
                              uint32_t n_edges, const double *edges, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                              unsigned long long *hist, uint8_t *stage, uint8_t *bin_stage, float *off_stage,
                              unsigned long long *delta, unsigned long long *draws, uint32_t grid_x, const char **err);

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
    std::vector<double> edges;
    std::vector<std::vector<mcgp_pace_prior>> scen;     // the items of every scenario
    bool offsets;                                       // the offsets are staged
    int one_group;                                      // scenario whose drivers all share one group and nothing else, or -1
};

mcgp_pace_prior own(int d, double s) { return {MCGP_PRIOR_DRIVER, d, 0u, 0u, s}; }
mcgp_pace_prior group(uint32_t members, double s) { return {MCGP_PRIOR_GROUP, 0, members, 0u, s}; }

}  // namespace

int main()
{
    std::vector<Run> runs;
    {   // 64 scenarios x 64 items (an own item and a group of one per driver), 32 cars, 15 edges
        Run r = {32, 12, 3, {}, {}, true, -1};
        for (int e = 0; e < MCGP_MAX_PRIOR_EDGES; ++e) r.edges.push_back(-0.35 + 0.05 * e);
        for (int s = 0; s < 64; ++s) {
            std::vector<mcgp_pace_prior> it;
            for (int d = 0; d < 32; ++d) it.push_back(own(d, 0.01 * ((s + d) % 40)));
            for (int d = 0; d < 32; ++d) it.push_back(group(1u << ((d + s) % 32), 0.02 * ((s * 7 + d) % 11)));
            r.scen.push_back(it);
        }
        runs.push_back(r);
    }
    // 1000 laps, 2 cars: a pair group and an own item, the largest sigma
    runs.push_back({2, 1000, 2, {-0.3, -0.1, 0.0, 0.1, 0.3}, {{}, {group(3u, 0.2), own(1, 10.0)}}, true, -1});
    // one lap, no edges
    runs.push_back({3, 1, 40, {}, {{}, {own(0, 1.5), group(6u, 1.0)}}, true, -1});
    // one group of all 32 drivers; groups whose lowest members are 4 and 28 beside own items
    runs.push_back({32, 20, 24, {0.0}, {{group(0xFFFFFFFFu, 0.3)},
                                       {group(1u << 4 | 1u << 9 | 1u << 31, 0.2), group(3u << 28, 0.4), own(9, 0.15), own(28, 0.05)}},
                    true, 0});
    // 5 cars, the offsets not staged
    runs.push_back({5, 30, 50, {-0.1, 0.1}, {{}, {own(0, 0.2), own(4, 0.0), group(1u << 1 | 1u << 3, 0.3)}}, false, -1});
    for (const Run &run : runs) {
        const uint32_t n = run.n, S = (uint32_t)run.scen.size(), E = (uint32_t)run.edges.size(), B = E + 1;
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

        std::vector<mcgp_pace_prior> items;
        std::vector<uint32_t> prior_count(S, 0), plan_count(S, 0), touched(S, 0);
        for (uint32_t s = 0; s < S; ++s) {
            prior_count[s] = (uint32_t)run.scen[s].size();
            for (const mcgp_pace_prior &it : run.scen[s]) {
                items.push_back(it);
                touched[s] |= it.kind == MCGP_PRIOR_DRIVER ? 1u << it.driver : it.members;
            }
        }
        const uint64_t m = run.sims;
        const size_t w = 2 * (size_t)n - 1, cells = (size_t)S * m * n;
        std::unique_ptr<unsigned long long[]> hist(new unsigned long long[S * n * n]()), delta(new unsigned long long[S * n * w]()),
            draws(new unsigned long long[(size_t)S * n * B * n]());
        std::unique_ptr<uint8_t[]> stage(new uint8_t[cells]), bins(new uint8_t[cells]);
        std::unique_ptr<float[]> offs(run.offsets ? new float[cells] : nullptr);
        std::unique_ptr<double[]> edges(E ? new double[E] : nullptr);
        for (uint32_t e = 0; e < E; ++e) edges[e] = run.edges[e];
        std::memset(bins.get(), 0xEE, cells);
        const char *err = "";
        const int rc = emu_priors_run(&cfg, &drv, grid.data(), nullptr, n, S, plan_count.data(), nullptr, prior_count.data(),
                                      items.empty() ? nullptr : items.data(), E, edges.get(), m, 0xFFFFFFFFull - 1, 77ull << 32 | 5,
                                      hist.get(), stage.get(), bins.get(), offs.get(), delta.get(), draws.get(), 3, &err);
        if (rc != MCGP_OK) {
            std::fprintf(stderr, "n = %u, %d laps: rc %d: %s\n", n, L, rc, err);
            return 1;
        }
        std::vector<unsigned long long> seen_c((size_t)S * n * B * n, 0);
        for (uint32_t s = 0; s < S; ++s)
            for (uint64_t i = 0; i < m; ++i) {
                const size_t at = ((size_t)s * m + i) * n;
                uint32_t seen = 0;
                for (uint32_t d = 0; d < n; ++d) {
                    const uint32_t pos = stage[at + d], bin = bins[at + d];
                    if (pos >= n || bin >= B) {
                        std::fprintf(stderr, "n = %u, %d laps, scenario %u, simulation %llu, driver %u: position %u, bin %u\n", n,
                                     L, s, (unsigned long long)i, d, pos, bin);
                        return 1;
                    }
                    seen |= 1u << pos;
                    seen_c[(((size_t)s * n + d) * B + bin) * n + pos] += 1;
                    if (!run.offsets) continue;
                    const float x = offs[at + d];
                    uint32_t want = 0, bits;
                    std::memcpy(&bits, &x, 4);
                    for (uint32_t e = 0; e < E; ++e) want += edges[e] <= (double)x;
                    const bool free_of_items = !((touched[s] >> d) & 1u);
                    if (want != bin || !(x == x) || (free_of_items && bits != 0u) ||
                        ((int)s == run.one_group && x != offs[at])) {
                        std::fprintf(stderr, "n = %u, %d laps, scenario %u, simulation %llu, driver %u: offset %g, bin %u\n", n, L,
                                     s, (unsigned long long)i, d, (double)x, bin);
                        return 1;
                    }
                }
                if (seen != (n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u)) {
                    std::fprintf(stderr, "n = %u, scenario %u, simulation %llu: not a permutation\n", n, s, (unsigned long long)i);
                    return 1;
                }
            }
        for (size_t k = 0; k < seen_c.size(); ++k)
            if (draws[k] != seen_c[k]) {
                std::fprintf(stderr, "n = %u, %d laps: draws cell %zu: counted %llu, staged %llu\n", n, L, k, draws[k], seen_c[k]);
                return 1;
            }
    }
    std::puts("ok");
    return 0;
}
