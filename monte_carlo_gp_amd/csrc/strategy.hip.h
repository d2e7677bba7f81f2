// strategy.hip.h -- race odds under planned pit stops (mcgp_run_strategies, include/mcgp.h).
//
// race_strategy_kernel runs S scenarios of one race with common random numbers: simulation i of every scenario draws
// what mcgp_run's (from the grid) or mcgp_run_from_state's (from a state) simulation i draws.  It is the generic kernel's
// code -- start_from_grid or start_from_state, run_laps, classify_and_count -- with two hooks:
//
//   start   a PlannedTyres hook for start_from_grid: a planned driver's starting compound and age (grid runs only);
//   stops   a PlanPit policy for run_laps: a planned driver never takes the model's rule; on a lap of its plan it
//           stops where the rule's stop would happen (after its lap time, before overtakes, only if still running).
//
// Layout: one lane runs one (scenario, simulation) pair in race_kernel's LDS rows; a block serves one scenario
// (blockIdx.y) and grid-strides over its simulations in batches of blockDim.x.  A scenario's plans reach the kernel as
// global memory, not LDS: a StrategyScenario (the planned-driver mask and the start table) and a StopLap per lap (the
// drivers stopping on that lap and their new compounds).  begin_lap reads the lap's stop mask once per lap at a
// wave-uniform address, so the stop test of a car-lap is two bit tests on registers; only a car that stops reads its
// compound, and the start table is read once per car and race.
//
// Counts: classify_and_count's u32 LDS histogram goes to hist[scenario][n][n] with u64 atomics, and each lane writes its
// classified position per driver, one byte, into a staging buffer [S][m][n] that strategy_count_deltas reads.  That
// kernel counts pos_s(d) - pos_0(d) for scenarios s >= 1 into u32 LDS bins and adds them into delta[s][d][2n - 1] with
// u64 atomics; the centre bin (no change) is not counted on the device: the host sets it to n_sims minus the rest.
// Overflow: a launch is at most max_sims_per_launch() < 2^32 simulations per scenario, so no u32 bin can wrap.
#pragma once
#include "resume.hip.h"

namespace mcgp {

constexpr uint32_t kMaxStrategyScenarios = 64;
constexpr int kMaxPlanStops = 8;
constexpr uint16_t kModelStart = 0xFFFFu;       // StrategyScenario::start: the model's starting tyres
constexpr int kStrategyCountBlock = 256;        // threads of a counting block

// One scenario in device memory.
struct StrategyScenario {
    uint32_t planned;               // bit d: driver d has a plan (the model's rule is off for it)
    uint32_t pad;
    uint16_t start[kMaxCars];       // kModelStart, or compound | age << 3 (grid runs)
};

// The stops of one scenario on one lap: 32 bytes, one scalar load.
struct StopLap {
    uint32_t mask;                  // bit d: driver d stops on this lap
    uint32_t comp[4];               // driver d's new compound: nibble d & 7 of comp[d >> 3]
    uint32_t pad[3];
};

// run_laps' pit policy for one scenario: the rule for unplanned drivers, the plan for the others.  Per lap it holds one
// wave-uniform word (the drivers stopping on the lap); a stopping car reads its compound from the lap's StopLap.
struct PlanPit {
    const StopLap *__restrict__ laps;   // this scenario's [L + 1]
    uint32_t planned;
    uint32_t mask;                      // the current lap's StopLap::mask
    int lap;

    __device__ __forceinline__ void begin_lap(int l)
    {
        lap = l;
        mask = laps[l].mask;
    }
    __device__ __forceinline__ int decide(uint32_t d, uint32_t &newc) const
    {
        if (!((planned >> d) & 1u)) return -1;
        if (!((mask >> d) & 1u)) return 0;
        newc = (laps[lap].comp[d >> 3] >> (4u * (d & 7u))) & 7u;
        return 1;
    }
    __device__ __forceinline__ double after_pit(uint32_t /*d*/, bool /*stopped*/, double t) const { return t; }
};

// start_from_grid's hook for one scenario: a planned driver's starting compound and age.
struct PlannedTyres {
    const StrategyScenario *__restrict__ sc;

    __device__ __forceinline__ void operator()(uint32_t driver, uint32_t &comp, uint32_t &age) const
    {
        const uint32_t o = sc->start[driver];
        if (o != kModelStart) { comp = o & 7u; age = o >> 3; }
    }
};

// Simulations sim_offset + [0, m) of every scenario (gridDim.y = S), from the grid (kFromState false) or from `state`.
// hist [S][n][n] is ACCUMULATED into; stage [S][m][n] is written (classified position of each driver).
template <bool kFromState>
__global__ void __launch_bounds__(512)
race_strategy_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state,
                     const StrategyScenario *__restrict__ scen, const StopLap *__restrict__ stop_laps, uint64_t m,
                     uint64_t sim_offset, uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist,
                     uint8_t *__restrict__ stage, uint32_t n_batches)
{
    const uint32_t sid = blockIdx.y;
    const StrategyScenario *__restrict__ sc = scen + sid;
    const PlanPit pit = {stop_laps + (size_t)sid * (size_t)(P->total_laps + 1), sc->planned, 0u, 0};
    run_block(P, m, n_batches, hist + (size_t)sid * (size_t)(P->n * P->n),
              [=](const Rows &s, const LapEnv &e, uint32_t *s_hist, uint64_t local) {
        const uint64_t sim = sim_offset + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);
        const RaceStart at = kFromState ? start_from_state(s, e, *state, c0, c1, seed_lo, seed_hi)
                                        : start_from_grid(s, e, c0, c1, seed_lo, seed_hi, nullptr, PlannedTyres{sc});
        NoLapObserver none;
        run_laps(s, e, c0, c1, seed_lo, seed_hi, at.first_lap, at.drs_disabled_until, none, pit);   // reference :166-228
        classify_and_count(s, e.n, s_hist, nullptr);                                                // reference :230-242
        // each driver's classified position
        uint8_t *row = stage + ((uint64_t)sid * m + local) * (uint64_t)e.n;
        for (int p = 0; p < e.n; ++p) row[s.Ord(p)] = (uint8_t)p;
    });
}

// delta [S][n][2n - 1] += the staged positions' paired changes against scenario 0: for scenario s = blockIdx.y + 1 and
// each of the m simulations, driver d adds one at (pos_s(d) - pos_0(d)) + n - 1, except at the centre (no change),
// which the host derives.  u32 LDS bins per block, one u64 global atomic per non-zero bin.
__global__ void __launch_bounds__(kStrategyCountBlock)
strategy_count_deltas(const uint8_t *__restrict__ stage, uint64_t m, uint32_t n, unsigned long long *__restrict__ delta)
{
    __shared__ uint32_t bins[kMaxCars * (2 * kMaxCars - 1)];
    const uint32_t t = threadIdx.x, s = blockIdx.y + 1u, w = 2u * n - 1u;
    for (uint32_t i = t; i < n * w; i += kStrategyCountBlock) bins[i] = 0u;
    __syncthreads();
    const uint8_t *base = stage + (uint64_t)s * m * n;
    for (uint64_t i = (uint64_t)blockIdx.x * kStrategyCountBlock + t; i < m; i += (uint64_t)gridDim.x * kStrategyCountBlock) {
        const uint8_t *r0 = stage + i * n, *r1 = base + i * n;
        for (uint32_t d = 0; d < n; ++d) {
            const uint32_t p0 = r0[d], p1 = r1[d];
            if (p0 != p1) atomicAdd(&bins[d * w + (p1 + n - 1u - p0)], 1u);
        }
    }
    __syncthreads();
    unsigned long long *out = delta + (uint64_t)s * n * w;
    for (uint32_t i = t; i < n * w; i += kStrategyCountBlock)
        if (bins[i]) atomicAdd(&out[i], (unsigned long long)bins[i]);
}

}  // namespace mcgp
