// strategy.hip.h -- race odds under planned pit stops (mcgp_run_strategies, include/mcgp.h): the tables and policies of a
// planned race, and what every scenario call's counting kernel shares.  The race kernel of all five scenario calls is
// race_scenario_kernel (scenario.hip.h); mcgp_run_strategies runs it with no rule set beside the plans.
//
// A scenario call runs S scenarios of one race with common random numbers: simulation i of every scenario draws what
// mcgp_run's (from the grid) or mcgp_run_from_state's (from a state) simulation i draws.  The plans are two hooks of the
// generic kernel's code:
//
//   start   a PlannedTyres hook for start_from_grid: a planned driver's starting compound and age (grid runs only);
//   stops   a PlanPit policy for run_laps: a planned driver never takes the model's rule; on a lap of its plan it
//           stops where the rule's stop would happen (after its lap time, before overtakes, only if still running).
//
// A scenario's plans reach the kernel as global memory, not LDS: a StrategyScenario (the planned-driver mask and the start
// table) and a StopLap per lap (the drivers stopping on that lap and their new compounds).  begin_lap reads the lap's stop
// mask once per lap at a wave-uniform address, so the stop test of a car-lap is two bit tests on registers; only a car
// that stops reads its compound, and the start table is read once per car and race.
//
// Counts: classify_and_count's u32 LDS histogram goes to hist[scenario][n][n] with u64 atomics, and each lane writes its
// classified position per driver, one byte, into a staging buffer [S][m][n] that strategy_count_deltas reads.  That
// kernel counts pos_s(d) - pos_0(d) for scenarios s >= 1 into u32 LDS bins (count_position_deltas) and adds them into
// delta[s][d][2n - 1] with u64 atomics (flush_bins); the centre bin (no change) is not counted on the device: the host
// sets it to n_sims minus the rest.  The counting kernels of the other calls (penalties_count, events_count, paces_count)
// count their deltas and flush their bins through the same two functions.
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

// The paired changes of position of one simulation, scenario s against scenario 0, from its staged bytes r0 [n] (scenario
// 0) and r1 [n] (scenario s) into the block's u32 LDS bins [n][2n - 1]: driver d adds one at (pos_s(d) - pos_0(d)) + n - 1,
// except at the centre (no change).  `mask` takes the position out of a staged byte.  seen(d, byte) is handed scenario
// s's byte of every driver in the same pass (penalties_count reads the fate above the position there; `deltas` false:
// only that).  One thread's work on its own simulation: no cross-lane operation, and the caller's loop over the
// simulations strides by its block's size (the emulator runs these kernels as blocks of one thread).
struct NoByteSeen {
    __device__ __forceinline__ void operator()(uint32_t /*d*/, uint32_t /*byte*/) const {}
};

template <class Seen = NoByteSeen>
__device__ __forceinline__ void count_position_deltas(const uint8_t *r0, const uint8_t *r1, uint32_t n, uint32_t mask,
                                                      uint32_t *bins, bool deltas = true, Seen seen = Seen())
{
    const uint32_t w = 2u * n - 1u;
    for (uint32_t d = 0; d < n; ++d) {
        const uint32_t b1 = r1[d], p1 = b1 & mask;
        if (deltas) {
            const uint32_t p0 = r0[d] & mask;
            if (p0 != p1) atomicAdd(&bins[d * w + (p1 + n - 1u - p0)], 1u);
        }
        seen(d, b1);
    }
}

// out[i] += bins[i] for the block's non-zero u32 LDS bins, one u64 global atomic each, by thread t of the block's nt.  No
// cross-lane operation; strides by the block's size.
__device__ __forceinline__ void flush_bins(const uint32_t *bins, uint32_t n_bins, unsigned long long *out, uint32_t t,
                                           uint32_t nt)
{
    for (uint32_t i = t; i < n_bins; i += nt)
        if (bins[i]) atomicAdd(&out[i], (unsigned long long)bins[i]);
}

// delta [S][n][2n - 1] += the staged positions' paired changes against scenario 0, for scenario s = blockIdx.y + 1 and
// each of the m simulations; the centre (no change) is left out: the host derives it.
__global__ void __launch_bounds__(kStrategyCountBlock)
strategy_count_deltas(const uint8_t *__restrict__ stage, uint64_t m, uint32_t n, unsigned long long *__restrict__ delta)
{
    __shared__ uint32_t bins[kMaxCars * (2 * kMaxCars - 1)];
    const uint32_t t = threadIdx.x, nt = kStrategyCountBlock, s = blockIdx.y + 1u, w = 2u * n - 1u, n_bins = n * w;
    for (uint32_t i = t; i < n_bins; i += nt) bins[i] = 0u;
    __syncthreads();
    const uint8_t *base = stage + (uint64_t)s * m * n;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt)
        count_position_deltas(stage + i * n, base + i * n, n, 0xFFu, bins);
    __syncthreads();
    flush_bins(bins, n_bins, delta + (uint64_t)s * n * w, t, nt);
}

}  // namespace mcgp
