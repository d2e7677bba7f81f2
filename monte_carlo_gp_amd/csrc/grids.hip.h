// grids.hip.h -- race odds under edits of the starting grid (mcgp_run_grids, include/mcgp.h).
//
// The table and the policy of the grid rule set of race_scenario_kernel (scenario.hip.h: S scenarios of one race with
// common random numbers, one lane per (scenario, simulation), blockIdx.y the scenario), and grid_count.  The rule set is
// one policy, GridEdits, in the grid slot of start_from_grid (race_kernel.hip.h):
//
//   edit    after the sampling loop every driver d holds its drawn slot s_d in its pk word.  The pit-lane drivers take the
//           last slots in the order of their s_d, the pinned drivers their slots, and every other driver is ranked by
//           (s_d + drop_d, s_d) and takes the free slot of its rank.  Then the cars are set up by the new slot -- the
//           model's start tyres of the slot, the plan's after them, the slot in pk, the driver in ord -- so that lap 1
//           (its position factor and its top-three clip read the slot) and every sort run on the edited grid;
//   lap1    a pit-lane car that sets a lap time on lap 1 gets t = (0.0 + lap_time) + seconds.
//
// The edit step runs once per race on the lane's own LDS rows.  `out` is free until the retirement draws at the end of
// the start and holds one u16 key per driver: kGridPlaced | slot for a pit-lane or pinned driver, else
// (s_d + drop_d) << 5 | s_d, which is unique and orders the others as specified, so a driver's rank is the number of
// smaller keys: n reads of `out` per driver.  The rank's free slot is found in the scenario's wave-uniform mask of free
// slots by clearing its `rank` lowest bits.  The loops run over the driver index, so every read of the table in the edit
// step is at a wave-uniform address; only lap1 reads by the lane's driver, and only a pit-lane car's seconds, as
// OffsetPace fetches its seconds.  A scenario without edits (GridScenario::edits == 0, wave-uniform: a block serves one
// scenario) skips the step and its lap1 tests an all-zero mask.  The rule set has no per-lane state beside the staging.
// Nothing new is drawn and no draw moves: the grid words are drawn as before, and lap 1's words are keyed by driver.
//
// The table reaches the kernel through the argument of a rule set this instantiation never meets (`pens`), as the
// weather tables do.
//
// Staging: the strategy call's byte per scenario, simulation and driver (the classified position; strategy_count_deltas
// counts the deltas) and, when start_out or gain_out is wanted, one u16 per scenario, simulation and driver: the start
// slot after the edits, read back from the pk word at the flag.  grid_count reads both once, blockIdx.y the scenario,
// blockIdx.z the driver, into n + 2n - 1 u32 LDS bins: the start slots, then (start slot - classified position) + n - 1.
// One u64 global atomic per non-zero bin.  It has no cross-lane operation and strides by its block's size.
// Overflow: a launch is at most max_sims_per_launch() < 2^32 simulations per scenario, so no u32 bin can wrap.
//
// Registers: race_scenario_kernel<false, kRuleGrid> has 131 VGPRs (occupancy 3 by registers, where the paces and weather
// instantiations are; <false, 0> has 123) and no scratch; its launch is shaped by LDS, as the whole family's.  The edit
// step as a real function has 127 VGPRs but 64 bytes of scratch per lane (profiles/grid_time.txt).
//
// Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five with max - min;
// profiles/grid_time.txt): two empty scenarios 98.20 (0.15) against 97.65 (0.20) for mcgp_run_strategies
// built from the parent commit; an empty scenario and a ten-place drop of one driver 98.27 (0.51); an empty scenario and
// a pit-lane start with start_out and gain_out wanted 99.31 (0.49).
#pragma once
#include "strategy.hip.h"

namespace mcgp {

constexpr int kGridDrop = 0, kGridPin = 1, kGridPitLane = 2;   // MCGP_GRID_DROP .. MCGP_GRID_PIT_LANE
constexpr uint32_t kMaxGridDrop = 255u;
constexpr double kMaxPitLaneSeconds = 1e6;
constexpr uint32_t kGridPlaced = 0x8000u;                   // a key in `out`: the slot is in its low five bits
constexpr int kGridKeyShift = 5;                            // else (s + drop) << 5 | s
constexpr int kGridCountBlock = 256;                        // threads of a counting block
static_assert(((kMaxCars - 1 + kMaxGridDrop) << kGridKeyShift | (kMaxCars - 1)) < kGridPlaced, "a key fits below the flag");

// One scenario's edits in device memory.
struct GridScenario {
    uint32_t edits;                 // their number; 0: the drawn grid stands
    uint32_t pit, pin;              // bit d: driver d starts from the pit lane / is pinned
    uint32_t free_slots;            // bit p: slot p is neither pinned nor a pit-lane slot
    uint8_t value[kMaxCars];        // driver d's places to drop (0: none), or its pinned slot (0-based)
    double seconds[kMaxCars];       // a pit-lane driver's seconds
};

// The grid policy of a scenario with edits (ModelGrid, race_kernel.hip.h, is the model's).
struct GridEdits {
    static constexpr bool kEdits = true;
    const GridScenario *__restrict__ g;
    uint32_t pit;                               // GridScenario::pit

    template <class StartHook>
    __device__ __forceinline__ void edit(const Rows &s, int n, int track, StartHook hook) const
    {
        if (!g->edits) return;                  // wave-uniform
        const uint32_t pin = g->pin, free_slots = g->free_slots;
        const uint32_t first_pit = (uint32_t)n - (uint32_t)__popc(pit);
        for (int d = 0; d < n; ++d) {
            const uint32_t bit = 1u << d, sd = gpos_of(s.Pk((uint32_t)d)), v = g->value[d];
            uint32_t key;
            if (pit & bit) {
                uint32_t slot = first_pit;
                for (uint32_t rest = pit & ~bit; rest; rest &= rest - 1u)
                    slot += gpos_of(s.Pk((uint32_t)__ffs((int)rest) - 1u)) < sd;
                key = kGridPlaced | slot;
            } else if (pin & bit) {
                key = kGridPlaced | v;
            } else {
                key = ((sd + v) << kGridKeyShift) | sd;
            }
            s.Out((uint32_t)d) = (uint16_t)key;
        }
        for (int d = 0; d < n; ++d) {
            const uint32_t key = s.Out((uint32_t)d);
            uint32_t slot = key & 31u;
            if (!(key & kGridPlaced)) {
                uint32_t rest = free_slots;
                for (int o = 0; o < n; ++o)
                    if (s.Out((uint32_t)o) < key) rest &= rest - 1u;
                slot = (uint32_t)__ffs((int)rest) - 1u;
            }
            uint32_t comp, age;
            start_tyres(track, (int)slot, comp, age);
            hook((uint32_t)d, comp, age);
            s.Pk((uint32_t)d) = age | (comp << kCompShift) | ((1u << comp) << kUsedShift) | (slot << kGposShift);
            s.Ord((int)slot) = (uint8_t)d;
        }
    }
    __device__ __forceinline__ double lap1(uint32_t d, double t) const
    {
        if ((pit >> d) & 1u) t = t + g->seconds[d];
        return t;
    }
};

// From the staged bytes and u16 of m simulations, for driver d = blockIdx.z of scenario s = blockIdx.y: start_out
// [S][n][n] += the simulations in which it started from that slot, gain_out [S][n][2n - 1] += those in which (start slot -
// classified position) + n - 1 was that column; either may be NULL.  u32 LDS bins per block, one u64 global atomic per
// non-zero bin; any block size.
__global__ void __launch_bounds__(kGridCountBlock)
grid_count(const uint8_t *__restrict__ stage, const uint16_t *__restrict__ start, uint64_t m, uint32_t n,
           unsigned long long *__restrict__ start_out, unsigned long long *__restrict__ gain_out)
{
    __shared__ uint32_t bins[kMaxCars + 2 * kMaxCars - 1];
    const uint32_t t = threadIdx.x, nt = blockDim.x, s = blockIdx.y, d = blockIdx.z, w = 2u * n - 1u, n_bins = n + w;
    if (d >= n) return;
    for (uint32_t i = t; i < n_bins; i += nt) bins[i] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)s * m * n;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt) {
        const uint32_t slot = start[base + i * n + d], pos = stage[base + i * n + d];
        if (slot < n && pos < n) {              // (always: the race kernel wrote both)
            atomicAdd(&bins[slot], 1u);
            atomicAdd(&bins[n + (slot + n - 1u - pos)], 1u);
        }
    }
    __syncthreads();
    if (start_out) flush_bins(bins, n, start_out + ((uint64_t)s * n + d) * n, t, nt);
    if (gain_out) flush_bins(bins + n, w, gain_out + ((uint64_t)s * n + d) * w, t, nt);
}

}  // namespace mcgp
