// events.hip.h -- race odds with the race-interrupting events of chosen laps set by the caller (mcgp_run_events,
// include/mcgp.h).
//
// The policies of the events rule set of race_scenario_kernel (scenario.hip.h: S scenarios of one race with common
// random numbers, one lane per (scenario, simulation), blockIdx.y the scenario), and events_count.  The rule set is an
// event policy for run_laps and a lap observer that counts the events:
//
//   events   ForcedEvents: one byte per scenario and lap, [S][L + 1] in global memory: 0 = the lap's event is drawn,
//            1 + kEvent* = that outcome replaces the short-circuit chain's.  run_laps reads the lap's byte once, at a
//            wave-uniform address (as PlanPit reads the lap's StopLap), before the event step.  A forced event runs the
//            drawn one's handler: same bunching, same tyre step (a VSC's age decrement still hangs on word 3 of the
//            lap's event block), same drs_disabled_until, same re-sort after a tie.  The lap's Philox block is computed
//            on every lap, forced or not: skipping it where it goes unread would save one block of about 25 per lap.
//   counts   PackedEventCounter: the lap's kEvent* as run_laps hands it over (forced and drawn alike, whether or not a car
//            still runs), three counters of 10 bits in one register (a race has at most kMaxLaps - 1 = 999 event laps).
//
// Nothing new is drawn and no other draw moves, so a scenario without overrides is mcgp_run_strategies' scenario cell
// for cell.
//
// Staging: the strategy call's byte per scenario, simulation and driver (the classified position), and one u32 per
// scenario and simulation (red flags | safety cars << 10 | VSCs << 20).  events_count reads both once, blockIdx.y the
// scenario: pos_s(d) - pos_0(d) for scenarios s >= 1 (count_position_deltas, strategy.hip.h: the centre bin left out) and
// the three event counts into u32 LDS bins, [n][2n - 1] + [3][L + 1] (20 KB at n = 32, L = 1000), then one u64 global
// atomic per non-zero bin (flush_bins).  It has no cross-lane operation and strides by its block's size.
// Overflow: a launch is at most max_sims_per_launch() < 2^32 simulations per scenario, so no u32 bin can wrap.
#pragma once
#include "strategy.hip.h"

namespace mcgp {

constexpr uint32_t kMaxScenarioEvents = 64;
constexpr int kEventCountBits = 10;             // PackedEventCounter: bits per kind
constexpr uint32_t kEventCountMask = (1u << kEventCountBits) - 1u;
constexpr int kEventsCountBlock = 256;          // threads of a counting block
static_assert(kMaxLaps - 1 <= (int)kEventCountMask, "a race's event laps fit a counter");

// run_laps' event policy for one scenario: the caller's override of a lap, or -1 (drawn).
struct ForcedEvents {
    const uint8_t *__restrict__ laps;   // this scenario's [L + 1]: 0 = drawn, 1 + kEvent* otherwise

    __device__ __forceinline__ int at(int lap) const { return (int)laps[lap] - 1; }
};

// run_laps' observer: the lane's events so far, red flags | safety cars << 10 | VSCs << 20.
struct PackedEventCounter {
    uint32_t packed;

    __device__ __forceinline__ void operator()(const Rows &, int /*lap*/, int event)
    {
        if (event != kEventNone) packed += 1u << (kEventCountBits * (event - 1));
    }
};

// From the staged data of m simulations: for scenario s = blockIdx.y, delta [S][n][2n - 1] += the paired changes of
// position against scenario 0 (s >= 1, the centre left out; delta may be NULL) and events [S][3][L + 1] += the
// simulations with that many red flags / safety cars / VSCs (events may be NULL).  u32 LDS bins per block, one u64
// global atomic per non-zero bin; any block size.
__global__ void __launch_bounds__(kEventsCountBlock)
events_count(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ ev_stage, uint64_t m, uint32_t n, uint32_t L,
             unsigned long long *__restrict__ delta, unsigned long long *__restrict__ events)
{
    __shared__ uint32_t bins[kMaxCars * (2 * kMaxCars - 1) + 3 * (kMaxLaps + 1)];
    const uint32_t t = threadIdx.x, nt = blockDim.x, s = blockIdx.y;
    const uint32_t n_delta = n * (2u * n - 1u), n_ev = 3u * (L + 1u), n_bins = n_delta + n_ev;
    const bool want_delta = delta != nullptr && s > 0u;
    for (uint32_t i = t; i < n_bins; i += nt) bins[i] = 0u;
    __syncthreads();
    const uint8_t *base = stage + (uint64_t)s * m * n;
    const uint32_t *ev = ev_stage + (uint64_t)s * m;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt) {
        if (want_delta) count_position_deltas(stage + i * n, base + i * n, n, 0xFFu, bins);
        if (events) {
            const uint32_t r = ev[i];
            for (uint32_t k = 0; k < 3u; ++k) {
                const uint32_t c = (r >> (kEventCountBits * k)) & kEventCountMask;
                atomicAdd(&bins[n_delta + k * (L + 1u) + (c < L ? c : L)], 1u);
            }
        }
    }
    __syncthreads();
    if (want_delta) flush_bins(bins, n_delta, delta + (uint64_t)s * n_delta, t, nt);
    if (events) flush_bins(bins + n_delta, n_ev, events + (uint64_t)s * n_ev, t, nt);
}

}  // namespace mcgp
