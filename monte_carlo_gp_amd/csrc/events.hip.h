// events.hip.h -- race odds with the race-interrupting events of chosen laps set by the caller (mcgp_run_events,
// include/mcgp.h).
//
// race_events_kernel is race_strategy_kernel (strategy.hip.h: S scenarios of one race with common random numbers, one
// lane per (scenario, simulation), blockIdx.y the scenario, load_block's LDS rows unchanged, PlannedTyres and PlanPit)
// with an event policy for run_laps and a lap observer that counts the events:
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
// Nothing new is drawn and no other draw moves, so a scenario without overrides is race_strategy_kernel's scenario
// cell for cell.
//
// Staging: the strategy kernel's byte per scenario, simulation and driver (the classified position), and one u32 per
// scenario and simulation (red flags | safety cars << 10 | VSCs << 20).  events_count reads both once, blockIdx.y the
// scenario: pos_s(d) - pos_0(d) for scenarios s >= 1 (the centre bin left out, as strategy_count_deltas does) and the
// three event counts into u32 LDS bins, [n][2n - 1] + [3][L + 1] (20 KB at n = 32, L = 1000), then one u64 global atomic
// per non-zero bin.  It has no cross-lane operation and strides by its block's size.
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

// Simulations sim_offset + [0, m) of every scenario (gridDim.y = S), from the grid (kFromState false) or from `state`.
// hist [S][n][n] is ACCUMULATED into; stage [S][m][n] (classified position of each driver) and ev_stage [S][m] (the
// packed event counts) are written.
template <bool kFromState>
__global__ void __launch_bounds__(512)
race_events_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state,
                   const StrategyScenario *__restrict__ scen, const StopLap *__restrict__ stop_laps,
                   const uint8_t *__restrict__ event_laps, uint64_t m, uint64_t sim_offset, uint32_t seed_lo,
                   uint32_t seed_hi, unsigned long long *__restrict__ hist, uint8_t *__restrict__ stage,
                   uint32_t *__restrict__ ev_stage, uint32_t n_batches)
{
    const uint32_t sid = blockIdx.y;
    const StrategyScenario *__restrict__ sc = scen + sid;
    const size_t lap0 = (size_t)sid * (size_t)(P->total_laps + 1);
    const PlanPit pit = {stop_laps + lap0, sc->planned, 0u, 0};
    const ForcedEvents forced = {event_laps + lap0};
    run_block(P, m, n_batches, hist + (size_t)sid * (size_t)(P->n * P->n),
              [=](const Rows &s, const LapEnv &e, uint32_t *s_hist, uint64_t local) {
        const uint64_t sim = sim_offset + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);
        const RaceStart at = kFromState ? start_from_state(s, e, *state, c0, c1, seed_lo, seed_hi)
                                        : start_from_grid(s, e, c0, c1, seed_lo, seed_hi, nullptr, PlannedTyres{sc});
        PackedEventCounter seen = {0u};
        run_laps(s, e, c0, c1, seed_lo, seed_hi, at.first_lap, at.drs_disabled_until, seen, pit, forced);   // reference :166-228
        classify_and_count(s, e.n, s_hist, nullptr);                                                // reference :230-242
        // each driver's classified position, and the lane's events
        uint8_t *row = stage + ((uint64_t)sid * m + local) * (uint64_t)e.n;
        for (int p = 0; p < e.n; ++p) row[s.Ord(p)] = (uint8_t)p;
        ev_stage[(uint64_t)sid * m + local] = seen.packed;
    });
}

// From the staged data of m simulations: for scenario s = blockIdx.y, delta [S][n][2n - 1] += the paired changes of
// position against scenario 0 (s >= 1, the centre left out; delta may be NULL) and events [S][3][L + 1] += the
// simulations with that many red flags / safety cars / VSCs (events may be NULL).  u32 LDS bins per block, one u64
// global atomic per non-zero bin; any block size.
__global__ void __launch_bounds__(kEventsCountBlock)
events_count(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ ev_stage, uint64_t m, uint32_t n, uint32_t L,
             unsigned long long *__restrict__ delta, unsigned long long *__restrict__ events)
{
    __shared__ uint32_t bins[kMaxCars * (2 * kMaxCars - 1) + 3 * (kMaxLaps + 1)];
    const uint32_t t = threadIdx.x, nt = blockDim.x, s = blockIdx.y, w = 2u * n - 1u;
    const uint32_t n_delta = n * w, n_ev = 3u * (L + 1u), n_bins = n_delta + n_ev;
    const bool want_delta = delta != nullptr && s > 0u;
    for (uint32_t i = t; i < n_bins; i += nt) bins[i] = 0u;
    __syncthreads();
    const uint8_t *base = stage + (uint64_t)s * m * n;
    const uint32_t *ev = ev_stage + (uint64_t)s * m;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt) {
        if (want_delta) {
            const uint8_t *r0 = stage + i * n, *r1 = base + i * n;
            for (uint32_t d = 0; d < n; ++d) {
                const uint32_t p0 = r0[d], p1 = r1[d];
                if (p0 != p1) atomicAdd(&bins[d * w + (p1 + n - 1u - p0)], 1u);
            }
        }
        if (events) {
            const uint32_t r = ev[i];
            for (uint32_t k = 0; k < 3u; ++k) {
                const uint32_t c = (r >> (kEventCountBits * k)) & kEventCountMask;
                atomicAdd(&bins[n_delta + k * (L + 1u) + (c < L ? c : L)], 1u);
            }
        }
    }
    __syncthreads();
    if (want_delta) {
        unsigned long long *out = delta + (uint64_t)s * n_delta;
        for (uint32_t i = t; i < n_delta; i += nt)
            if (bins[i]) atomicAdd(&out[i], (unsigned long long)bins[i]);
    }
    if (events) {
        unsigned long long *out = events + (uint64_t)s * n_ev;
        for (uint32_t i = t; i < n_ev; i += nt)
            if (bins[n_delta + i]) atomicAdd(&out[i], (unsigned long long)bins[n_delta + i]);
    }
}

}  // namespace mcgp
