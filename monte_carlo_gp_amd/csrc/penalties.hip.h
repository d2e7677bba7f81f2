// penalties.hip.h -- race odds under time penalties and planned pit stops (mcgp_run_penalties, include/mcgp.h).
//
// The tables and constants of the penalties rule set of race_scenario_kernel (scenario.hip.h: S scenarios of one race
// with common random numbers, one lane per (scenario, simulation), blockIdx.y the scenario), and penalties_count.  The
// rule set adds time to a car in three places:
//
//   serve    a SERVE_AT_STOP penalty pending from lap p: at the car's first stop (the rule's or a planned one) on a lap
//            >= p, run_laps' after_pit hook (ScenarioPit) adds the seconds after pit_loss, and the lane's `served` bit of
//            the driver is set;
//   lap      an ON_LAP addition: the same hook adds the seconds on that lap, after any stop of the lap (a served penalty
//            included), before the overtakes; a car that retires on that lap never reaches the hook;
//   flag     after run_laps and before classify_and_count, every running car adds its unserved SERVE_AT_STOP seconds,
//            then its AT_FLAG seconds, and sort_by_time orders the field again.  A scenario without serve and flag
//            penalties skips the step: its field is sorted already, so the sort would change nothing.
//
// Penalty data reach the kernel as global memory at wave-uniform base addresses, as a scenario's StopLap does: a
// PenaltyScenario (the serve and flag masks, the serve-from laps, the seconds) and a PenaltyLap per lap (the drivers
// with an ON_LAP addition and where their seconds start in the scenario's list).  begin_lap reads the lap's mask once;
// the test of a car-lap is two bit tests on registers (unserved serve penalty, ON_LAP mask), and only a car that takes
// an addition reads its seconds.  The per-lane state is one u32 in a register, the drivers that served in the pits;
// the policy (passed to run_laps by value) holds a pointer to it.  Nothing new is drawn.
//
// Staging: one byte per scenario, simulation and driver: bits 0-4 the classified position, bits 5-6 the fate of the
// driver's SERVE_AT_STOP penalty (0 none, 1 served at a stop, 2 added at the flag, 3 retired unserved).  penalties_count
// counts pos_s(d) - pos_0(d) for scenarios s >= 1 (count_position_deltas, strategy.hip.h: the centre bin left out) and the
// fates 1..3 of every scenario into u32 LDS bins, then one u64 global atomic per non-zero bin (flush_bins); the host
// derives the centre bin and fate column 0 from n_sims.  It has no cross-lane operation and strides by its block's size.
// Overflow: a launch is at most max_sims_per_launch() < 2^32 simulations per scenario, so no u32 bin can wrap.
//
// Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five; profiles/penalties_time.txt,
// DESIGN 3.16): two empty scenarios 98.76 against 97.76 for mcgp_run_strategies built from the parent commit (its runs
// spread over 0.38), all of it in the race kernel; with a penalty to serve 98.88, at the flag 98.60, on a lap 98.98.
#pragma once
#include "strategy.hip.h"

namespace mcgp {

constexpr uint32_t kMaxScenarioPenalties = 256;
constexpr int kPenServeAtStop = 0, kPenAtFlag = 1, kPenOnLap = 2;      // MCGP_PEN_* of include/mcgp.h
constexpr uint32_t kFateNone = 0, kFateServed = 1, kFateFlag = 2, kFateRetired = 3;
constexpr uint32_t kStagePosMask = 31u;
constexpr int kStageFateShift = 5;
constexpr int kPenaltyCountBlock = 256;         // threads of a counting block

// One scenario's penalties in device memory.
struct PenaltyScenario {
    uint32_t serve;                     // bit d: driver d has a SERVE_AT_STOP penalty
    uint32_t flag;                      // bit d: driver d has an AT_FLAG penalty
    uint16_t serve_from[kMaxCars];      // the lap the SERVE_AT_STOP penalty is pending from
    double serve_sec[kMaxCars];
    double flag_sec[kMaxCars];
    double lap_sec[kMaxScenarioPenalties];      // the ON_LAP seconds, by lap and then by driver
};

// The ON_LAP additions of one scenario on one lap: 8 bytes, one scalar load.
struct PenaltyLap {
    uint32_t mask;                      // bit d: driver d adds time on this lap
    uint32_t first;                     // lap_sec[first + (number of set bits below d)] is driver d's
};

// From the staged bytes of m simulations: for scenario s = blockIdx.y, delta [S][n][2n - 1] += the paired changes of
// position against scenario 0 (s >= 1, the centre left out; delta may be NULL) and fate [S][n][4] += the fates 1..3
// (fate may be NULL).  u32 LDS bins per block, one u64 global atomic per non-zero bin; any block size.
__global__ void __launch_bounds__(kPenaltyCountBlock)
penalties_count(const uint8_t *__restrict__ stage, uint64_t m, uint32_t n, unsigned long long *__restrict__ delta,
                unsigned long long *__restrict__ fate)
{
    __shared__ uint32_t bins[kMaxCars * (2 * kMaxCars - 1) + kMaxCars * 4];
    const uint32_t t = threadIdx.x, nt = blockDim.x, s = blockIdx.y;
    const uint32_t n_delta = n * (2u * n - 1u), n_bins = n_delta + n * 4u;
    const bool want_delta = delta != nullptr && s > 0u;
    for (uint32_t i = t; i < n_bins; i += nt) bins[i] = 0u;
    __syncthreads();
    const uint8_t *base = stage + (uint64_t)s * m * n;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt) {
        count_position_deltas(stage + i * n, base + i * n, n, kStagePosMask, bins, want_delta, [&](uint32_t d, uint32_t b1) {
            const uint32_t f = (b1 >> kStageFateShift) & 3u;
            if (f && fate) atomicAdd(&bins[n_delta + d * 4u + f], 1u);
        });
    }
    __syncthreads();
    if (want_delta) flush_bins(bins, n_delta, delta + (uint64_t)s * n_delta, t, nt);
    if (fate) flush_bins(bins + n_delta, n * 4u, fate + (uint64_t)s * n * 4u, t, nt);
}

}  // namespace mcgp
