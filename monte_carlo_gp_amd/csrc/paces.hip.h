// paces.hip.h -- race odds under lap-time offsets by lap or until a car's next stop (mcgp_run_paces, include/mcgp.h).
//
// The tables and policies of the paces rule set of race_scenario_kernel (scenario.hip.h: S scenarios of one race with
// common random numbers, one lane per (scenario, simulation), blockIdx.y the scenario), and paces_count.  The rule set
// is two policies:
//
//   pace     OffsetPace, the pace policy of start_from_grid (lap 1) and run_laps: wherever the model reads base_pace[d]
//            -- lap 1's base_lap, the lap time of laps >= 2, the pace of the three overtake passes -- the car's base is
//            b = base_pace[d]; b = b + seconds of the LAPS offset that covers the lap; b = b + seconds of the car's
//            active UNTIL_STOP offset: at most two binary64 additions, in that order;
//   pit      ScenarioPit's after_pit clears the lane's UNTIL_STOP bit of a car that stopped (the rule's stop or a planned
//            one) on a lap >= the offset's first_lap.  The lap time of that lap is computed before the pit step and
//            carries the offset; the overtakes of that lap are after it and do not.
//
// Offset data reach the kernel as read-only global memory at wave-uniform addresses, as a scenario's StopLap does: a
// PaceLap per scenario and lap (16 bytes, one scalar load: the drivers with a LAPS offset on the lap, where their seconds
// start in the call's list, and the drivers whose UNTIL_STOP offset has begun), a PaceScenario (the UNTIL_STOP mask,
// from-laps and seconds) and one list of LAPS seconds, by lap and then by driver, in which consecutive laps covered by
// the same offsets share their entries (at most 2 * 64 + 1 runs of at most 32 entries per scenario).  begin_lap reads the
// lap's PaceLap once; a base read on a lap without an offset in the scenario costs one wave-uniform test, on any other
// lap one bit test on registers (two more for a car that has an offset), and only a car whose bit is set fetches its
// seconds.  The per-lane state is one u32 in a register, the UNTIL_STOP offsets not yet cleared; both policies (passed
// by value) hold a pointer to it.  Nothing new is drawn and no draw moves.
//
// Staging: the strategy call's byte per scenario, simulation and driver (the classified position) and, when
// carried_out is wanted, one u16 per scenario, simulation and driver: the laps whose lap time carried the driver's
// UNTIL_STOP offset.  It is written when the bit clears (lap - first_lap + 1) and, after run_laps, for the bits still set
// (from the retirement lap in `pk`, or L); cells of drivers without such an offset are not written and not read.
// paces_count reads the staging once, blockIdx.y the scenario: blockIdx.z = 0 counts pos_s(d) - pos_0(d) for scenarios
// s >= 1 (count_position_deltas, strategy.hip.h: the centre bin left out); blockIdx.z = 1 + d counts driver d's laps carried, if
// the scenario gives d an UNTIL_STOP offset, into [L + 1] u32 LDS bins (4 KB at L = 1000; a whole [n][L + 1] block of bins
// would be 128 KB), column 0 left out: the host derives it, for every driver, from n_sims.  One u64 global atomic per
// non-zero bin.  It has no cross-lane operation and strides by its block's size.
// Overflow: a launch is at most max_sims_per_launch() < 2^32 simulations per scenario, so no u32 bin can wrap.
//
// Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five with max - min;
// profiles/paces_time.txt): two empty scenarios 99.61 (0.48) against 97.72 (0.34) for mcgp_run_strategies
// built from the parent commit; with one LAPS range of ten laps 101.24 (0.50); with one UNTIL_STOP offset 105.76 (0.43).
#pragma once
#include "strategy.hip.h"

namespace mcgp {

constexpr uint32_t kMaxScenarioPaces = 64;
constexpr int kPaceLaps = 0, kPaceUntilStop = 1;            // MCGP_PACE_* of include/mcgp.h
constexpr double kMaxPaceSeconds = 60.0;
constexpr int kPacesCountBlock = 256;                       // threads of a counting block
constexpr uint32_t kPaceDeltaBins = kMaxCars * (2 * kMaxCars - 1);
static_assert(kMaxLaps + 1 <= (int)kPaceDeltaBins, "a driver's laps-carried bins fit the block's delta bins");
static_assert(kMaxLaps <= 0xFFFF, "a count of laps fits the staged u16");

// One scenario's UNTIL_STOP offsets in device memory.
struct PaceScenario {
    uint32_t until;                     // bit d: driver d has an UNTIL_STOP offset
    uint32_t pad;
    uint16_t until_from[kMaxCars];      // its first_lap
    double until_sec[kMaxCars];
};

// The offsets of one scenario on one lap: 16 bytes, one scalar load.
struct PaceLap {
    uint32_t mask;                      // bit d: a LAPS offset of driver d covers this lap
    uint32_t first;                     // lap_sec[first + (number of set bits below d)] is driver d's
    uint32_t until;                     // bit d: driver d's UNTIL_STOP offset has first_lap <= this lap
    uint32_t pad;
};

// The pace policy under offsets (ModelPace, race_kernel.hip.h, is the model's): the car's base pace on the current lap.
struct OffsetPace {
    const PaceLap *__restrict__ laps;           // this scenario's [L + 1]
    const double *__restrict__ lap_sec;         // the call's LAPS seconds
    const double *__restrict__ until_sec;       // PaceScenario::until_sec
    const uint32_t *active;                     // the lane's UNTIL_STOP offsets not yet cleared
    uint32_t mask, first, until;                // the current lap's PaceLap

    __device__ __forceinline__ void begin_lap(int l)
    {
        const PaceLap pl = laps[l];
        mask = pl.mask;
        first = pl.first;
        until = pl.until;
    }
    __device__ __forceinline__ double base(uint32_t d, double b) const
    {
        if (!(mask | until)) return b;          // wave-uniform: the lap has no offset in this scenario
        const uint32_t bit = 1u << d, open = until & *active;
        if ((mask | open) & bit) {              // one test where the car has none
            if (mask & bit) b = b + lap_sec[first + (uint32_t)__popc(mask & (bit - 1u))];
            if (open & bit) b = b + until_sec[d];
        }
        return b;
    }
};

// From the staged data of m simulations, for scenario s = blockIdx.y: a block with blockIdx.z = 0 adds the paired
// changes of position against scenario 0 to delta [S][n][2n - 1] (s >= 1, the centre left out; delta may be NULL); a
// block with blockIdx.z = 1 + d adds driver d's laps carried to carried_out [S][n][L + 1] (column 0 left out; only if the
// scenario gives d an UNTIL_STOP offset; carried_out may be NULL, and gridDim.z 1 then).  u32 LDS bins per block, one u64
// global atomic per non-zero bin; any block size.
__global__ void __launch_bounds__(kPacesCountBlock)
paces_count(const uint8_t *__restrict__ stage, const uint16_t *__restrict__ carried, const PaceScenario *__restrict__ paces,
            uint64_t m, uint32_t n, uint32_t L, unsigned long long *__restrict__ delta,
            unsigned long long *__restrict__ carried_out)
{
    __shared__ uint32_t bins[kPaceDeltaBins];
    const uint32_t t = threadIdx.x, nt = blockDim.x, s = blockIdx.y, w = 2u * n - 1u;
    const bool deltas = blockIdx.z == 0u;
    const uint32_t d = deltas ? 0u : blockIdx.z - 1u;
    if (deltas ? (delta == nullptr || s == 0u) : (carried_out == nullptr || d >= n || !((paces[s].until >> d) & 1u))) return;
    const uint32_t n_bins = deltas ? n * w : L + 1u;
    for (uint32_t i = t; i < n_bins; i += nt) bins[i] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)s * m * n;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt) {
        if (deltas) {
            count_position_deltas(stage + i * n, stage + base + i * n, n, 0xFFu, bins);
        } else {
            const uint32_t c = carried[base + i * n + d];
            if (c) atomicAdd(&bins[c < L ? c : L], 1u);
        }
    }
    __syncthreads();
    flush_bins(bins, n_bins, deltas ? delta + (uint64_t)s * n_bins : carried_out + ((uint64_t)s * n + d) * n_bins, t, nt);
}

}  // namespace mcgp
