// weather.hip.h -- race odds when the track condition changes by lap (mcgp_run_weather, include/mcgp.h).
//
// The tables and policies of the weather rule set of race_scenario_kernel (scenario.hip.h: S scenarios of one race with
// common random numbers, one lane per (scenario, simulation), blockIdx.y the scenario), and weather_count.  The rule set
// is two policies:
//
//   track    WeatherTrack, the track policy of run_laps: the lap's condition c_k stands wherever lap k's code reads the
//            track condition -- the red flag's and the rule stop's stint_compound, the rule stop's two-compound waiver --
//            and a car under the model's rule also stops when it is on the wrong tyres (the class of its compound, dry
//            SOFT / MEDIUM / HARD or wet INTERMEDIATE / WET, is not the class of c_k), under the rule's own
//            remaining_laps > 5.  It sees every lap time of laps >= 2 with the compound it was computed on and counts the
//            laps on the wrong tyres;
//   pace     WeatherPace, the pace policy of start_from_grid (lap 1, the configuration's condition) and run_laps: wherever
//            the model reads base_pace[d] the car's base is b = base_pace[d] + wrong_tyre_sec[c_k][compound], the compound
//            read from the car's pk word at that point: before the pit step for the lap time, after it for the overtakes.
//
// Weather data reach the kernel as read-only global memory: one byte per scenario and lap, [S][L + 1], always filled (the
// configuration's condition where no change covers the lap), read once per lap and policy at a wave-uniform address as
// ForcedEvents reads its byte; and the call's 3 x 5 table of seconds, read by compound, beside the other rule sets'
// seconds.  Bits 0-1 of the byte are the condition; bit 2 + k says that the table's entry of the condition and compound
// k is non-zero.  A base read on a lap whose row is all zero costs one wave-uniform test, on any other lap one bit test
// on registers, and only a car whose entry is non-zero fetches it (b + 0.0 is b), as OffsetPace fetches its seconds.
// The rule set has no per-lane state beside the staging.  Nothing new is drawn and no draw moves.
//
// Staging: the strategy call's byte per scenario, simulation and driver (the classified position; strategy_count_deltas
// counts the deltas) and, when wrong_laps_out is wanted, one u16 per scenario, simulation and driver: the laps whose lap
// time was computed with the car on the wrong tyres.  The lane writes every driver's cell after the start (lap 1: 1 for
// a car that set a lap time on the wrong class for the configuration's condition, else 0; from a state 0) and adds one
// where a lap time of laps >= 2 is on the wrong tyres.  weather_count reads the u16 once, blockIdx.y the scenario,
// blockIdx.z the driver, into [L + 1] u32 LDS bins, column 0 left out: the host derives it from n_sims.  One u64 global
// atomic per non-zero bin.  It has no cross-lane operation and strides by its block's size.
// Overflow: a launch is at most max_sims_per_launch() < 2^32 simulations per scenario, so no u32 bin can wrap.
//
// Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five with max - min;
// profiles/weather_time.txt): two empty scenarios and a zero table 101.64 (0.21) against 97.39 (0.11) for
// mcgp_run_strategies built from the parent commit; damp from lap L / 2 to the flag under a zero table 101.44 (0.43); the
// same change under the default table 107.27 (0.15).
#pragma once
#include "strategy.hip.h"

namespace mcgp {

constexpr uint32_t kMaxScenarioTrackChanges = 64;
constexpr int kTrackConditions = 3, kCompounds = 5;         // MCGP_DRY .. MCGP_WET_TRACK, MCGP_SOFT .. MCGP_WET
constexpr double kMaxWrongTyreSeconds = 60.0;
constexpr uint32_t kCondMask = 3u;                          // a lap's byte: the condition ...
constexpr int kCondLiveShift = 2;                           // ... and above it, bit k: the table's entry of compound k is non-zero
constexpr int kWeatherCountBlock = 256;                     // threads of a counting block
static_assert(kMaxLaps <= 0xFFFF, "a count of laps fits the staged u16");

// Is a car on compound `comp` on the wrong tyres under condition `cond`?  Dry tyres on a wet track or wet tyres on a dry one.
__device__ __forceinline__ bool wrong_tyres(uint32_t cond, uint32_t comp) { return (comp >= 3u) != (cond != 0u); }

// The track policy under a condition that changes by lap (ModelTrack, race_kernel.hip.h, is the model's).
struct WeatherTrack {
    const uint8_t *__restrict__ laps;           // this scenario's [L + 1]
    uint16_t *wrong;                            // the lane's staged [n], or NULL
    uint32_t cond;                              // the current lap's condition

    __device__ __forceinline__ int begin_lap(int l, int /*track*/)
    {
        cond = laps[l] & kCondMask;
        return (int)cond;
    }
    __device__ __forceinline__ bool lap_time_on(uint32_t d, uint32_t comp) const
    {
        const bool w = wrong_tyres(cond, comp);
        if (w && wrong) wrong[d] = (uint16_t)(wrong[d] + 1u);
        return w;
    }
};

// The pace policy under the wrong-tyre table: the car's base pace on the current lap, on the compound its pk word holds.
struct WeatherPace {
    const uint8_t *__restrict__ laps;           // this scenario's [L + 1]
    const double *__restrict__ table;           // the call's [3][5] seconds
    Rows s;                                     // the lane's rows
    const double *row;                          // the current lap's row of the table
    uint32_t live;                              // bit k: its entry of compound k is non-zero

    __device__ __forceinline__ void begin_lap(int l)
    {
        const uint32_t b = laps[l];
        row = table + (b & kCondMask) * (uint32_t)kCompounds;
        live = b >> kCondLiveShift;
    }
    __device__ __forceinline__ double base(uint32_t d, double b) const
    {
        if (!live) return b;                    // wave-uniform: the lap's condition costs nothing on any compound
        const uint32_t comp = (s.Pk(d) >> kCompShift) & 7u;
        if ((live >> comp) & 1u) b = b + row[comp];
        return b;
    }
};

// From the staged u16 of m simulations: wrong_out [S][n][L + 1] += the simulations in which driver d = blockIdx.z of
// scenario s = blockIdx.y had that many laps on the wrong tyres, column 0 left out.  u32 LDS bins per block, one u64 global
// atomic per non-zero bin; any block size.
__global__ void __launch_bounds__(kWeatherCountBlock)
weather_count(const uint16_t *__restrict__ wrong, uint64_t m, uint32_t n, uint32_t L,
              unsigned long long *__restrict__ wrong_out)
{
    __shared__ uint32_t bins[kMaxLaps + 1];
    const uint32_t t = threadIdx.x, nt = blockDim.x, s = blockIdx.y, d = blockIdx.z, n_bins = L + 1u;
    if (d >= n) return;
    for (uint32_t i = t; i < n_bins; i += nt) bins[i] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)s * m * n;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt) {
        const uint32_t c = wrong[base + i * n + d];
        if (c) atomicAdd(&bins[c < L ? c : L], 1u);
    }
    __syncthreads();
    flush_bins(bins, n_bins, wrong_out + ((uint64_t)s * n + d) * n_bins, t, nt);
}

}  // namespace mcgp
