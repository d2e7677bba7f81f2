// penalties.hip.h -- race odds under time penalties and planned pit stops (mcgp_run_penalties, include/mcgp.h).
//
// race_penalties_kernel is race_strategy_kernel (strategy.hip.h: S scenarios of one race with common random numbers, one
// lane per (scenario, simulation), blockIdx.y the scenario, load_block's LDS rows unchanged) with a pit policy that
// wraps PlanPit and adds time to a car in three places:
//
//   serve    a SERVE_AT_STOP penalty pending from lap p: at the car's first stop (the rule's or a planned one) on a lap
//            >= p, run_laps' after_pit hook adds the seconds after pit_loss, and the lane's `served` bit of the driver
//            is set;
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
// reads it once: pos_s(d) - pos_0(d) for scenarios s >= 1 (the centre bin left out, as strategy_count_deltas does) and the
// fates 1..3 of every scenario into u32 LDS bins, then one u64 global atomic per non-zero bin; the host derives the centre
// bin and fate column 0 from n_sims.  It has no cross-lane operation and strides by its block's size.
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

// run_laps' pit policy under penalties: PlanPit decides the stops; after_pit adds the served penalty and the lap's.
struct PenaltyPit {
    PlanPit plan;
    const PenaltyScenario *__restrict__ pen;
    const PenaltyLap *__restrict__ laps;        // this scenario's [L + 1]
    uint32_t *served;                           // the lane's mask of drivers that served in the pits
    uint32_t serve;                             // PenaltyScenario::serve
    uint32_t lap_mask, lap_first;               // the current lap's PenaltyLap

    __device__ __forceinline__ void begin_lap(int l)
    {
        plan.begin_lap(l);
        const PenaltyLap pl = laps[l];
        lap_mask = pl.mask;
        lap_first = pl.first;
    }
    __device__ __forceinline__ int decide(uint32_t d, uint32_t &newc) const { return plan.decide(d, newc); }
    __device__ __forceinline__ double after_pit(uint32_t d, bool stopped, double t) const
    {
        const uint32_t bit = 1u << d;
        if (stopped && ((serve & ~*served) & bit) && plan.lap >= (int)pen->serve_from[d]) {
            t = t + pen->serve_sec[d];
            *served |= bit;
        }
        if (lap_mask & bit) t = t + pen->lap_sec[lap_first + (uint32_t)__popc(lap_mask & (bit - 1u))];
        return t;
    }
};

// Simulations sim_offset + [0, m) of every scenario (gridDim.y = S), from the grid (kFromState false) or from `state`.
// hist [S][n][n] is ACCUMULATED into; stage [S][m][n] is written (classified position | fate << 5 of each driver).
template <bool kFromState>
__global__ void __launch_bounds__(512)
race_penalties_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state,
                      const StrategyScenario *__restrict__ scen, const StopLap *__restrict__ stop_laps,
                      const PenaltyScenario *__restrict__ pens, const PenaltyLap *__restrict__ pen_laps, uint64_t m,
                      uint64_t sim_offset, uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist,
                      uint8_t *__restrict__ stage, uint32_t n_batches)
{
    const uint32_t sid = blockIdx.y;
    const StrategyScenario *__restrict__ sc = scen + sid;
    const PenaltyScenario *__restrict__ pen = pens + sid;
    const size_t lap0 = (size_t)sid * (size_t)(P->total_laps + 1);
    const PlanPit plan = {stop_laps + lap0, sc->planned, 0u, 0};
    const PenaltyLap *__restrict__ pl = pen_laps + lap0;
    const uint32_t serve = pen->serve, flag = pen->flag;
    run_block(P, m, n_batches, hist + (size_t)sid * (size_t)(P->n * P->n),
              [=](const Rows &s, const LapEnv &e, uint32_t *s_hist, uint64_t local) {
        const uint64_t sim = sim_offset + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);
        const RaceStart at = kFromState ? start_from_state(s, e, *state, c0, c1, seed_lo, seed_hi)
                                        : start_from_grid(s, e, c0, c1, seed_lo, seed_hi, nullptr, PlannedTyres{sc});
        NoLapObserver none;
        uint32_t served = 0u;
        const PenaltyPit pit = {plan, pen, pl, &served, serve, 0u, 0u};
        run_laps(s, e, c0, c1, seed_lo, seed_hi, at.first_lap, at.drs_disabled_until, none, pit);   // reference :166-228
        // at the flag: the unserved penalty, then the post-race one, of every running car
        const uint32_t unserved = serve & ~served;
        uint32_t retired = 0u;
        if (serve | flag) {
            for (uint32_t rest = unserved | flag; rest; rest &= rest - 1u) {
                const uint32_t d = (uint32_t)__ffs((int)rest) - 1u, bit = 1u << d;
                if (s.Pk(d) & kDnf) { retired |= bit; continue; }
                double t = s.Cum(d);
                if (unserved & bit) t = t + pen->serve_sec[d];
                if (flag & bit) t = t + pen->flag_sec[d];
                s.Cum(d) = t;
            }
            sort_by_time(s, e.n);
        }
        classify_and_count(s, e.n, s_hist, nullptr);                                                // reference :230-242
        // each driver's classified position and the fate of its serve penalty
        uint8_t *row = stage + ((uint64_t)sid * m + local) * (uint64_t)e.n;
        for (int p = 0; p < e.n; ++p) {
            const uint32_t d = s.Ord(p), bit = 1u << d;
            const uint32_t fate = !(serve & bit) ? kFateNone : (served & bit) ? kFateServed
                                  : (retired & bit) ? kFateRetired : kFateFlag;
            row[d] = (uint8_t)((uint32_t)p | (fate << kStageFateShift));
        }
    });
}

// From the staged bytes of m simulations: for scenario s = blockIdx.y, delta [S][n][2n - 1] += the paired changes of
// position against scenario 0 (s >= 1, the centre left out; delta may be NULL) and fate [S][n][4] += the fates 1..3
// (fate may be NULL).  u32 LDS bins per block, one u64 global atomic per non-zero bin; any block size.
__global__ void __launch_bounds__(kPenaltyCountBlock)
penalties_count(const uint8_t *__restrict__ stage, uint64_t m, uint32_t n, unsigned long long *__restrict__ delta,
                unsigned long long *__restrict__ fate)
{
    __shared__ uint32_t bins[kMaxCars * (2 * kMaxCars - 1) + kMaxCars * 4];
    const uint32_t t = threadIdx.x, nt = blockDim.x, s = blockIdx.y, w = 2u * n - 1u;
    const uint32_t n_delta = n * w, n_bins = n_delta + n * 4u;
    const bool want_delta = delta != nullptr && s > 0u;
    for (uint32_t i = t; i < n_bins; i += nt) bins[i] = 0u;
    __syncthreads();
    const uint8_t *base = stage + (uint64_t)s * m * n;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt) {
        const uint8_t *r0 = stage + i * n, *r1 = base + i * n;
        for (uint32_t d = 0; d < n; ++d) {
            const uint32_t b1 = r1[d], p1 = b1 & kStagePosMask, f = (b1 >> kStageFateShift) & 3u;
            if (want_delta) {
                const uint32_t p0 = r0[d] & kStagePosMask;
                if (p0 != p1) atomicAdd(&bins[d * w + (p1 + n - 1u - p0)], 1u);
            }
            if (f && fate) atomicAdd(&bins[n_delta + d * 4u + f], 1u);
        }
    }
    __syncthreads();
    if (want_delta) {
        unsigned long long *out = delta + (uint64_t)s * n_delta;
        for (uint32_t i = t; i < n_delta; i += nt)
            if (bins[i]) atomicAdd(&out[i], (unsigned long long)bins[i]);
    }
    if (fate) {
        unsigned long long *out = fate + (uint64_t)s * n * 4u;
        for (uint32_t i = t; i < n * 4u; i += nt)
            if (bins[n_delta + i]) atomicAdd(&out[i], (unsigned long long)bins[n_delta + i]);
    }
}

}  // namespace mcgp
