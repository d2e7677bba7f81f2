// combined.hip.h -- race odds under planned stops, time penalties, forced events and lap-time offsets in one scenario
// (mcgp_run_combined, include/mcgp.h, which states how the rule sets meet on one lap).
//
// race_combined_kernel is race_strategy_kernel (strategy.hip.h: S scenarios of one race with common random numbers, one
// lane per (scenario, simulation), blockIdx.y the scenario, load_block's LDS rows unchanged, PlannedTyres) with all four
// policy slots of run_laps filled:
//
//   pit      CombinedPit holds one PlanPit and does in after_pit what PenaltyPit (penalties.hip.h) and PacePit
//            (paces.hip.h) do there, in this order: the served SERVE_AT_STOP penalty is added after pit_loss, the
//            UNTIL_STOP offset of a car that stopped is cleared (which does not touch the time), the lap's ON_LAP
//            addition is added.  A forced red flag's free tyre change is in the event step and never reaches the hook;
//   events   ForcedEvents (events.hip.h), unchanged;
//   pace     OffsetPace (paces.hip.h), unchanged, for start_from_grid (lap 1 reads the base pace) and run_laps;
//   observer PackedEventCounter (events.hip.h), unchanged.
//
// The flag step and the fate of a serve penalty are race_penalties_kernel's, the laps carried of an offset that no stop
// cleared race_paces_kernel's.  Every table is the sibling's own (PenaltyScenario, PenaltyLap, PaceScenario, PaceLap,
// the event bytes, StopLap), packed by the sibling's packer and read at wave-uniform addresses once per lap: begin_lap
// reads the lap's StopLap, PenaltyLap and PaceLap::until, OffsetPace::begin_lap the lap's PaceLap, ForcedEvents the lap's
// byte.  A lap on which the scenario has nothing of a kind pays that kind's sibling test: the two bit tests of
// PenaltyPit on registers, `stopped &&` in front of PacePit's, OffsetPace's wave-uniform `mask | until`.  The per-lane
// state is two u32 in registers, `served` and `active`; the policies (passed by value) hold pointers to them.  Nothing
// new is drawn and no draw moves, so a call with one kind of item is that kind's own call cell for cell.
//
// Staging per scenario and simulation, each in its sibling's layout so that the siblings' counting kernels read them as
// they are: n bytes (position | fate << 5: penalties_count, which also counts the deltas since it masks the position),
// one u32 when events_out is wanted (the packed event counts: events_count with delta NULL), n u16 when carried_out is
// wanted (paces_count with delta NULL; it reads no position byte then).
//
// Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five with max - min;
// profiles/combined_time.txt): two empty scenarios 102.84 (0.41) against 98.22 (0.39) for mcgp_run_strategies
// and 106.69 (0.39) for mcgp_run_paces with an UNTIL_STOP offset, the dearest single-kind call, both built from the parent
// commit; with a penalty to serve 103.08 (0.35), a forced safety car 102.50 (0.45), an UNTIL_STOP offset 108.13 (0.49),
// all three and a planned stop 109.59 (0.42).
#pragma once
#include "penalties.hip.h"
#include "events.hip.h"
#include "paces.hip.h"

namespace mcgp {

// run_laps' pit policy under penalties and offsets together: PlanPit decides the stops; after_pit is PenaltyPit's serve,
// PacePit's clear, PenaltyPit's lap addition.
struct CombinedPit {
    PlanPit plan;
    const PenaltyScenario *__restrict__ pen;
    const PenaltyLap *__restrict__ pen_laps;    // this scenario's [L + 1]
    const PaceLap *__restrict__ pace_laps;      // this scenario's [L + 1]
    const uint16_t *__restrict__ until_from;    // PaceScenario::until_from
    uint32_t *served;                           // the lane's mask of drivers that served in the pits
    uint32_t *active;                           // the lane's UNTIL_STOP offsets not yet cleared
    uint16_t *carried;                          // the lane's staged [n], or NULL
    uint32_t serve;                             // PenaltyScenario::serve
    uint32_t lap_mask, lap_first;               // the current lap's PenaltyLap
    uint32_t until;                             // the current lap's PaceLap::until

    __device__ __forceinline__ void begin_lap(int l)
    {
        plan.begin_lap(l);
        const PenaltyLap pl = pen_laps[l];
        lap_mask = pl.mask;
        lap_first = pl.first;
        until = pace_laps[l].until;
    }
    __device__ __forceinline__ int decide(uint32_t d, uint32_t &newc) const { return plan.decide(d, newc); }
    __device__ __forceinline__ double after_pit(uint32_t d, bool stopped, double t) const
    {
        const uint32_t bit = 1u << d;
        if (stopped) {
            if (((serve & ~*served) & bit) && plan.lap >= (int)pen->serve_from[d]) {
                t = t + pen->serve_sec[d];
                *served |= bit;
            }
            if ((until & *active) & bit) {
                *active &= ~bit;
                if (carried) carried[d] = (uint16_t)(plan.lap - (int)until_from[d] + 1);
            }
        }
        if (lap_mask & bit) t = t + pen->lap_sec[lap_first + (uint32_t)__popc(lap_mask & (bit - 1u))];
        return t;
    }
};

// Simulations sim_offset + [0, m) of every scenario (gridDim.y = S), from the grid (kFromState false) or from `state`.
// hist [S][n][n] is ACCUMULATED into; stage [S][m][n] (classified position | fate << 5 of each driver) is written, and,
// where wanted (NULL: not), ev_stage [S][m] (the packed event counts) and carried [S][m][n] u16 at the drivers that have
// an UNTIL_STOP offset in the scenario.
template <bool kFromState>
__global__ void __launch_bounds__(512)
race_combined_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state,
                     const StrategyScenario *__restrict__ scen, const StopLap *__restrict__ stop_laps,
                     const PenaltyScenario *__restrict__ pens, const PenaltyLap *__restrict__ pen_laps,
                     const uint8_t *__restrict__ event_laps, const PaceScenario *__restrict__ paces,
                     const PaceLap *__restrict__ pace_laps, const double *__restrict__ lap_sec, uint64_t m,
                     uint64_t sim_offset, uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist,
                     uint8_t *__restrict__ stage, uint32_t *__restrict__ ev_stage, uint16_t *__restrict__ carried,
                     uint32_t n_batches)
{
    const uint32_t sid = blockIdx.y;
    const StrategyScenario *__restrict__ sc = scen + sid;
    const PenaltyScenario *__restrict__ pen = pens + sid;
    const PaceScenario *__restrict__ ps = paces + sid;
    const size_t lap0 = (size_t)sid * (size_t)(P->total_laps + 1);
    const PlanPit plan = {stop_laps + lap0, sc->planned, 0u, 0};
    const PenaltyLap *__restrict__ nl = pen_laps + lap0;
    const PaceLap *__restrict__ pl = pace_laps + lap0;
    const ForcedEvents forced = {event_laps + lap0};
    const uint32_t serve = pen->serve, flag = pen->flag, until = ps->until;
    run_block(P, m, n_batches, hist + (size_t)sid * (size_t)(P->n * P->n),
              [=](const Rows &s, const LapEnv &e, uint32_t *s_hist, uint64_t local) {
        const uint64_t sim = sim_offset + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);
        const uint64_t lane = (uint64_t)sid * m + local, cell = lane * (uint64_t)e.n;
        uint16_t *crow = carried ? carried + cell : nullptr;
        uint32_t served = 0u, active = until;
        const OffsetPace pace = {pl, lap_sec, ps->until_sec, &active, 0u, 0u, 0u};
        const CombinedPit pit = {plan, pen, nl, pl, ps->until_from, &served, &active, crow, serve, 0u, 0u, 0u};
        const RaceStart at = kFromState ? start_from_state(s, e, *state, c0, c1, seed_lo, seed_hi)
                                        : start_from_grid(s, e, c0, c1, seed_lo, seed_hi, nullptr, PlannedTyres{sc}, pace);
        PackedEventCounter seen = {0u};
        run_laps(s, e, c0, c1, seed_lo, seed_hi, at.first_lap, at.drs_disabled_until, seen, pit, forced,
                 pace);                                                                             // reference :166-228
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
        uint8_t *row = stage + cell;
        for (int p = 0; p < e.n; ++p) {
            const uint32_t d = s.Ord(p), bit = 1u << d;
            const uint32_t fate = !(serve & bit) ? kFateNone : (served & bit) ? kFateServed
                                  : (retired & bit) ? kFateRetired : kFateFlag;
            row[d] = (uint8_t)((uint32_t)p | (fate << kStageFateShift));
        }
        if (ev_stage) ev_stage[lane] = seen.packed;
        // the offsets no stop cleared: carried up to the car's retirement, or to the flag
        if (crow) {
            for (uint32_t rest = active; rest; rest &= rest - 1u) {
                const uint32_t d = (uint32_t)__ffs((int)rest) - 1u, pk = s.Pk(d);
                const int from = (int)ps->until_from[d];
                const int end = (pk & kDnf) ? (int)(pk & kAgeMask) : e.L + 1;       // the first lap without a lap time
                crow[d] = (uint16_t)(end > from ? end - from : 0);
            }
        }
    });
}

}  // namespace mcgp
