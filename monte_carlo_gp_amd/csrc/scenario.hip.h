// scenario.hip.h -- the race kernel of the eight what-if calls: mcgp_run_strategies, mcgp_run_penalties, mcgp_run_events,
// mcgp_run_paces, mcgp_run_combined (include/mcgp.h, which states how the rule sets meet on one lap), mcgp_run_weather,
// mcgp_run_grids and mcgp_run_priors.
//
// race_scenario_kernel<kFromState, kRules> is the generic kernel's code -- start_from_grid or start_from_state, run_laps,
// classify_and_count -- over S scenarios of one race with common random numbers: one lane runs one (scenario, simulation)
// pair in race_kernel's LDS rows; a block serves one scenario (blockIdx.y) and grid-strides over its simulations in
// batches of blockDim.x.  Every scenario has plans (strategy.hip.h: PlannedTyres for the start, PlanPit for the stops).
// kRules names what else it has, and each rule set's code is here once, compiled in where its bit is set:
//
//   kRulePenalties  (penalties.hip.h) ScenarioPit's serve and lap additions; the flag step between run_laps and
//                   classify_and_count; the fate bits of the staged byte;
//   kRuleEvents     (events.hip.h) ForcedEvents in run_laps' event slot, PackedEventCounter as its observer; the staged
//                   event word;
//   kRulePaces      (paces.hip.h) OffsetPace in the pace slot of start_from_grid (lap 1 reads the base pace) and of
//                   run_laps; ScenarioPit's clear of an UNTIL_STOP offset; the laps carried of an offset no stop cleared.
//   kRuleWeather    (weather.hip.h) WeatherTrack in run_laps' track slot and WeatherPace in the pace slot of
//                   start_from_grid and of run_laps; the laps on the wrong tyres.  It is instantiated alone, and its
//                   tables come in the arguments of the rule sets it never meets: the condition bytes in `event_laps`
//                   (the same [S][L + 1] bytes), the table of seconds in `lap_sec`, the staged u16 in `carried`.
//   kRuleGrid       (grids.hip.h) GridEdits in the grid slot of start_from_grid: drops, pins and pit-lane starts on the
//                   drawn grid; every driver's start slot.  It is instantiated alone and only from the grid (a mid-race
//                   state has no grid), and its table comes the same way: the GridScenario [S] in `pens`, the staged u16
//                   in `carried`.
//   kRulePriors     (priors.hip.h) draw_priors before the start; PriorPace in the pace slot of start_from_grid and of
//                   run_laps.  It is instantiated alone, and its table comes the same way: the PriorScenario [S] in `pens`,
//                   the staged bin bytes in `carried` (as bytes), the staged binary32 offsets in `ev_stage` (as floats).
//                   Its lanes have n binary32 offsets in LDS behind their rows, which the launch counts.
//
// A slot whose bit is clear holds the model's policy (ModelPace, DrawnEvents, NoLapObserver, ModelTrack, ModelGrid), which
// vanishes at compile time.  The instantiations are the fifteen the C ABI has: no rule set, each one alone, the first
// three together, each from the grid and, but for the grid edits, from a state.  An instantiation never reads a table whose bit is clear: callers pass NULL there.
//
// Every table is packed by its rule set's packer and read at wave-uniform addresses once per lap: ScenarioPit::begin_lap
// reads the lap's StopLap, PenaltyLap and PaceLap::until, OffsetPace::begin_lap the lap's PaceLap, ForcedEvents the lap's
// byte.  A lap on which the scenario has nothing of a kind pays that kind's test: two bit tests on registers for the
// penalties, `stopped &&` in front of the UNTIL_STOP clear, OffsetPace's wave-uniform `mask | until`.  The per-lane state
// is at most two u32 in registers, `served` and `active`; the policies (passed by value) hold pointers to them.  Nothing
// new is drawn and no draw moves, so a combined call with one kind of item is that kind's own call cell for cell.
//
// Staging per scenario and simulation, each in the layout its counting kernel reads: n bytes (the classified position;
// with penalties | fate << 5, and penalties_count, which masks the position, also counts mcgp_run_combined's deltas), one
// u32 with events (the packed event counts: events_count; with all three rule sets only when ev_stage is given), n u16
// with paces when `carried` is given (paces_count; for mcgp_run_combined both with delta NULL), n u16 with weather when
// `carried` is given (the laps on the wrong tyres: weather_count), n u16 with grid edits when `carried` is given (the
// start slots: grid_count), n bin bytes with priors and n floats when the offsets are wanted (priors_count).
//
// Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five with max - min;
// profiles/combined_time.txt): all three rule sets, two empty scenarios 102.84 (0.41) against 98.22 (0.39) with
// none and 106.69 (0.39) for mcgp_run_paces with an UNTIL_STOP offset, the dearest single-kind call; with a penalty to
// serve 103.08 (0.35), a forced safety car 102.50 (0.45), an UNTIL_STOP offset 108.13 (0.49), all three and a planned stop
// 109.59 (0.42).  profiles/penalties_time.txt, events_time.txt, paces_time.txt, weather_time.txt and grid_time.txt have
// each rule set alone.
#pragma once
#include <type_traits>

#include "penalties.hip.h"
#include "events.hip.h"
#include "paces.hip.h"
#include "weather.hip.h"
#include "grids.hip.h"
#include "priors.hip.h"

namespace mcgp {

constexpr uint32_t kRulePenalties = 1u, kRuleEvents = 2u, kRulePaces = 4u, kRuleWeather = 8u, kRuleGrid = 16u,
                   kRulePriors = 32u;
constexpr uint32_t kRuleAll = kRulePenalties | kRuleEvents | kRulePaces;

// run_laps' pit policy of a scenario: PlanPit decides the stops; after_pit adds the served SERVE_AT_STOP penalty after
// pit_loss, clears the UNTIL_STOP offset of a car that stopped on a lap >= its first_lap (which does not touch the time)
// and stages the laps it was carried, then adds the lap's ON_LAP addition.  A forced red flag's free tyre change is in the
// event step and never reaches the hook.  The members of a rule set whose bit is clear are never read.
template <uint32_t kRules>
struct ScenarioPit {
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
        if constexpr (kRules & kRulePenalties) {
            const PenaltyLap pl = pen_laps[l];
            lap_mask = pl.mask;
            lap_first = pl.first;
        }
        if constexpr (kRules & kRulePaces) until = pace_laps[l].until;
    }
    __device__ __forceinline__ int decide(uint32_t d, uint32_t &newc) const { return plan.decide(d, newc); }
    __device__ __forceinline__ double after_pit(uint32_t d, bool stopped, double t) const
    {
        const uint32_t bit = 1u << d;
        if (stopped) {
            if constexpr (kRules & kRulePenalties) {
                if (((serve & ~*served) & bit) && plan.lap >= (int)pen->serve_from[d]) {
                    t = t + pen->serve_sec[d];
                    *served |= bit;
                }
            }
            if constexpr (kRules & kRulePaces) {
                if ((until & *active) & bit) {
                    *active &= ~bit;
                    if (carried) carried[d] = (uint16_t)(plan.lap - (int)until_from[d] + 1);
                }
            }
        }
        if constexpr (kRules & kRulePenalties) {
            if (lap_mask & bit) t = t + pen->lap_sec[lap_first + (uint32_t)__popc(lap_mask & (bit - 1u))];
        }
        return t;
    }
};

// Simulations sim_offset + [0, m) of every scenario (gridDim.y = S), from the grid (kFromState false) or from `state`.
// hist [S][n][n] is ACCUMULATED into; stage [S][m][n] (classified position of each driver, | fate << 5 with penalties) is
// written, and, where wanted (NULL: not), ev_stage [S][m] (the packed event counts) with events and carried [S][m][n] u16
// at the drivers that have an UNTIL_STOP offset in the scenario with paces.  With weather event_laps [S][L + 1] holds the
// laps' condition bytes, lap_sec the [3][5] table and carried [S][m][n] u16 (NULL: not wanted) gets every driver's laps
// on the wrong tyres.  With grid edits pens holds the GridScenario [S] and carried [S][m][n] u16 (NULL: not wanted) gets
// every driver's start slot.  With priors pens holds the PriorScenario [S], carried [S][m][n] BYTES gets every driver's bin
// and ev_stage [S][m][n] FLOATS (NULL: not wanted) its offset.  Pointers of a rule set outside kRules are not read: pass NULL.
template <bool kFromState, uint32_t kRules>
__global__ void __launch_bounds__(512)
race_scenario_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state,
                     const StrategyScenario *__restrict__ scen, const StopLap *__restrict__ stop_laps,
                     const PenaltyScenario *__restrict__ pens, const PenaltyLap *__restrict__ pen_laps,
                     const uint8_t *__restrict__ event_laps, const PaceScenario *__restrict__ paces,
                     const PaceLap *__restrict__ pace_laps, const double *__restrict__ lap_sec, uint64_t m,
                     uint64_t sim_offset, uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist,
                     uint8_t *__restrict__ stage, uint32_t *__restrict__ ev_stage, uint16_t *__restrict__ carried,
                     uint32_t n_batches)
{
    static_assert(kRules == 0u || kRules == kRulePenalties || kRules == kRuleEvents || kRules == kRulePaces ||
                      kRules == kRuleAll || kRules == kRuleWeather || (kRules == kRuleGrid && !kFromState) ||
                      kRules == kRulePriors,
                  "the rule sets of the C ABI");
    constexpr bool kPen = (kRules & kRulePenalties) != 0u, kEv = (kRules & kRuleEvents) != 0u;
    constexpr bool kPace = (kRules & kRulePaces) != 0u, kWx = (kRules & kRuleWeather) != 0u;
    constexpr bool kGrid = (kRules & kRuleGrid) != 0u, kPri = (kRules & kRulePriors) != 0u;
    using Pace = std::conditional_t<kPace, OffsetPace,
                                    std::conditional_t<kWx, WeatherPace, std::conditional_t<kPri, PriorPace, ModelPace>>>;
    using Track = std::conditional_t<kWx, WeatherTrack, ModelTrack>;
    using Events = std::conditional_t<kEv, ForcedEvents, DrawnEvents>;
    using Observer = std::conditional_t<kEv, PackedEventCounter, NoLapObserver>;
    using Grid = std::conditional_t<kGrid, GridEdits, ModelGrid>;
    const uint32_t sid = blockIdx.y;
    const StrategyScenario *__restrict__ sc = scen + sid;
    const PenaltyScenario *__restrict__ pen = kPen ? pens + sid : nullptr;
    const PaceScenario *__restrict__ ps = kPace ? paces + sid : nullptr;
    const size_t lap0 = (size_t)sid * (size_t)(P->total_laps + 1);
    const PlanPit plan = {stop_laps + lap0, sc->planned, 0u, 0};
    const PenaltyLap *__restrict__ nl = kPen ? pen_laps + lap0 : nullptr;
    const PaceLap *__restrict__ pl = kPace ? pace_laps + lap0 : nullptr;
    Events forced;
    if constexpr (kEv) forced = {event_laps + lap0};
    Grid grid;
    if constexpr (kGrid) {
        const GridScenario *__restrict__ gs = reinterpret_cast<const GridScenario *>(pens) + sid;
        grid = {gs, gs->pit};
    }
    const PriorScenario *__restrict__ pri = kPri ? reinterpret_cast<const PriorScenario *>(pens) + sid : nullptr;
    const uint32_t serve = kPen ? pen->serve : 0u, flag = kPen ? pen->flag : 0u, until = kPace ? ps->until : 0u;
    run_block(P, m, n_batches, hist + (size_t)sid * (size_t)(P->n * P->n),
              [=](const Rows &s, const LapEnv &e, uint32_t *s_hist, uint64_t local) {
        const uint64_t sim = sim_offset + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);
        // the lane's place in the stagings: worked out here where events, paces or weather stage beside the position
        // bytes, after the race otherwise (the start slots are staged after the race too)
        uint64_t lane = 0, cell = 0;
        if constexpr (kEv || kPace || kWx || kPri) {
            lane = (uint64_t)sid * m + local;
            cell = lane * (uint64_t)e.n;
        }
        uint16_t *crow = (kPace || kWx) && carried ? carried + cell : nullptr;
        uint32_t served = 0u, active = until;
        Pace pace;
        if constexpr (kPace) pace = {pl, lap_sec, ps->until_sec, &active, 0u, 0u, 0u};
        Track trk;
        if constexpr (kWx) {
            pace = {event_laps + lap0, lap_sec, s, nullptr, 0u};
            trk = {event_laps + lap0, crow, 0u};
        }
        if constexpr (kPri) {
            // the lane's offsets, behind its rows; their bins and, where wanted, the floats are staged before the race
            float *x = reinterpret_cast<float *>(s.out + (size_t)e.n * s.B) + s.tid;
            float *offs = reinterpret_cast<float *>(ev_stage);
            draw_priors(pri, e.n, e.norm, c0, c1, seed_lo, seed_hi, x, s.B, reinterpret_cast<uint8_t *>(carried) + cell,
                        offs ? offs + cell : nullptr);
            pace = {x, s.B, pri->items};
        }
        const ScenarioPit<kRules> pit = {plan, pen, nl, pl, kPace ? ps->until_from : nullptr, &served, &active, crow, serve,
                                         0u, 0u, 0u};
        const RaceStart at = kFromState ? start_from_state(s, e, *state, c0, c1, seed_lo, seed_hi)
                                        : start_from_grid(s, e, c0, c1, seed_lo, seed_hi, nullptr, PlannedTyres{sc}, pace,
                                                          grid);
        if constexpr (kWx) {
            // lap 1's lap time, from the grid: on the start compound under the configuration's condition
            if (crow) {
                for (int d = 0; d < e.n; ++d) {
                    const uint32_t pk = s.Pk((uint32_t)d);
                    crow[d] = (uint16_t)(!kFromState && !(pk & kDnf) &&
                                         wrong_tyres((uint32_t)e.track, (pk >> kCompShift) & 7u));
                }
            }
        }
        Observer seen = {};
        run_laps(s, e, c0, c1, seed_lo, seed_hi, at.first_lap, at.drs_disabled_until, seen, pit, forced, pace,
                 trk);                                                                              // reference :166-228
        // at the flag: the unserved penalty, then the post-race one, of every running car.  A scenario without serve and
        // flag penalties skips the step: its field is sorted already
        uint32_t retired = 0u;
        if constexpr (kPen) {
            const uint32_t unserved = serve & ~served;
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
        }
        classify_and_count(s, e.n, s_hist, nullptr);                                                // reference :230-242
        // each driver's classified position and, with penalties, the fate of its serve penalty
        if constexpr (!(kEv || kPace || kWx || kPri)) cell = ((uint64_t)sid * m + local) * (uint64_t)e.n;
        uint8_t *row = stage + cell;
        for (int p = 0; p < e.n; ++p) {
            const uint32_t d = s.Ord(p);
            uint32_t b = (uint32_t)p;
            if constexpr (kPen) {
                const uint32_t bit = 1u << d;
                const uint32_t fate = !(serve & bit) ? kFateNone : (served & bit) ? kFateServed
                                      : (retired & bit) ? kFateRetired : kFateFlag;
                b |= fate << kStageFateShift;
            }
            row[d] = (uint8_t)b;
        }
        // each driver's start slot after the edits: its pk word keeps it to the flag
        if constexpr (kGrid) {
            if (carried) {
                uint16_t *srow = carried + cell;
                for (int d = 0; d < e.n; ++d) srow[d] = (uint16_t)gpos_of(s.Pk((uint32_t)d));
            }
        }
        if constexpr (kEv) {
            // mcgp_run_events always stages the word (its chunk budget counts it); only mcgp_run_combined can do without
            if (kRules == kRuleEvents || ev_stage) ev_stage[lane] = seen.packed;
        }
        // the offsets no stop cleared: carried up to the car's retirement, or to the flag
        if (kPace && crow) {
            for (uint32_t rest = active; rest; rest &= rest - 1u) {
                const uint32_t d = (uint32_t)__ffs((int)rest) - 1u, pk = s.Pk(d);
                const int from = (int)ps->until_from[d];
                const int end = (pk & kDnf) ? (int)(pk & kAgeMask) : e.L + 1;       // the first lap without a lap time
                crow[d] = (uint16_t)(end > from ? end - from : 0);
            }
        }
    });
}

// The instantiation behind a scenario call, for the launch and for its register count: `rules` is one of the five sets
// above, kRuleWeather, kRulePriors or, from the grid only, kRuleGrid (anything else: NULL), from the grid or from a state.
using ScenarioKernel = decltype(&race_scenario_kernel<false, 0u>);
inline ScenarioKernel scenario_kernel(uint32_t rules, bool from_state)
{
    switch (rules) {
    case 0u: return from_state ? &race_scenario_kernel<true, 0u> : &race_scenario_kernel<false, 0u>;
    case kRulePenalties:
        return from_state ? &race_scenario_kernel<true, kRulePenalties> : &race_scenario_kernel<false, kRulePenalties>;
    case kRuleEvents: return from_state ? &race_scenario_kernel<true, kRuleEvents> : &race_scenario_kernel<false, kRuleEvents>;
    case kRulePaces: return from_state ? &race_scenario_kernel<true, kRulePaces> : &race_scenario_kernel<false, kRulePaces>;
    case kRuleAll: return from_state ? &race_scenario_kernel<true, kRuleAll> : &race_scenario_kernel<false, kRuleAll>;
    case kRuleWeather:
        return from_state ? &race_scenario_kernel<true, kRuleWeather> : &race_scenario_kernel<false, kRuleWeather>;
    case kRuleGrid: return from_state ? nullptr : &race_scenario_kernel<false, kRuleGrid>;
    case kRulePriors:
        return from_state ? &race_scenario_kernel<true, kRulePriors> : &race_scenario_kernel<false, kRulePriors>;
    }
    return nullptr;
}

}  // namespace mcgp
