// plan_pack.h -- host side of mcgp_run_from_state and mcgp_run_strategies: a caller's mcgp_race_state and mcgp_pit_plan[]
// (include/mcgp.h) checked against the documented limits and packed into what the kernels read (ResumeState,
// resume.hip.h; StrategyScenario and StopLap, strategy.hip.h).  Plain C++, no device code: mcgp_hip.hip includes it for
// the C ABI, and the host debugging build of the generic kernels (tools/emu/emu_generic.cpp) includes the same text,
// so that what a test packs on the CPU is what the library packs.
#pragma once
#include "../../include/mcgp.h"
#include "strategy.hip.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace mcgp {

// One mcgp_race_state in the resume kernel's encoding, checked against the limits of include/mcgp.h; "" if it passes,
// else the message (naming the field and state `si`).
inline std::string pack_race_state(const mcgp_race_state &rs, uint32_t si, uint32_t n, int total_laps,
                                   mcgp::ResumeState *out)
{
    const std::string at = "state " + std::to_string(si) + ": ";
    if (rs.lap < 1 || rs.lap > total_laps) return at + "lap must be in [1, total_laps]";
    if (rs.drs_disabled_until < 0 || rs.drs_disabled_until > total_laps + 2)
        return at + "drs_disabled_until must be in [0, total_laps + 2]";
    if (!rs.cumulative_time) return at + "cumulative_time is NULL";
    if (!rs.last_lap_time) return at + "last_lap_time is NULL";
    if (!rs.grid_slot) return at + "grid_slot is NULL";
    if (!rs.compound) return at + "compound is NULL";
    if (!rs.used_compounds) return at + "used_compounds is NULL";
    if (!rs.tire_age) return at + "tire_age is NULL";
    if (!rs.retired_lap) return at + "retired_lap is NULL";
    const int max_age = (int)mcgp::kAgeMask - (total_laps - rs.lap);
    uint32_t seen = 0;
    std::memset(out, 0, sizeof(*out));
    for (uint32_t d = 0; d < n; ++d) {
        const std::string car = at + "car " + std::to_string(d) + ": ";
        if (!std::isfinite(rs.cumulative_time[d])) return car + "cumulative_time is not finite";
        if (!std::isfinite(rs.last_lap_time[d])) return car + "last_lap_time is not finite";
        const uint32_t g = rs.grid_slot[d];
        if (g >= n || ((seen >> g) & 1u)) return car + "grid_slot is not a permutation of 0..n-1";
        seen |= 1u << g;
        const uint32_t comp = rs.compound[d];
        if (comp > MCGP_WET) return car + "compound must be in [MCGP_SOFT, MCGP_WET]";
        const uint32_t used = rs.used_compounds[d];
        if (used > 31u || !((used >> comp) & 1u)) return car + "used_compounds must be a subset of the 5 compounds that contains compound";
        const int age = rs.tire_age[d];
        if (age < 0 || age > max_age) return car + "tire_age must be in [0, 1023 - (total_laps - lap)]";
        const int ret = rs.retired_lap[d];
        if (ret < 0 || ret > rs.lap) return car + "retired_lap must be in [0, lap]";
        uint32_t pk = (comp << mcgp::kCompShift) | (used << mcgp::kUsedShift) | (g << mcgp::kGposShift);
        pk |= ret ? (mcgp::kDnf | (uint32_t)ret) : (uint32_t)age;       // a retired car's age field holds its lap
        out->cum[d] = rs.cumulative_time[d];
        out->last[d] = rs.last_lap_time[d];
        out->pk[d] = pk;
    }
    out->lap = rs.lap;
    out->drs_disabled_until = rs.drs_disabled_until;
    return "";
}

// The scenarios of mcgp_run_strategies in the kernel's encoding, checked against the limits of include/mcgp.h; "" if
// they pass, else the message (naming the scenario, the plan and the field).  first_lap: 2 from the grid, state lap + 1.
inline std::string pack_scenarios(uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans, uint32_t n,
                           int total_laps, int first_lap, bool from_state, std::vector<mcgp::StrategyScenario> *scen,
                           std::vector<mcgp::StopLap> *laps)
{
    scen->assign(n_scenarios, mcgp::StrategyScenario());
    laps->assign((size_t)n_scenarios * (total_laps + 1), mcgp::StopLap());
    size_t next = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        mcgp::StrategyScenario &sc = (*scen)[si];
        sc.planned = 0u;
        sc.pad = 0u;
        for (int d = 0; d < mcgp::kMaxCars; ++d) sc.start[d] = mcgp::kModelStart;
        mcgp::StopLap *sl = laps->data() + (size_t)si * (total_laps + 1);
        for (uint32_t pi = 0; pi < plan_count[si]; ++pi, ++next) {
            const mcgp_pit_plan &pl = plans[next];
            const std::string at = "scenario " + std::to_string(si) + ", plan " + std::to_string(pi) + ": ";
            if (pl.driver < 0 || pl.driver >= (int)n) return at + "driver must be in [0, n)";
            const uint32_t d = (uint32_t)pl.driver;
            if ((sc.planned >> d) & 1u) return at + "driver " + std::to_string(d) + " has two plans in this scenario";
            sc.planned |= 1u << d;
            if (from_state) {
                if (pl.start_compound != -1 || pl.start_age != 0)
                    return at + "start_compound / start_age: a state fixes the tyres (start_compound must be -1, start_age 0)";
            } else if (pl.start_compound == -1) {
                if (pl.start_age != 0) return at + "start_age must be 0 with start_compound -1";
            } else {
                if (pl.start_compound < MCGP_SOFT || pl.start_compound > MCGP_WET)
                    return at + "start_compound must be -1 or in [MCGP_SOFT, MCGP_WET]";
                if (pl.start_age < 0 || pl.start_age > (int)mcgp::kAgeMask - total_laps)
                    return at + "start_age must be in [0, 1023 - total_laps]";
                sc.start[d] = (uint16_t)((uint32_t)pl.start_compound | ((uint32_t)pl.start_age << 3));
            }
            if (pl.n_stops > (uint32_t)mcgp::kMaxPlanStops) return at + "n_stops must be in [0, 8]";
            int prev = 0;
            for (uint32_t k = 0; k < pl.n_stops; ++k) {
                const std::string stop = at + "stop " + std::to_string(k) + ": ";
                const int lap = pl.stop_lap[k];
                if (lap < first_lap || lap > total_laps)
                    return stop + "stop_lap must be in [" + std::to_string(first_lap) + ", total_laps]" +
                           (from_state ? " (after the state's lap)" : " (lap 1 has no pit step)");
                if (lap <= prev) return stop + "stop_lap must be strictly increasing";
                prev = lap;
                const uint32_t comp = pl.stop_compound[k];
                if (comp > MCGP_WET) return stop + "stop_compound must be in [MCGP_SOFT, MCGP_WET]";
                sl[lap].mask |= 1u << d;
                sl[lap].comp[d >> 3] |= comp << (4u * (d & 7u));
            }
        }
    }
    return "";
}

}  // namespace mcgp
