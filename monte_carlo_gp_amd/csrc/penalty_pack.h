// penalty_pack.h -- host side of mcgp_run_penalties: a caller's mcgp_time_penalty[] (include/mcgp.h) checked against the
// documented limits and packed into what race_scenario_kernel reads (PenaltyScenario and PenaltyLap, penalties.hip.h).
// Plain C++, no device code, beside plan_pack.h and for the same reason: mcgp_hip.hip includes it for the C ABI, and the
// host debugging build of the generic kernels (tools/emu/emu_generic.cpp) includes the same text.
#pragma once
#include "plan_pack.h"
#include "penalties.hip.h"

namespace mcgp {

// penalty_count [S] against the limit; "" if it passes.  *total = the penalties of all scenarios.
inline std::string check_penalty_counts(uint32_t n_scenarios, const uint32_t *penalty_count, uint64_t *total)
{
    *total = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        if (penalty_count[si] > mcgp::kMaxScenarioPenalties)
            return "scenario " + std::to_string(si) + ": penalty_count must be in [0, 256]";
        *total += penalty_count[si];
    }
    return "";
}

// The penalties of mcgp_run_penalties in the kernel's encoding, checked against the limits of include/mcgp.h; "" if they
// pass, else the message (naming the scenario, the penalty and the field).  first_lap: 2 from the grid, state lap + 1.
// penalty_count has passed check_penalty_counts.
inline std::string pack_penalties(uint32_t n_scenarios, const uint32_t *penalty_count, const mcgp_time_penalty *penalties,
                                  uint32_t n, int total_laps, int first_lap, bool from_state,
                                  std::vector<mcgp::PenaltyScenario> *pens, std::vector<mcgp::PenaltyLap> *laps)
{
    pens->assign(n_scenarios, mcgp::PenaltyScenario());
    laps->assign((size_t)n_scenarios * (total_laps + 1), mcgp::PenaltyLap());
    size_t next = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        mcgp::PenaltyScenario &ps = (*pens)[si];
        std::memset(&ps, 0, sizeof(ps));
        mcgp::PenaltyLap *pl = laps->data() + (size_t)si * (total_laps + 1);
        const mcgp_time_penalty *mine = penalties + next;
        for (uint32_t pi = 0; pi < penalty_count[si]; ++pi, ++next) {
            const mcgp_time_penalty &pn = mine[pi];
            const std::string at = "scenario " + std::to_string(si) + ", penalty " + std::to_string(pi) + ": ";
            if (pn.kind != MCGP_PEN_SERVE_AT_STOP && pn.kind != MCGP_PEN_AT_FLAG && pn.kind != MCGP_PEN_ON_LAP)
                return at + "kind must be MCGP_PEN_SERVE_AT_STOP, MCGP_PEN_AT_FLAG or MCGP_PEN_ON_LAP";
            if (pn.driver < 0 || pn.driver >= (int)n) return at + "driver must be in [0, n)";
            if (!std::isfinite(pn.seconds) || !(pn.seconds > 0.0) || pn.seconds > 1e6)
                return at + "seconds must be finite and in (0, 1e6]";
            const uint32_t d = (uint32_t)pn.driver, bit = 1u << d;
            if (pn.kind == MCGP_PEN_AT_FLAG) {
                if (pn.lap != 0) return at + "lap must be 0 with MCGP_PEN_AT_FLAG";
                if (ps.flag & bit)
                    return at + "driver " + std::to_string(d) + " has two MCGP_PEN_AT_FLAG penalties in this scenario (sum them)";
                ps.flag |= bit;
                ps.flag_sec[d] = pn.seconds;
                continue;
            }
            if (pn.lap < first_lap || pn.lap > total_laps)
                return at + "lap must be in [" + std::to_string(first_lap) + ", total_laps]" +
                       (from_state ? " (after the state's lap)" : " (lap 1 has no pit step)");
            if (pn.kind == MCGP_PEN_SERVE_AT_STOP) {
                if (ps.serve & bit)
                    return at + "driver " + std::to_string(d) +
                           " has two MCGP_PEN_SERVE_AT_STOP penalties in this scenario (sum them)";
                ps.serve |= bit;
                ps.serve_from[d] = (uint16_t)pn.lap;
                ps.serve_sec[d] = pn.seconds;
            } else {
                if (pl[pn.lap].mask & bit)
                    return at + "driver " + std::to_string(d) + " has two MCGP_PEN_ON_LAP penalties on lap " +
                           std::to_string(pn.lap) + " in this scenario (sum them)";
                pl[pn.lap].mask |= bit;
            }
        }
        // the ON_LAP seconds, by lap and then by driver
        uint32_t first = 0;
        for (int lap = 0; lap <= total_laps; ++lap) {
            pl[lap].first = first;
            first += (uint32_t)__builtin_popcount(pl[lap].mask);
        }
        for (uint32_t pi = 0; pi < penalty_count[si]; ++pi) {
            const mcgp_time_penalty &pn = mine[pi];
            if (pn.kind != MCGP_PEN_ON_LAP) continue;
            const uint32_t below = pl[pn.lap].mask & ((1u << (uint32_t)pn.driver) - 1u);
            ps.lap_sec[pl[pn.lap].first + (uint32_t)__builtin_popcount(below)] = pn.seconds;
        }
    }
    return "";
}

}  // namespace mcgp
