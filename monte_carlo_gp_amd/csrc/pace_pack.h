// pace_pack.h -- host side of mcgp_run_paces: a caller's mcgp_pace_offset[] (include/mcgp.h) checked against the
// documented limits and packed into what race_scenario_kernel reads (PaceScenario, PaceLap and the list of LAPS seconds,
// paces.hip.h).  Plain C++, no device code, beside plan_pack.h, penalty_pack.h and event_pack.h and for the same reason:
// mcgp_hip.hip includes it for the C ABI, and the host debugging build of the generic kernels
// (tools/emu/emu_generic.cpp) includes the same text.
#pragma once
#include "plan_pack.h"
#include "paces.hip.h"

namespace mcgp {

static_assert(MCGP_PACE_LAPS == kPaceLaps && MCGP_PACE_UNTIL_STOP == kPaceUntilStop &&
                  MCGP_MAX_SCENARIO_PACES == kMaxScenarioPaces,
              "the C ABI's pace kinds and limit are the kernel's");

// pace_count [S] against the limit; "" if it passes.  *total = the offsets of all scenarios.
inline std::string check_pace_counts(uint32_t n_scenarios, const uint32_t *pace_count, uint64_t *total)
{
    *total = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        if (pace_count[si] > mcgp::kMaxScenarioPaces)
            return "scenario " + std::to_string(si) + ": pace_count must be in [0, 64]";
        *total += pace_count[si];
    }
    return "";
}

// The offsets of mcgp_run_paces in the kernel's encoding, checked against the limits of include/mcgp.h; "" if they pass,
// else the message (naming the scenario, the offset and the field).  first_lap: 1 from the grid (lap 1 reads the base
// pace too), state lap + 1.  pace_count has passed check_pace_counts.  laps [S][L + 1]; lap_sec: the LAPS seconds by lap
// and then by driver, where consecutive laps of a scenario that the same offsets cover share their entries.
inline std::string pack_paces(uint32_t n_scenarios, const uint32_t *pace_count, const mcgp_pace_offset *paces, uint32_t n,
                              int total_laps, int first_lap, bool from_state, std::vector<mcgp::PaceScenario> *scen,
                              std::vector<mcgp::PaceLap> *laps, std::vector<double> *lap_sec)
{
    scen->assign(n_scenarios, mcgp::PaceScenario());
    laps->assign((size_t)n_scenarios * (total_laps + 1), mcgp::PaceLap());
    lap_sec->clear();
    std::vector<uint8_t> owner;                 // [L + 1][kMaxCars]: the LAPS offset that covers (lap, driver)
    size_t next = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        mcgp::PaceScenario &ps = (*scen)[si];
        std::memset(&ps, 0, sizeof(ps));
        mcgp::PaceLap *pl = laps->data() + (size_t)si * (total_laps + 1);
        const mcgp_pace_offset *mine = paces + next;
        owner.assign((size_t)(total_laps + 1) * mcgp::kMaxCars, 0);
        for (uint32_t pi = 0; pi < pace_count[si]; ++pi, ++next) {
            const mcgp_pace_offset &po = mine[pi];
            const std::string at = "scenario " + std::to_string(si) + ", offset " + std::to_string(pi) + ": ";
            if (po.kind != MCGP_PACE_LAPS && po.kind != MCGP_PACE_UNTIL_STOP)
                return at + "kind must be MCGP_PACE_LAPS or MCGP_PACE_UNTIL_STOP";
            if (po.driver < 0 || po.driver >= (int)n) return at + "driver must be in [0, n)";
            const std::string range = "[" + std::to_string(first_lap) + ", total_laps]" +
                                      (from_state ? " (after the state's lap)" : "");
            if (po.first_lap < first_lap || po.first_lap > total_laps) return at + "first_lap must be in " + range;
            if (po.kind == MCGP_PACE_LAPS) {
                if (po.last_lap < first_lap || po.last_lap > total_laps) return at + "last_lap must be in " + range;
                if (po.first_lap > po.last_lap) return at + "first_lap must not be above last_lap";
            } else if (po.last_lap != 0) {
                return at + "last_lap must be 0 with MCGP_PACE_UNTIL_STOP";
            }
            if (!std::isfinite(po.seconds) || std::fabs(po.seconds) > mcgp::kMaxPaceSeconds)
                return at + "seconds must be finite and in [-60, 60]";
            const uint32_t d = (uint32_t)po.driver, bit = 1u << d;
            if (po.kind == MCGP_PACE_UNTIL_STOP) {
                if (ps.until & bit)
                    return at + "driver " + std::to_string(d) + " has two MCGP_PACE_UNTIL_STOP offsets in this scenario";
                ps.until |= bit;
                ps.until_from[d] = (uint16_t)po.first_lap;
                ps.until_sec[d] = po.seconds;
                for (int lap = po.first_lap; lap <= total_laps; ++lap) pl[lap].until |= bit;
                continue;
            }
            for (int lap = po.first_lap; lap <= po.last_lap; ++lap) {
                if (pl[lap].mask & bit)
                    return at + "first_lap..last_lap: driver " + std::to_string(d) + " has two MCGP_PACE_LAPS offsets on lap " +
                           std::to_string(lap) + " in this scenario";
                pl[lap].mask |= bit;
                owner[(size_t)lap * mcgp::kMaxCars + d] = (uint8_t)pi;
            }
        }
        // the LAPS seconds, by lap and then by driver; a lap that the previous lap's offsets cover reuses its entries
        for (int lap = 1; lap <= total_laps; ++lap) {
            if (!pl[lap].mask) continue;
            const uint8_t *own = owner.data() + (size_t)lap * mcgp::kMaxCars;
            if (pl[lap - 1].mask == pl[lap].mask && std::memcmp(own - mcgp::kMaxCars, own, mcgp::kMaxCars) == 0) {
                pl[lap].first = pl[lap - 1].first;
                continue;
            }
            pl[lap].first = (uint32_t)lap_sec->size();
            for (uint32_t d = 0; d < n; ++d)
                if ((pl[lap].mask >> d) & 1u) lap_sec->push_back(mine[own[d]].seconds);
        }
    }
    if (lap_sec->empty()) lap_sec->push_back(0.0);          // never read: no lap has a bit set
    return "";
}

}  // namespace mcgp
