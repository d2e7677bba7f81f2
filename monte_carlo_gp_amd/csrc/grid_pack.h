// grid_pack.h -- host side of mcgp_run_grids: a caller's mcgp_grid_edit[] (include/mcgp.h) checked against the documented
// limits and packed into what race_scenario_kernel reads (one GridScenario per scenario, grids.hip.h).  Plain C++, no
// device code, beside plan_pack.h, penalty_pack.h, event_pack.h, pace_pack.h and weather_pack.h and for the same reason:
// mcgp_hip.hip includes it for the C ABI, and the host debugging build of the generic kernels
// (tools/emu/emu_generic.cpp) includes the same text.
#pragma once
#include "plan_pack.h"
#include "grids.hip.h"

namespace mcgp {

static_assert(MCGP_GRID_DROP == kGridDrop && MCGP_GRID_PIN == kGridPin && MCGP_GRID_PIT_LANE == kGridPitLane,
              "the C ABI's kinds are the kernel's");

// edit_count [S] against the limit (one edit per driver); "" if it passes.  *total = the edits of all scenarios.
inline std::string check_edit_counts(uint32_t n_scenarios, const uint32_t *edit_count, uint32_t n, uint64_t *total)
{
    *total = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        if (edit_count[si] > n)
            return "scenario " + std::to_string(si) + ": edit_count must be in [0, n] (one edit per driver)";
        *total += edit_count[si];
    }
    return "";
}

// The edits of mcgp_run_grids in the kernel's encoding, checked against the limits of include/mcgp.h; "" if they pass,
// else the message (naming the scenario, the edit and the field).  edit_count has passed check_edit_counts.
inline std::string pack_grids(uint32_t n_scenarios, const uint32_t *edit_count, const mcgp_grid_edit *edits, uint32_t n,
                              std::vector<GridScenario> *out)
{
    out->assign(n_scenarios, GridScenario{});
    const uint32_t all = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
    size_t next = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        GridScenario &g = (*out)[si];
        uint32_t edited = 0u, pinned_slots = 0u;
        int pin_edit[kMaxCars];                 // the edit that pinned a slot
        const size_t first = next;
        for (uint32_t ei = 0; ei < edit_count[si]; ++ei, ++next) {
            const mcgp_grid_edit &ed = edits[next];
            const std::string at = "scenario " + std::to_string(si) + ", edit " + std::to_string(ei) + ": ";
            if (ed.driver < 0 || ed.driver >= (int32_t)n) return at + "driver must be in [0, n)";
            const uint32_t bit = 1u << ed.driver;
            if (ed.kind < MCGP_GRID_DROP || ed.kind > MCGP_GRID_PIT_LANE)
                return at + "kind must be MCGP_GRID_DROP, MCGP_GRID_PIN or MCGP_GRID_PIT_LANE";
            if (ed.kind == MCGP_GRID_DROP && (ed.value < 1 || ed.value > (int32_t)kMaxGridDrop))
                return at + "value must be in [1, 255] places for MCGP_GRID_DROP";
            if (ed.kind == MCGP_GRID_PIN && (ed.value < 1 || ed.value > (int32_t)n))
                return at + "value must be a slot in [1, n] for MCGP_GRID_PIN";
            if (ed.kind == MCGP_GRID_PIT_LANE && ed.value != 0) return at + "value must be 0 for MCGP_GRID_PIT_LANE";
            if (ed.kind == MCGP_GRID_PIT_LANE) {
                if (!std::isfinite(ed.seconds) || ed.seconds < 0.0 || ed.seconds > kMaxPitLaneSeconds)
                    return at + "seconds must be finite and in [0, 1e6]";
            } else if (!(ed.seconds == 0.0)) {
                return at + "seconds must be 0 for MCGP_GRID_DROP and MCGP_GRID_PIN";
            }
            if (edited & bit) return at + "driver " + std::to_string(ed.driver) + " has two edits in this scenario";
            edited |= bit;
            if (ed.kind == MCGP_GRID_DROP) {
                g.value[ed.driver] = (uint8_t)ed.value;
            } else if (ed.kind == MCGP_GRID_PIN) {
                const uint32_t slot = (uint32_t)ed.value - 1u;
                if (pinned_slots & (1u << slot))
                    return at + "value: slot " + std::to_string(ed.value) + " is pinned by edit " +
                           std::to_string(pin_edit[slot]) + " of this scenario too";
                pinned_slots |= 1u << slot;
                pin_edit[slot] = (int)ei;
                g.pin |= bit;
                g.value[ed.driver] = (uint8_t)slot;
            } else {
                g.pit |= bit;
                g.seconds[ed.driver] = ed.seconds;
            }
        }
        // a pin must lie in front of the pit-lane slots, the last popcount(pit) of the grid
        uint32_t n_pit = 0;
        for (uint32_t m = g.pit; m; m &= m - 1u) ++n_pit;
        const uint32_t front = n_pit >= 32 ? 0u : (all >> n_pit);
        for (uint32_t ei = 0; ei < edit_count[si]; ++ei) {
            const mcgp_grid_edit &ed = edits[first + ei];
            if (ed.kind == MCGP_GRID_PIN && !((front >> (ed.value - 1)) & 1u))
                return "scenario " + std::to_string(si) + ", edit " + std::to_string(ei) + ": value: slot " +
                       std::to_string(ed.value) + " is one of the last " + std::to_string(n_pit) +
                       ", which the scenario's pit-lane starters take";
        }
        g.edits = edit_count[si];
        g.free_slots = front & ~pinned_slots;
    }
    return "";
}

}  // namespace mcgp
