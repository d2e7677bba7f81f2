// event_pack.h -- host side of mcgp_run_events: a caller's mcgp_lap_event[] (include/mcgp.h) checked against the
// documented limits and packed into what race_scenario_kernel reads (one byte per scenario and lap, events.hip.h).
// Plain C++, no device code, beside plan_pack.h and penalty_pack.h and for the same reason: mcgp_hip.hip includes it for
// the C ABI, and the host debugging build of the generic kernels (tools/emu/emu_generic.cpp) includes the same text.
#pragma once
#include "plan_pack.h"
#include "events.hip.h"

namespace mcgp {

static_assert(MCGP_EVT_NONE == kEventNone && MCGP_EVT_RED_FLAG == kEventRed && MCGP_EVT_SAFETY_CAR == kEventSc &&
                  MCGP_EVT_VSC == kEventVsc && MCGP_MAX_SCENARIO_EVENTS == kMaxScenarioEvents,
              "the C ABI's event kinds are the kernel's");

// event_count [S] against the limit; "" if it passes.  *total = the overrides of all scenarios.
inline std::string check_event_counts(uint32_t n_scenarios, const uint32_t *event_count, uint64_t *total)
{
    *total = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        if (event_count[si] > mcgp::kMaxScenarioEvents)
            return "scenario " + std::to_string(si) + ": event_count must be in [0, 64]";
        *total += event_count[si];
    }
    return "";
}

// The overrides of mcgp_run_events in the kernel's encoding ([S][L + 1]: 0 = drawn, 1 + kind), checked against the
// limits of include/mcgp.h; "" if they pass, else the message (naming the scenario, the override and the field).
// first_lap: 2 from the grid, state lap + 1.  event_count has passed check_event_counts.
inline std::string pack_events(uint32_t n_scenarios, const uint32_t *event_count, const mcgp_lap_event *events,
                               int total_laps, int first_lap, bool from_state, std::vector<uint8_t> *laps)
{
    laps->assign((size_t)n_scenarios * (total_laps + 1), 0);
    size_t next = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        uint8_t *el = laps->data() + (size_t)si * (total_laps + 1);
        for (uint32_t ei = 0; ei < event_count[si]; ++ei, ++next) {
            const mcgp_lap_event &ev = events[next];
            const std::string at = "scenario " + std::to_string(si) + ", event " + std::to_string(ei) + ": ";
            if (ev.kind < MCGP_EVT_NONE || ev.kind > MCGP_EVT_VSC)
                return at + "kind must be MCGP_EVT_NONE, MCGP_EVT_RED_FLAG, MCGP_EVT_SAFETY_CAR or MCGP_EVT_VSC";
            const char *why = from_state ? " (after the state's lap)" : " (lap 1 has no event)";
            if (ev.first_lap < first_lap || ev.first_lap > total_laps)
                return at + "first_lap must be in [" + std::to_string(first_lap) + ", total_laps]" + why;
            if (ev.last_lap < first_lap || ev.last_lap > total_laps)
                return at + "last_lap must be in [" + std::to_string(first_lap) + ", total_laps]" + why;
            if (ev.first_lap > ev.last_lap) return at + "first_lap must not be above last_lap";
            for (int lap = ev.first_lap; lap <= ev.last_lap; ++lap) {
                if (el[lap])
                    return at + "first_lap..last_lap: lap " + std::to_string(lap) +
                           " has two overrides in this scenario";
                el[lap] = (uint8_t)(1 + ev.kind);
            }
        }
    }
    return "";
}

}  // namespace mcgp
