// weather_pack.h -- host side of mcgp_run_weather: a caller's mcgp_track_change[] and mcgp_weather_model (include/mcgp.h)
// checked against the documented limits and packed into what race_scenario_kernel reads (one byte per scenario and lap
// and the table of seconds, weather.hip.h).  Plain C++, no device code, beside plan_pack.h, penalty_pack.h, event_pack.h
// and pace_pack.h and for the same reason: mcgp_hip.hip includes it for the C ABI, and the host debugging build of the
// generic kernels (tools/emu/emu_generic.cpp) includes the same text.
#pragma once
#include "plan_pack.h"
#include "weather.hip.h"

namespace mcgp {

static_assert(MCGP_MAX_SCENARIO_TRACK_CHANGES == kMaxScenarioTrackChanges && MCGP_WET_TRACK == kTrackConditions - 1 &&
                  MCGP_WET == kCompounds - 1 &&
                  sizeof(mcgp_weather_model) == sizeof(double) * kTrackConditions * kCompounds,
              "the C ABI's limit, conditions, compounds and table are the kernel's");

// change_count [S] against the limit; "" if it passes.  *total = the changes of all scenarios.
inline std::string check_change_counts(uint32_t n_scenarios, const uint32_t *change_count, uint64_t *total)
{
    *total = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        if (change_count[si] > mcgp::kMaxScenarioTrackChanges)
            return "scenario " + std::to_string(si) + ": change_count must be in [0, 64]";
        *total += change_count[si];
    }
    return "";
}

// The changes and the model of mcgp_run_weather in the kernel's encoding, checked against the limits of include/mcgp.h;
// "" if they pass, else the message (naming the scenario, the change and the field, or the table entry).  track: the
// configuration's condition (checked by then).  first_lap: 2 from the grid, state lap + 1.  change_count has passed
// check_change_counts.  laps [S][L + 1]: every lap's condition, with bit kCondLiveShift + k set where the table's entry of
// the condition and compound k is non-zero; table [3][5].
inline std::string pack_weather(uint32_t n_scenarios, const uint32_t *change_count, const mcgp_track_change *changes,
                                const mcgp_weather_model *model, int track, int total_laps, int first_lap, bool from_state,
                                std::vector<uint8_t> *laps, std::vector<double> *table)
{
    if (!model) return "model is NULL";
    table->clear();
    uint8_t byte_of[mcgp::kTrackConditions];
    for (int c = 0; c < mcgp::kTrackConditions; ++c) {
        byte_of[c] = (uint8_t)c;
        for (int k = 0; k < mcgp::kCompounds; ++k) {
            const double sec = model->wrong_tyre_sec[c][k];
            if (!std::isfinite(sec) || sec < 0.0 || sec > mcgp::kMaxWrongTyreSeconds)
                return "model: wrong_tyre_sec[" + std::to_string(c) + "][" + std::to_string(k) +
                       "] must be finite and in [0, 60]";
            if (sec != 0.0) byte_of[c] |= (uint8_t)(1u << (mcgp::kCondLiveShift + k));
            table->push_back(sec);
        }
    }
    laps->assign((size_t)n_scenarios * (total_laps + 1), byte_of[track]);
    std::vector<uint8_t> covered;
    size_t next = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        uint8_t *cl = laps->data() + (size_t)si * (total_laps + 1);
        covered.assign((size_t)total_laps + 1, 0);
        for (uint32_t ci = 0; ci < change_count[si]; ++ci, ++next) {
            const mcgp_track_change &ch = changes[next];
            const std::string at = "scenario " + std::to_string(si) + ", change " + std::to_string(ci) + ": ";
            if (ch.condition < MCGP_DRY || ch.condition > MCGP_WET_TRACK)
                return at + "condition must be MCGP_DRY, MCGP_DAMP or MCGP_WET_TRACK";
            const char *why = from_state ? " (after the state's lap)" : " (lap 1 has the configuration's condition)";
            if (ch.first_lap < first_lap || ch.first_lap > total_laps)
                return at + "first_lap must be in [" + std::to_string(first_lap) + ", total_laps]" + why;
            if (ch.last_lap < first_lap || ch.last_lap > total_laps)
                return at + "last_lap must be in [" + std::to_string(first_lap) + ", total_laps]" + why;
            if (ch.first_lap > ch.last_lap) return at + "first_lap must not be above last_lap";
            for (int lap = ch.first_lap; lap <= ch.last_lap; ++lap) {
                if (covered[lap])
                    return at + "first_lap..last_lap: lap " + std::to_string(lap) + " has two changes in this scenario";
                covered[lap] = 1;
                cl[lap] = byte_of[ch.condition];
            }
        }
    }
    return "";
}

}  // namespace mcgp
