// prior_pack.h -- host side of mcgp_run_priors: a caller's mcgp_pace_prior[] and edges (include/mcgp.h) checked against
// the documented limits and packed into what race_scenario_kernel reads (one PriorScenario per scenario, priors.hip.h).
// Plain C++, no device code, beside plan_pack.h, penalty_pack.h, event_pack.h, pace_pack.h, weather_pack.h and
// grid_pack.h and for the same reason: mcgp_hip.hip includes it for the C ABI, and the host debugging build of the
// generic kernels (tools/emu/emu_generic.cpp) includes the same text.
#pragma once
#include "plan_pack.h"
#include "priors.hip.h"

namespace mcgp {

static_assert(MCGP_PRIOR_DRIVER == kPriorDriver && MCGP_PRIOR_GROUP == kPriorGroup &&
                  MCGP_MAX_SCENARIO_PRIORS == kMaxScenarioPriors && MCGP_MAX_PRIOR_EDGES == kMaxPriorEdges,
              "the C ABI's prior kinds and limits are the kernel's");

// prior_count [S] against the limit; "" if it passes.  *total = the items of all scenarios.
inline std::string check_prior_counts(uint32_t n_scenarios, const uint32_t *prior_count, uint64_t *total)
{
    *total = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        if (prior_count[si] > kMaxScenarioPriors)
            return "scenario " + std::to_string(si) + ": prior_count must be in [0, 64]";
        *total += prior_count[si];
    }
    return "";
}

// The call's edges; "" if they pass.
inline std::string check_prior_edges(uint32_t n_edges, const double *edges)
{
    if (n_edges > kMaxPriorEdges) return "n_edges must be in [0, 15]";
    if (n_edges && !edges) return "edges is NULL";
    for (uint32_t i = 0; i < n_edges; ++i) {
        if (!std::isfinite(edges[i])) return "edges[" + std::to_string(i) + "] must be finite";
        if (i && !(edges[i] > edges[i - 1])) return "edges[" + std::to_string(i) + "] must be above edges[" + std::to_string(i - 1) + "]";
    }
    return "";
}

// The items of mcgp_run_priors in the kernel's encoding, checked against the limits of include/mcgp.h; "" if they pass,
// else the message (naming the scenario, the item and the field).  prior_count has passed check_prior_counts and the
// edges check_prior_edges.
inline std::string pack_priors(uint32_t n_scenarios, const uint32_t *prior_count, const mcgp_pace_prior *priors, uint32_t n,
                               uint32_t n_edges, const double *edges, std::vector<PriorScenario> *out)
{
    out->assign(n_scenarios, PriorScenario{});
    const uint32_t all = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
    size_t next = 0;
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        PriorScenario &p = (*out)[si];
        p.n_edges = n_edges;
        for (uint32_t i = 0; i < n_edges; ++i) p.edges[i] = edges[i];
        for (uint32_t pi = 0; pi < prior_count[si]; ++pi, ++next) {
            const mcgp_pace_prior &it = priors[next];
            const std::string at = "scenario " + std::to_string(si) + ", item " + std::to_string(pi) + ": ";
            if (it.kind != MCGP_PRIOR_DRIVER && it.kind != MCGP_PRIOR_GROUP)
                return at + "kind must be MCGP_PRIOR_DRIVER or MCGP_PRIOR_GROUP";
            if (!std::isfinite(it.sigma) || it.sigma < 0.0 || it.sigma > kMaxPriorSigma)
                return at + "sigma must be finite and in [0, 10]";
            if (it.kind == MCGP_PRIOR_DRIVER) {
                if (it.driver < 0 || it.driver >= (int32_t)n) return at + "driver must be in [0, n)";
                if (it.members != 0u) return at + "members must be 0 for MCGP_PRIOR_DRIVER";
                const uint32_t d = (uint32_t)it.driver, bit = 1u << d;
                if (p.own & bit) return at + "driver " + std::to_string(d) + " has two MCGP_PRIOR_DRIVER items in this scenario";
                p.own |= bit;
                p.sigma_own[d] = it.sigma;
                continue;
            }
            if (it.driver != 0) return at + "driver must be 0 for MCGP_PRIOR_GROUP";
            if (it.members == 0u) return at + "members must have at least one bit";
            if (it.members & ~all) return at + "members must have no bit at or above n";
            if (it.members & p.grouped) {
                const uint32_t both = it.members & p.grouped;
                return at + "members: driver " + std::to_string(__builtin_ctz(both)) + " is in two groups in this scenario";
            }
            const uint32_t low = (uint32_t)__builtin_ctz(it.members);
            p.grouped |= it.members;
            p.lows |= 1u << low;
            for (uint32_t m = it.members; m; m &= m - 1u) {
                const uint32_t d = (uint32_t)__builtin_ctz(m);
                p.low_of[d] = (uint8_t)low;
                p.sigma_grp[d] = it.sigma;
            }
        }
        p.items = prior_count[si];
    }
    return "";
}

}  // namespace mcgp
