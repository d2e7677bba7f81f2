// emu_generic.cpp -- DEBUGGING build of the generic kernel family's source for the host (not product code, not a
// fallback: nothing in monte_carlo_gp_amd/ can reach it).  Compiles csrc/race_kernel.hip.h, resume.hip.h, trace.hip.h,
// gaps.hip.h, pit_window.hip.h, conditions.hip.h, stints.hip.h, moves.hip.h, fastest.hip.h and scenario.hip.h (with strategy.hip.h,
// penalties.hip.h, events.hip.h, paces.hip.h, weather.hip.h, grids.hip.h and priors.hip.h) with g++ through the stand-in <hip/hip_runtime.h> of this directory and
// calls the real __global__ functions: race_kernel, race_resume_kernel, race_trace_kernel, race_gaps_kernel<false / true>,
// race_window_kernel<false / true>,
// race_conditions_kernel<false / true>, conditions_count, race_stints_kernel<false / true>, race_moves_kernel<false /
// true>, race_fastest_kernel, the fifteen instantiations of race_scenario_kernel, penalties_count, events_count,
// paces_count, weather_count, grid_count, priors_count.
//
// Execution model: these kernels give one simulation to a lane and have no cross-lane operation, only
// __syncthreads() between "load tables", "simulate" and "flush".  With blockDim = gridDim.x = 1 and n_batches = n_sims
// a kernel is an ordinary host function that walks the simulations one after another (the no-op __syncthreads() of the
// stand-in header is correct for a block of one thread); blockIdx.y (states, scenarios) is looped over here.  The
// state and plan arguments go through csrc/plan_pack.h, the text the C ABI itself uses.
//
// Not run here: trace_count_positions, gaps_count_rows, window_count_rows and moves_count_laps (__shfl_down), the matchups kernel and
// stints_count (__ballot), moves_count_drivers (a fixed block of 256 threads), and
// trace_count_laps, trace_count_records and strategy_count_deltas, whose loops are written for their fixed block of 256
// threads (a one-thread block would visit a 256th of the data).  The tests derive the counts from the staging bytes and
// records in numpy instead; the counting kernels are compared on the device.  conditions_count has no cross-lane
// operation and strides by its block's size, so it does run here, as blocks of one thread; so do penalties_count, events_count
// paces_count, weather_count, grid_count and priors_count.
//
// Shared text: the six analysis calls (emu_generic_trace, emu_gaps_run, emu_window_run, emu_conditions_run,
// emu_stints_run, emu_moves_run) start with analysis_setup, the eight scenario calls are scenario_run with their rule sets.
//
// Used by tests/test_generic_host_build.py (race, resume, trace, strategies) and by tests/test_<call>_host_build.py for
// gaps, pit_window, conditions, stints, moves, fastest, penalties, events, paces, combined, weather, grids and priors, each through its helper
// tests/<call>_host_build.py (tests/kernel_host_build.py compiles this file); the stand-alone programs
// tools/emu/sanitize_{penalties,events,paces,combined,bonus,weather,grids,priors}_main.cpp are built with it for
// tests/test_{penalties,events,paces,combined,fastest,weather,grids,priors}_sanitize.py.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../monte_carlo_gp_amd/csrc/params_build.h"
#include "../../monte_carlo_gp_amd/csrc/trace.hip.h"
#include "../../monte_carlo_gp_amd/csrc/gaps.hip.h"
#include "../../monte_carlo_gp_amd/csrc/pit_window.hip.h"
#include "../../monte_carlo_gp_amd/csrc/conditions.hip.h"
#include "../../monte_carlo_gp_amd/csrc/stints.hip.h"
#include "../../monte_carlo_gp_amd/csrc/moves.hip.h"
#include "../../monte_carlo_gp_amd/csrc/fastest.hip.h"
#include "../../monte_carlo_gp_amd/csrc/plan_pack.h"
#include "../../monte_carlo_gp_amd/csrc/penalty_pack.h"
#include "../../monte_carlo_gp_amd/csrc/event_pack.h"
#include "../../monte_carlo_gp_amd/csrc/pace_pack.h"
#include "../../monte_carlo_gp_amd/csrc/weather_pack.h"
#include "../../monte_carlo_gp_amd/csrc/grid_pack.h"
#include "../../monte_carlo_gp_amd/csrc/prior_pack.h"
#include "../../monte_carlo_gp_amd/csrc/scenario.hip.h"

emu_dim3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0}, blockDim{1, 1, 1}, gridDim{1, 1, 1};
namespace mcgp {
alignas(16) unsigned char smem[1 << 20];
}

namespace {

std::string g_err;

int fail(int rc, const std::string &msg, const char **err)
{
    g_err = msg;
    *err = g_err.c_str();
    return rc;
}

// The parameter block of a call, as the C ABI builds it.  The generic kernels are the 32-bit-deviate build.
int params(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n, mcgp::KParams *kp,
           const char **err)
{
    static const char *none = "";
    *err = none;
    const char *e = "";
    const int rc = mcgp::build_params(cfg, drv, grid_probs, n, kp, &e);
    if (rc != MCGP_OK) return fail(rc, e, err);
    if (kp->wide) return fail(MCGP_E_BAD_ARG, "the generic kernels run MCGP_DEVIATES_32", err);
    return MCGP_OK;
}

void one_thread_block(uint32_t grid_y)
{
    threadIdx = {0, 0, 0};
    blockIdx = {0, 0, 0};
    blockDim = {1, 1, 1};
    gridDim = {1, grid_y, 1};
}

// The start of the six analysis calls (trace, gaps, pit windows, conditions, stints, moves): the parameter block, the source (a state
// or grid_probs; the trace passes no state, so it needs grid_probs), the call's own complaint `own` (NULL: none), the
// staging's stride (masks: conditions' u64 masks sit behind the rows, so a multiple of 8), the state as the kernels read
// it (zero from the grid) and a block of one thread.
int analysis_setup(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                   uint32_t n, uint64_t n_sims, uint64_t stride, bool masks, const char *own, mcgp::KParams *kp,
                   mcgp::ResumeState *st, const char **err)
{
    const int rc = params(cfg, drv, grid_probs, n, kp, err);
    if (rc != MCGP_OK) return rc;
    if ((state != nullptr) == (grid_probs != nullptr)) return fail(MCGP_E_BAD_ARG, "either a state or grid_probs", err);
    if (own) return fail(MCGP_E_BAD_ARG, own, err);
    if (masks && (stride < n_sims || stride % 8))
        return fail(MCGP_E_BAD_ARG, "stride must be at least n_sims and a multiple of 8", err);
    if (stride < n_sims) return fail(MCGP_E_BAD_ARG, "stride must be at least n_sims", err);
    std::memset(st, 0, sizeof(*st));
    if (state) {
        const std::string e = mcgp::pack_race_state(*state, 0, n, cfg->total_laps, st);
        if (!e.empty()) return fail(MCGP_E_BAD_ARG, e, err);
    }
    one_thread_block(1);
    return MCGP_OK;
}

// The scenario calls: race_scenario_kernel<false, rules> (state NULL: from the grid) or <true, rules> over simulations
// sim_offset + [0, n_sims) of every scenario, one thread block per scenario, and then the rule sets' counting kernels as
// the C ABI runs them, as grid_x x S (x 1 + n, paces_count with carried) blocks of one thread.  The plans are packed by
// plan_pack.h; of the three item tables those in `rules` (mcgp::kRule*) are checked and packed by penalty_pack.h,
// event_pack.h and pace_pack.h, and the kernel gets NULL for the others.  hist [S][n][n] is accumulated into; stage
// [S][n_sims][n] is written, and ev_stage [S][n_sims] and car_stage [S][n_sims][n] u16 where given (NULL: not staged).
// delta [S][n][2n - 1], fate [S][n][4], events_cnt [S][3][L + 1] (needs ev_stage) and carried [S][n][L + 1] (needs
// car_stage), each of which may be NULL, are accumulated into: delta by penalties_count where the call has penalties,
// else by the counting kernel of its one rule set; the centre bin and the columns 0 stay what they were, as on the device.
// The weather call (rules = kRuleWeather) hands its own inputs in `wx`: they are checked and packed by weather_pack.h into
// the condition bytes and the table, which the kernel reads through its event_laps and lap_sec arguments; car_stage
// gets the laps on the wrong tyres, and weather_count (grid_x x S x n blocks) adds them to `wrong` [S][n][L + 1].
// The grid call (rules = kRuleGrid, from the grid only) hands its own inputs in `gr`: they are checked and packed by
// grid_pack.h into the GridScenario table, which the kernel reads through its `pens` argument; car_stage gets the start
// slots, and grid_count (grid_x x S x n blocks) adds them to `start` [S][n][n] and `gain` [S][n][2n - 1].
// The priors call (rules = kRulePriors) hands its own inputs in `pr`: they are checked and packed by prior_pack.h into the
// PriorScenario table, which the kernel reads through its `pens` argument; bin_stage [S][n_sims][n] bytes gets the bins
// of the drawn offsets through `carried`, off_stage [S][n_sims][n] floats (NULL: not staged) the offsets through
// `ev_stage`, and priors_count (grid_x x S x (1 + n) blocks) adds to `delta` and to `draws` [S][n][n_edges + 1][n].
struct PriorArgs {
    const uint32_t *prior_count;
    const mcgp_pace_prior *priors;
    uint32_t n_edges;
    const double *edges;
    uint8_t *bin_stage;
    float *off_stage;
    unsigned long long *draws;
};

struct GridArgs {
    const uint32_t *edit_count;
    const mcgp_grid_edit *edits;
    unsigned long long *start, *gain;
};

struct WeatherArgs {
    const uint32_t *change_count;
    const mcgp_track_change *changes;
    const mcgp_weather_model *model;
    unsigned long long *wrong;
};

int scenario_run(uint32_t rules, const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                 const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                 const mcgp_pit_plan *plans, const uint32_t *penalty_count, const mcgp_time_penalty *penalties,
                 const uint32_t *event_count, const mcgp_lap_event *events, const uint32_t *pace_count,
                 const mcgp_pace_offset *paces, uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist,
                 uint8_t *stage, uint32_t *ev_stage, uint16_t *car_stage, unsigned long long *delta, unsigned long long *fate,
                 unsigned long long *events_cnt, unsigned long long *carried, uint32_t grid_x, const char **err,
                 const WeatherArgs *wx = nullptr, const GridArgs *gr = nullptr, const PriorArgs *pr = nullptr)
{
    const bool pen = rules & mcgp::kRulePenalties, ev = rules & mcgp::kRuleEvents, pace = rules & mcgp::kRulePaces;
    static mcgp::KParams kp;
    const int rc = params(cfg, drv, grid_probs, n, &kp, err);
    if (rc != MCGP_OK) return rc;
    if (n_scenarios < 1 || n_scenarios > mcgp::kMaxStrategyScenarios)
        return fail(MCGP_E_BAD_ARG, "n_scenarios must be in [1, 64]", err);
    if ((state != nullptr) == (grid_probs != nullptr)) return fail(MCGP_E_BAD_ARG, "either a state or grid_probs", err);
    // (the events call always stages the event word: its kernel does not test the pointer.  The check is new for
    // emu_events_run, whose old body had none)
    if ((events_cnt || rules == mcgp::kRuleEvents) && !ev_stage) return fail(MCGP_E_BAD_ARG, "events need ev_stage", err);
    if ((carried || (wx && wx->wrong)) && !car_stage) return fail(MCGP_E_BAD_ARG, "carried needs car_stage", err);
    if ((rules == mcgp::kRuleWeather) != (wx != nullptr)) return fail(MCGP_E_BAD_ARG, "weather needs its inputs", err);
    if ((rules == mcgp::kRuleGrid) != (gr != nullptr)) return fail(MCGP_E_BAD_ARG, "grid edits need their inputs", err);
    if ((rules == mcgp::kRulePriors) != (pr != nullptr)) return fail(MCGP_E_BAD_ARG, "priors need their inputs", err);
    if (pr && !pr->bin_stage) return fail(MCGP_E_BAD_ARG, "priors need bin_stage", err);
    if (gr && state) return fail(MCGP_E_BAD_ARG, "grid edits run from the grid only", err);
    if (gr && (gr->start || gr->gain) && !car_stage) return fail(MCGP_E_BAD_ARG, "start and gain need car_stage", err);
    const int L = cfg->total_laps;
    mcgp::ResumeState st;
    std::memset(&st, 0, sizeof(st));
    if (state) {
        const std::string e = mcgp::pack_race_state(*state, 0, n, L, &st);
        if (!e.empty()) return fail(MCGP_E_BAD_ARG, e, err);
        st.sim_offset = sim_offset;
    }
    const int first_lap = state ? st.lap + 1 : 2;
    const bool resumed = state != nullptr;
    std::vector<mcgp::StrategyScenario> scen;
    std::vector<mcgp::StopLap> stop_laps;
    std::vector<mcgp::PenaltyScenario> pens;
    std::vector<mcgp::PenaltyLap> pen_laps;
    std::vector<uint8_t> event_laps;
    std::vector<mcgp::PaceScenario> pscen;
    std::vector<mcgp::PaceLap> pace_laps;
    std::vector<double> lap_sec;
    std::vector<mcgp::GridScenario> grids;
    std::vector<mcgp::PriorScenario> priors;
    uint64_t n_pens = 0, n_events = 0, n_paces = 0, n_changes = 0, n_edits = 0, n_priors = 0;
    std::string e = mcgp::pack_scenarios(n_scenarios, plan_count, plans, n, L, first_lap, resumed, &scen, &stop_laps);
    if (e.empty() && pen) e = mcgp::check_penalty_counts(n_scenarios, penalty_count, &n_pens);
    if (e.empty() && ev) e = mcgp::check_event_counts(n_scenarios, event_count, &n_events);
    if (e.empty() && pace) e = mcgp::check_pace_counts(n_scenarios, pace_count, &n_paces);
    if (e.empty() && n_pens && !penalties) e = "penalties is NULL";
    if (e.empty() && n_events && !events) e = "events is NULL";
    if (e.empty() && n_paces && !paces) e = "paces is NULL";
    if (e.empty() && pen)
        e = mcgp::pack_penalties(n_scenarios, penalty_count, penalties, n, L, first_lap, resumed, &pens, &pen_laps);
    if (e.empty() && ev) e = mcgp::pack_events(n_scenarios, event_count, events, L, first_lap, resumed, &event_laps);
    if (e.empty() && pace)      // lap 1 reads the base pace too: from the grid an offset may name it
        e = mcgp::pack_paces(n_scenarios, pace_count, paces, n, L, state ? first_lap : 1, resumed, &pscen, &pace_laps, &lap_sec);
    if (e.empty() && wx && !wx->change_count) e = "change_count is NULL";
    if (e.empty() && wx) e = mcgp::check_change_counts(n_scenarios, wx->change_count, &n_changes);
    if (e.empty() && n_changes && !wx->changes) e = "changes is NULL";
    if (e.empty() && wx)
        e = mcgp::pack_weather(n_scenarios, wx->change_count, wx->changes, wx->model, cfg->track_condition, L, first_lap,
                               resumed, &event_laps, &lap_sec);
    if (e.empty() && gr && !gr->edit_count) e = "edit_count is NULL";
    if (e.empty() && gr) e = mcgp::check_edit_counts(n_scenarios, gr->edit_count, n, &n_edits);
    if (e.empty() && n_edits && !gr->edits) e = "edits is NULL";
    if (e.empty() && gr) e = mcgp::pack_grids(n_scenarios, gr->edit_count, gr->edits, n, &grids);
    if (e.empty() && pr && !pr->prior_count) e = "prior_count is NULL";
    if (e.empty() && pr) e = mcgp::check_prior_counts(n_scenarios, pr->prior_count, &n_priors);
    if (e.empty() && pr) e = mcgp::check_prior_edges(pr->n_edges, pr->edges);
    if (e.empty() && n_priors && !pr->priors) e = "priors is NULL";
    if (e.empty() && pr) e = mcgp::pack_priors(n_scenarios, pr->prior_count, pr->priors, n, pr->n_edges, pr->edges, &priors);
    if (!e.empty()) return fail(MCGP_E_BAD_ARG, e, err);
    const auto kernel = mcgp::scenario_kernel(rules, resumed);
    const mcgp::PenaltyScenario *pens_arg = pen  ? pens.data()
                                            : gr ? reinterpret_cast<const mcgp::PenaltyScenario *>(grids.data())
                                            : pr ? reinterpret_cast<const mcgp::PenaltyScenario *>(priors.data()) : nullptr;
    if (pr) {
        ev_stage = reinterpret_cast<uint32_t *>(pr->off_stage);
        car_stage = reinterpret_cast<uint16_t *>(pr->bin_stage);
    }
    one_thread_block(n_scenarios);
    for (uint32_t si = 0; si < n_scenarios; ++si) {
        blockIdx.y = si;
        kernel(&kp, &st, scen.data(), stop_laps.data(), pens_arg, pen ? pen_laps.data() : nullptr,
               ev || wx ? event_laps.data() : nullptr, pace ? pscen.data() : nullptr, pace ? pace_laps.data() : nullptr,
               pace || wx ? lap_sec.data() : nullptr, n_sims, sim_offset, (uint32_t)seed, (uint32_t)(seed >> 32), hist, stage,
               ev_stage, car_stage, (uint32_t)n_sims);
    }
    unsigned long long *ev_delta = pen ? nullptr : delta, *pace_delta = pen ? nullptr : delta;
    const uint32_t gz = carried ? 1u + n : 1u;
    for (uint32_t z = 0; rules != 0u && !pr && z < gz; ++z)  // (the strategies call has no counting kernel that runs here)
        for (uint32_t y = 0; y < n_scenarios; ++y)
            for (uint32_t x = 0; x < grid_x; ++x) {
                blockIdx = {x, y, z};
                if (z == 0) {
                    gridDim = {grid_x, n_scenarios, 1};
                    if (pen && (delta || fate)) mcgp::penalties_count(stage, n_sims, n, delta, fate);
                    if (ev && (ev_delta || events_cnt))
                        mcgp::events_count(stage, ev_stage, n_sims, n, (uint32_t)L, ev_delta, events_cnt);
                }
                gridDim = {grid_x, n_scenarios, gz};
                if (pace && (pace_delta || carried))
                    mcgp::paces_count(stage, car_stage, pscen.data(), n_sims, n, (uint32_t)L, pace_delta, carried);
            }
    if (wx && wx->wrong) {
        gridDim = {grid_x, n_scenarios, n};
        for (uint32_t z = 0; z < n; ++z)
            for (uint32_t y = 0; y < n_scenarios; ++y)
                for (uint32_t x = 0; x < grid_x; ++x) {
                    blockIdx = {x, y, z};
                    mcgp::weather_count(car_stage, n_sims, n, (uint32_t)L, wx->wrong);
                }
    }
    if (gr && (gr->start || gr->gain)) {
        gridDim = {grid_x, n_scenarios, n};
        for (uint32_t z = 0; z < n; ++z)
            for (uint32_t y = 0; y < n_scenarios; ++y)
                for (uint32_t x = 0; x < grid_x; ++x) {
                    blockIdx = {x, y, z};
                    mcgp::grid_count(stage, car_stage, n_sims, n, gr->start, gr->gain);
                }
    }
    if (pr && (delta || pr->draws)) {
        const uint32_t layers = pr->draws ? 1u + n : 1u;
        gridDim = {grid_x, n_scenarios, layers};
        for (uint32_t z = 0; z < layers; ++z)
            for (uint32_t y = 0; y < n_scenarios; ++y)
                for (uint32_t x = 0; x < grid_x; ++x) {
                    blockIdx = {x, y, z};
                    mcgp::priors_count(stage, pr->bin_stage, n_sims, n, pr->n_edges + 1u, delta, pr->draws);
                }
    }
    one_thread_block(1);
    return MCGP_OK;
}

}  // namespace

extern "C" {

// race_kernel: hist [n][n] is accumulated into; orders [n_sims][n] or NULL; fixed_grid [n] or NULL.
int emu_generic_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n, uint64_t n_sims,
                    uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *orders,
                    const uint8_t *fixed_grid, const char **err)
{
    static mcgp::KParams kp;
    const int rc = params(cfg, drv, grid_probs, n, &kp, err);
    if (rc != MCGP_OK) return rc;
    one_thread_block(1);
    mcgp::race_kernel(&kp, n_sims, sim_offset, (uint32_t)seed, (uint32_t)(seed >> 32), hist, orders, fixed_grid,
                      (uint32_t)n_sims, nullptr, nullptr);
    return MCGP_OK;
}

// race_resume_kernel: n_sims simulations of every state, ids sim_offsets[s] + [0, n_sims).  hist [states][n][n] is
// accumulated into; orders [states][n_sims][n] or NULL.
int emu_generic_resume(const mcgp_config *cfg, const mcgp_drivers *drv, uint32_t n, uint32_t n_states,
                       const mcgp_race_state *states, uint64_t n_sims, const uint64_t *sim_offsets, uint64_t seed,
                       unsigned long long *hist, uint8_t *orders, const char **err)
{
    static mcgp::KParams kp;
    const int rc = params(cfg, drv, nullptr, n, &kp, err);
    if (rc != MCGP_OK) return rc;
    std::vector<mcgp::ResumeState> st(n_states);
    for (uint32_t si = 0; si < n_states; ++si) {
        const std::string e = mcgp::pack_race_state(states[si], si, n, cfg->total_laps, &st[si]);
        if (!e.empty()) return fail(MCGP_E_BAD_ARG, e, err);
        st[si].sim_offset = sim_offsets ? sim_offsets[si] : 0;
    }
    one_thread_block(n_states);
    for (uint32_t si = 0; si < n_states; ++si) {
        blockIdx.y = si;
        mcgp::race_resume_kernel(&kp, st.data(), n_sims, 0, (uint32_t)seed, (uint32_t)(seed >> 32), hist, orders,
                                 (uint32_t)n_sims);
    }
    blockIdx.y = 0;
    return MCGP_OK;
}

// race_trace_kernel: hist [n][n] is accumulated into; stage [L n][stride] (stride >= n_sims) and rec [n_sims] are
// written, in the layout documented at the top of csrc/trace.hip.h.
int emu_generic_trace(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n, uint64_t n_sims,
                      uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage, uint64_t stride,
                      uint64_t *rec, const char **err)
{
    static mcgp::KParams kp;
    mcgp::ResumeState st;
    const int rc = analysis_setup(cfg, drv, grid_probs, nullptr, n, n_sims, stride, false, nullptr, &kp, &st, err);
    if (rc != MCGP_OK) return rc;
    mcgp::race_trace_kernel(&kp, n_sims, sim_offset, (uint32_t)seed, (uint32_t)(seed >> 32), hist, stage, stride, rec,
                            (uint32_t)n_sims);
    return MCGP_OK;
}

// race_gaps_kernel<false> (state NULL: from the grid) or <true>: simulations sim_offset + [0, n_sims).  hist [n][n] is
// accumulated into; stage [(L - first_lap + 1) (n + 1 + n_pairs)][stride] (stride >= n_sims) is written.
int emu_gaps_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                 uint32_t n, uint32_t n_edges, const double *edges, uint32_t n_pairs, const uint8_t *pairs, uint64_t n_sims,
                 uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage, uint64_t stride,
                 const char **err)
{
    static mcgp::KParams kp;
    mcgp::ResumeState st;
    const bool bad = n_edges < 1 || n_edges > mcgp::kMaxGapEdges || n_pairs > mcgp::kMaxGapPairs;
    const int rc = analysis_setup(cfg, drv, grid_probs, state, n, n_sims, stride, false,
                                  bad ? "n_edges in [1, 63], n_pairs in [0, 64]" : nullptr, &kp, &st, err);
    if (rc != MCGP_OK) return rc;
    double table[mcgp::kGapEdgeSlots];                      // the call's edges, then +inf, as the C ABI uploads them
    for (uint32_t i = 0; i < mcgp::kGapEdgeSlots; ++i) table[i] = i < n_edges ? edges[i] : HUGE_VAL;
    const auto kernel = state ? &mcgp::race_gaps_kernel<true> : &mcgp::race_gaps_kernel<false>;
    kernel(&kp, &st, table, n_edges, pairs, n_pairs, n_sims, sim_offset, (uint32_t)seed, (uint32_t)(seed >> 32), hist, stage,
           stride, (uint32_t)n_sims);
    return MCGP_OK;
}

// race_window_kernel<false> (state NULL: from the grid) or <true>: simulations sim_offset + [0, n_sims).  hist [n][n] is
// accumulated into; stage [(L - first_lap + 1) 5 n_windows][stride] (stride >= n_sims) is written.
int emu_window_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                   uint32_t n, uint32_t n_edges, const double *edges, uint32_t n_windows, const uint8_t *window_drivers,
                   const double *window_losses, uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist,
                   uint8_t *stage, uint64_t stride, const char **err)
{
    static mcgp::KParams kp;
    mcgp::ResumeState st;
    bool bad = n_edges < 1 || n_edges > mcgp::kMaxGapEdges || n_windows < 1 || n_windows > mcgp::kMaxPitWindows;
    for (uint32_t w = 0; !bad && w < n_windows; ++w)
        bad = window_drivers[w] >= n || !std::isfinite(window_losses[w]) || !(window_losses[w] >= 0.0);
    const int rc = analysis_setup(cfg, drv, grid_probs, state, n, n_sims, stride, false,
                                  bad ? "n_edges in [1, 63], n_windows in [1, 64], drivers below n, losses finite and >= 0"
                                      : nullptr, &kp, &st, err);
    if (rc != MCGP_OK) return rc;
    double table[mcgp::kGapEdgeSlots];                      // the tables padded as the C ABI uploads them
    for (uint32_t i = 0; i < mcgp::kGapEdgeSlots; ++i) table[i] = i < n_edges ? edges[i] : HUGE_VAL;
    uint8_t drivers[mcgp::kWindowSlots] = {};
    double losses[mcgp::kWindowSlots] = {};
    for (uint32_t w = 0; w < n_windows; ++w) drivers[w] = window_drivers[w], losses[w] = window_losses[w];
    const auto kernel = state ? &mcgp::race_window_kernel<true> : &mcgp::race_window_kernel<false>;
    kernel(&kp, &st, table, n_edges, drivers, losses, n_windows, n_sims, sim_offset, (uint32_t)seed, (uint32_t)(seed >> 32),
           hist, stage, stride, (uint32_t)n_sims);
    return MCGP_OK;
}

// race_conditions_kernel<false> (state NULL: from the grid) or <true>: simulations sim_offset + [0, n_sims).  hist [n][n]
// is accumulated into; stage ([n][stride] bytes, then [stride] u64 masks; stride >= n_sims, a multiple of 8) is written.
// count [C] and cond_hist [C][n][n] (or NULL) are accumulated into by conditions_count, run as grid_x x ceil(C / 8) blocks
// of one thread (count NULL: not run).
int emu_conditions_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                       const mcgp_race_state *state, uint32_t n, uint32_t n_conditions, const mcgp_condition *conditions,
                       uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage,
                       uint64_t stride, unsigned long long *count, unsigned long long *cond_hist, uint32_t grid_x,
                       const char **err)
{
    static_assert(sizeof(mcgp::Cond) == sizeof(mcgp_condition), "the table is the C ABI's array");
    static mcgp::KParams kp;
    mcgp::ResumeState st;
    const bool bad = n_conditions < 1 || n_conditions > mcgp::kMaxConditions;
    const int rc = analysis_setup(cfg, drv, grid_probs, state, n, n_sims, stride, true, bad ? "n_conditions in [1, 64]" : nullptr,
                                  &kp, &st, err);
    if (rc != MCGP_OK) return rc;
    const auto kernel = state ? &mcgp::race_conditions_kernel<true> : &mcgp::race_conditions_kernel<false>;
    kernel(&kp, &st, reinterpret_cast<const mcgp::Cond *>(conditions), n_conditions, n_sims, sim_offset, (uint32_t)seed,
           (uint32_t)(seed >> 32), hist, stage, stride, (uint32_t)n_sims);
    if (count) {
        const uint32_t groups = (n_conditions + mcgp::kCondGroup - 1) / mcgp::kCondGroup;
        gridDim = {grid_x, groups, 1};
        for (uint32_t y = 0; y < groups; ++y)
            for (uint32_t x = 0; x < grid_x; ++x) {
                blockIdx = {x, y, 0};
                mcgp::conditions_count(stage, stride, n_sims, n, n_conditions, count, cond_hist);
            }
        one_thread_block(1);
    }
    return MCGP_OK;
}

// race_stints_kernel<false> (state NULL: from the grid) or <true>: simulations sim_offset + [0, n_sims).  hist [n][n] is
// accumulated into; rec [n][stride] u64 and pos [n][stride] bytes (stride >= n_sims) are written, in the layout
// documented at the top of csrc/stints.hip.h.
int emu_stints_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                   uint32_t n, uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint64_t *rec,
                   uint8_t *pos, uint64_t stride, const char **err)
{
    static mcgp::KParams kp;
    mcgp::ResumeState st;
    const int rc = analysis_setup(cfg, drv, grid_probs, state, n, n_sims, stride, false, nullptr, &kp, &st, err);
    if (rc != MCGP_OK) return rc;
    const auto kernel = state ? &mcgp::race_stints_kernel<true> : &mcgp::race_stints_kernel<false>;
    kernel(&kp, &st, n_sims, sim_offset, (uint32_t)seed, (uint32_t)(seed >> 32), hist, rec, pos, stride, (uint32_t)n_sims);
    return MCGP_OK;
}

// race_moves_kernel<false> (state NULL: from the grid) or <true>: simulations sim_offset + [0, n_sims).  hist [n][n] is
// accumulated into; stage [(L + 2) n][stride] bytes (stride >= n_sims) is written, in the layout documented at the top
// of csrc/moves.hip.h.
int emu_moves_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                  uint32_t n, uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage,
                  uint64_t stride, const char **err)
{
    static mcgp::KParams kp;
    mcgp::ResumeState st;
    const int rc = analysis_setup(cfg, drv, grid_probs, state, n, n_sims, stride, false, nullptr, &kp, &st, err);
    if (rc != MCGP_OK) return rc;
    const auto kernel = state ? &mcgp::race_moves_kernel<true> : &mcgp::race_moves_kernel<false>;
    kernel(&kp, &st, n_sims, sim_offset, (uint32_t)seed, (uint32_t)(seed >> 32), hist, stage, stride, (uint32_t)n_sims);
    return MCGP_OK;
}

// race_fastest_kernel: simulations sim_offset + [0, n_sims).  hist [n][n] is accumulated into; orders [n_sims][n],
// fl_driver [n_sims] and fl_pos [n_sims] are written, in the layout documented at the top of csrc/fastest.hip.h.
int emu_fastest_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n, uint64_t n_sims,
                    uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *orders, uint8_t *fl_driver,
                    uint8_t *fl_pos, const char **err)
{
    static mcgp::KParams kp;
    const int rc = params(cfg, drv, grid_probs, n, &kp, err);
    if (rc != MCGP_OK) return rc;
    if (!grid_probs || !orders || !fl_driver || !fl_pos) return fail(MCGP_E_BAD_ARG, "grid_probs / an output is NULL", err);
    one_thread_block(1);
    mcgp::race_fastest_kernel(&kp, n_sims, sim_offset, (uint32_t)seed, (uint32_t)(seed >> 32), hist, orders, fl_driver, fl_pos,
                              (uint32_t)n_sims);
    return MCGP_OK;
}

// The seven scenario calls (scenario_run above).  stage [S][n_sims][n] holds each driver's classified position, with
// penalties | fate << 5; ev_stage the packed event counts (red | sc << 10 | vsc << 20); car_stage the laps carried at the
// drivers with an UNTIL_STOP offset (emu_weather_run: every driver's laps on the wrong tyres, or NULL: not staged).
// emu_combined_run takes a NULL count array as none in any scenario.  emu_grid_run: car_stage gets every driver's start
// slot after the edits (NULL: not staged).
int emu_generic_strategy(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                         const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                         const mcgp_pit_plan *plans, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                         unsigned long long *hist, uint8_t *positions, const char **err)
{
    return scenario_run(0u, cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, n_sims, sim_offset, seed, hist, positions, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, 1, err);
}

int emu_penalties_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                      uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                      const uint32_t *penalty_count, const mcgp_time_penalty *penalties, uint64_t n_sims, uint64_t sim_offset,
                      uint64_t seed, unsigned long long *hist, uint8_t *stage, unsigned long long *delta,
                      unsigned long long *fate, uint32_t grid_x, const char **err)
{
    return scenario_run(mcgp::kRulePenalties, cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, penalty_count,
                        penalties, nullptr, nullptr, nullptr, nullptr, n_sims, sim_offset, seed, hist, stage, nullptr, nullptr,
                        delta, fate, nullptr, nullptr, grid_x, err);
}

int emu_events_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                   uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                   const uint32_t *event_count, const mcgp_lap_event *events, uint64_t n_sims, uint64_t sim_offset,
                   uint64_t seed, unsigned long long *hist, uint8_t *stage, uint32_t *ev_stage, unsigned long long *delta,
                   unsigned long long *events_cnt, uint32_t grid_x, const char **err)
{
    return scenario_run(mcgp::kRuleEvents, cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, nullptr, nullptr,
                        event_count, events, nullptr, nullptr, n_sims, sim_offset, seed, hist, stage, ev_stage, nullptr, delta,
                        nullptr, events_cnt, nullptr, grid_x, err);
}

int emu_paces_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                  uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                  const uint32_t *pace_count, const mcgp_pace_offset *paces, uint64_t n_sims, uint64_t sim_offset,
                  uint64_t seed, unsigned long long *hist, uint8_t *stage, uint16_t *car_stage, unsigned long long *delta,
                  unsigned long long *carried, uint32_t grid_x, const char **err)
{
    return scenario_run(mcgp::kRulePaces, cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, nullptr, nullptr,
                        nullptr, nullptr, pace_count, paces, n_sims, sim_offset, seed, hist, stage, nullptr, car_stage, delta,
                        nullptr, nullptr, carried, grid_x, err);
}

int emu_combined_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                     uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                     const uint32_t *penalty_count, const mcgp_time_penalty *penalties, const uint32_t *event_count,
                     const mcgp_lap_event *events, const uint32_t *pace_count, const mcgp_pace_offset *paces, uint64_t n_sims,
                     uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage, uint32_t *ev_stage,
                     uint16_t *car_stage, unsigned long long *delta, unsigned long long *fate, unsigned long long *events_cnt,
                     unsigned long long *carried, uint32_t grid_x, const char **err)
{
    static const uint32_t none[mcgp::kMaxStrategyScenarios] = {};
    return scenario_run(mcgp::kRuleAll, cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans,
                        penalty_count ? penalty_count : none, penalties, event_count ? event_count : none, events,
                        pace_count ? pace_count : none, paces, n_sims, sim_offset, seed, hist, stage, ev_stage, car_stage, delta,
                        fate, events_cnt, carried, grid_x, err);
}

int emu_weather_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                    uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                    const uint32_t *change_count, const mcgp_track_change *changes, const mcgp_weather_model *model,
                    uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage,
                    uint16_t *car_stage, unsigned long long *wrong, uint32_t grid_x, const char **err)
{
    const WeatherArgs wx = {change_count, changes, model, wrong};
    return scenario_run(mcgp::kRuleWeather, cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, nullptr, nullptr,
                        nullptr, nullptr, nullptr, nullptr, n_sims, sim_offset, seed, hist, stage, nullptr, car_stage, nullptr,
                        nullptr, nullptr, nullptr, grid_x, err, &wx);
}

int emu_grid_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n, uint32_t n_scenarios,
                 const uint32_t *plan_count, const mcgp_pit_plan *plans, const uint32_t *edit_count,
                 const mcgp_grid_edit *edits, uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist,
                 uint8_t *stage, uint16_t *car_stage, unsigned long long *start, unsigned long long *gain, uint32_t grid_x,
                 const char **err)
{
    const GridArgs gr = {edit_count, edits, start, gain};
    return scenario_run(mcgp::kRuleGrid, cfg, drv, grid_probs, nullptr, n, n_scenarios, plan_count, plans, nullptr, nullptr,
                        nullptr, nullptr, nullptr, nullptr, n_sims, sim_offset, seed, hist, stage, nullptr, car_stage, nullptr,
                        nullptr, nullptr, nullptr, grid_x, err, nullptr, &gr);
}

// stage [S][n_sims][n] positions, bin_stage [S][n_sims][n] the bins of the drawn offsets, off_stage [S][n_sims][n] the
// offsets (NULL: not staged); delta [S][n][2n - 1] and draws [S][n][n_edges + 1][n] (either may be NULL) are accumulated
// into by priors_count.
int emu_priors_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                   uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                   const uint32_t *prior_count, const mcgp_pace_prior *priors, uint32_t n_edges, const double *edges,
                   uint64_t n_sims, uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage,
                   uint8_t *bin_stage, float *off_stage, unsigned long long *delta, unsigned long long *draws, uint32_t grid_x,
                   const char **err)
{
    const PriorArgs pr = {prior_count, priors, n_edges, edges, bin_stage, off_stage, draws};
    return scenario_run(mcgp::kRulePriors, cfg, drv, grid_probs, state, n, n_scenarios, plan_count, plans, nullptr, nullptr,
                        nullptr, nullptr, nullptr, nullptr, n_sims, sim_offset, seed, hist, stage, nullptr, nullptr, delta,
                        nullptr, nullptr, nullptr, grid_x, err, nullptr, nullptr, &pr);
}

}  // extern "C"
