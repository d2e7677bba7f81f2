// emu_gaps.cpp -- DEBUGGING build of csrc/gaps.hip.h for the host (not product code, not a fallback: nothing in
// monte_carlo_gp_amd/ can reach it).  Compiles the header with g++ through the stand-in <hip/hip_runtime.h> of this
// directory and calls the real __global__ functions race_gaps_kernel<false / true>, in the manner of emu_generic.cpp:
// blockDim = gridDim = 1 and n_batches = n_sims make the kernel an ordinary host function that walks the simulations
// one after another.  The state goes through csrc/plan_pack.h, the text the C ABI itself uses.
//
// Not run here: gaps_count_rows (__shfl_down, a fixed block of 256 threads).  The tests derive the counts from the
// staging bytes in numpy by the layout documented at the top of gaps.hip.h; the counting kernel is compared on the
// device.  tests/test_gaps_host_build.py.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../monte_carlo_gp_amd/csrc/params_build.h"
#include "../../monte_carlo_gp_amd/csrc/gaps.hip.h"
#include "../../monte_carlo_gp_amd/csrc/plan_pack.h"

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

}  // namespace

extern "C" {

// race_gaps_kernel<false> (state NULL: from the grid) or <true>: simulations sim_offset + [0, n_sims).  hist [n][n] is
// accumulated into; stage [(L - first_lap + 1) (n + 1 + n_pairs)][stride] (stride >= n_sims) is written.
int emu_gaps_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, const mcgp_race_state *state,
                 uint32_t n, uint32_t n_edges, const double *edges, uint32_t n_pairs, const uint8_t *pairs, uint64_t n_sims,
                 uint64_t sim_offset, uint64_t seed, unsigned long long *hist, uint8_t *stage, uint64_t stride,
                 const char **err)
{
    static const char *none = "";
    static mcgp::KParams kp;
    *err = none;
    const char *e = "";
    const int rc = mcgp::build_params(cfg, drv, grid_probs, n, &kp, &e);
    if (rc != MCGP_OK) return fail(rc, e, err);
    if (kp.wide) return fail(MCGP_E_BAD_ARG, "the generic kernels run MCGP_DEVIATES_32", err);
    if ((state != nullptr) == (grid_probs != nullptr)) return fail(MCGP_E_BAD_ARG, "either a state or grid_probs", err);
    if (n_edges < 1 || n_edges > mcgp::kMaxGapEdges || n_pairs > mcgp::kMaxGapPairs)
        return fail(MCGP_E_BAD_ARG, "n_edges in [1, 63], n_pairs in [0, 64]", err);
    if (stride < n_sims) return fail(MCGP_E_BAD_ARG, "stride must be at least n_sims", err);
    mcgp::ResumeState st;
    std::memset(&st, 0, sizeof(st));
    if (state) {
        const std::string es = mcgp::pack_race_state(*state, 0, n, cfg->total_laps, &st);
        if (!es.empty()) return fail(MCGP_E_BAD_ARG, es, err);
    }
    double table[mcgp::kGapEdgeSlots];                      // the call's edges, then +inf, as the C ABI uploads them
    for (uint32_t i = 0; i < mcgp::kGapEdgeSlots; ++i) table[i] = i < n_edges ? edges[i] : HUGE_VAL;
    edges = table;
    threadIdx = {0, 0, 0};
    blockIdx = {0, 0, 0};
    blockDim = {1, 1, 1};
    gridDim = {1, 1, 1};
    if (state)
        mcgp::race_gaps_kernel<true>(&kp, &st, edges, n_edges, pairs, n_pairs, n_sims, sim_offset, (uint32_t)seed,
                                     (uint32_t)(seed >> 32), hist, stage, stride, (uint32_t)n_sims);
    else
        mcgp::race_gaps_kernel<false>(&kp, &st, edges, n_edges, pairs, n_pairs, n_sims, sim_offset, (uint32_t)seed,
                                      (uint32_t)(seed >> 32), hist, stage, stride, (uint32_t)n_sims);
    return MCGP_OK;
}

}  // extern "C"
