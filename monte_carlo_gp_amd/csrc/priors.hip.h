// priors.hip.h -- race odds under per-simulation pace draws (mcgp_run_priors, include/mcgp.h).
//
// The table, the draw and the policy of the priors rule set of race_scenario_kernel (scenario.hip.h: S scenarios of one
// race with common random numbers, one lane per (scenario, simulation), blockIdx.y the scenario), and priors_count.
//
//   draw    before the start the lane draws an offset x_d (binary32 seconds a lap) for every driver: an own deviate z_d
//           for a driver with a DRIVER item (counter {sim, 0, kPurposePrior | d >> 2}, word d & 3) and one deviate z_g per
//           group, keyed by the group's lowest member g (counter {sim, 0, kPurposePrior | 8 + (g >> 2)}, word g & 3), both
//           through the binary32 inverse-normal table of the block's LDS.  t = sigma_own[d] * (double)z_d (+0.0 for a
//           driver without a DRIVER item); t = t + sigma_g * (double)z_g for a member of a group; x_d = (float)t.  A
//           deviate depends on (seed, simulation, driver index) alone: the same in every scenario, from the grid and from
//           a state, so that scenarios that differ in their sigmas are compared under common random numbers;
//   pace    PriorPace, the pace policy of start_from_grid (lap 1) and run_laps: wherever the model reads base_pace[d] the
//           car's base is b = base_pace[d] + (double)x_d, one binary64 addition.
//
// Which Philox blocks are drawn is wave-uniform: a block serves one scenario, and PriorScenario holds the masks.  The
// group deviates go first, each into the offset row of its lowest member; the drivers are then finished from the last
// to the first, so that every member reads its group's deviate before the lowest member's own offset replaces it.
// The per-lane state is the n binary32 offsets, in the block's dynamic LDS behind the lane's rows (stride blockDim.x,
// bank-conflict free like the other rows): 4n bytes a lane, which the host counts for this call only
// (prior_lane_lds_bytes).  A scenario without items draws nothing and its base() is one wave-uniform test.
//
// Staging per scenario, simulation and driver: the strategy call's position byte, one more byte with the bin of x_d
// among the call's edges (the number of edges e with e <= (double)x_d, an IEEE compare), written before the race, and the
// binary32 offset itself when offsets_out is wanted.  priors_count reads the bytes once, blockIdx.y the scenario:
// blockIdx.z = 0 counts pos_s(d) - pos_0(d) for scenarios s >= 1 (count_position_deltas, strategy.hip.h: the centre bin
// left out); blockIdx.z = 1 + d counts driver d's [bin][position] into [16][32] u32 LDS bins (2 KB).  One u64 global atomic
// per non-zero bin.  It has no cross-lane operation and strides by its block's size.
// Overflow: a launch is at most max_sims_per_launch() < 2^32 simulations per scenario, so no u32 bin can wrap.
#pragma once
#include "strategy.hip.h"

namespace mcgp {

constexpr uint32_t kPriorGroupBlock = 8u;                   // the group deviates' first block
constexpr uint32_t kMaxScenarioPriors = 64;
constexpr int kPriorDriver = 0, kPriorGroup = 1;            // MCGP_PRIOR_* of include/mcgp.h
constexpr double kMaxPriorSigma = 10.0;
constexpr uint32_t kMaxPriorEdges = 15;
constexpr uint32_t kPriorBins = kMaxPriorEdges + 1;
constexpr int kPriorsCountBlock = 256;                      // threads of a counting block
constexpr uint32_t kPriorDeltaBins = kMaxCars * (2 * kMaxCars - 1);
static_assert(kPriorBins * kMaxCars <= kPriorDeltaBins, "a driver's [bin][position] bins fit the block's delta bins");

// LDS bytes a lane of the priors instantiation has behind per_thread_lds_bytes(n): its offsets
__host__ __device__ constexpr size_t prior_lane_lds_bytes(int n) { return (size_t)n * 4; }

// One scenario's items in device memory, and the call's edges (the same in every scenario).
struct PriorScenario {
    uint32_t items;                     // their number; 0: the race as forecast, nothing is drawn
    uint32_t own;                       // bit d: driver d has a DRIVER item
    uint32_t grouped;                   // bit d: driver d is a member of a group
    uint32_t lows;                      // bit g: driver g is the lowest member of a group
    uint32_t n_edges;
    uint32_t pad;
    uint8_t low_of[kMaxCars];           // a member's group: its lowest member
    double sigma_own[kMaxCars];
    double sigma_grp[kMaxCars];         // a member's group's sigma
    double edges[kMaxPriorEdges + 1];
};

// The pace policy under drawn offsets (ModelPace, race_kernel.hip.h, is the model's).
struct PriorPace {
    const float *x;                     // the lane's offsets: x[d * B]
    int B;
    uint32_t items;                     // PriorScenario::items

    __device__ __forceinline__ void begin_lap(int /*lap*/) {}
    __device__ __forceinline__ double base(uint32_t d, double b) const
    {
        if (!items) return b;           // wave-uniform: the scenario has no item
        return b + (double)x[d * (uint32_t)B];
    }
};

// The lane's offsets of one simulation into x[d * B], d < n, and each one's bin into bins[d]; into offs[d] too unless NULL.
__device__ __forceinline__ void draw_priors(const PriorScenario *__restrict__ p, int n, const float4 *__restrict__ norm,
                                            uint32_t c0, uint32_t c1, uint32_t seed_lo, uint32_t seed_hi, float *x, int B,
                                            uint8_t *__restrict__ bins, float *__restrict__ offs)
{
    const uint32_t own = p->own, grouped = p->grouped, lows = p->lows, n_edges = p->n_edges;
    const int n_blocks = (n + 3) >> 2;
    if (p->items) {
        for (int j = 0; j < n_blocks; ++j) {
            const uint32_t in_block = (lows >> (4 * j)) & 15u;
            if (!in_block) continue;    // wave-uniform
            uint32_t w[4];
            philox4x32_10(c0, c1, 0u, kPurposePrior | (kPriorGroupBlock + (uint32_t)j), seed_lo, seed_hi, w[0], w[1], w[2], w[3]);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((in_block >> k) & 1u) x[(4 * j + k) * B] = normal_from_u32(w[k], norm);
        }
    }
    for (int j = n_blocks - 1; j >= 0; --j) {
        const uint32_t in_block = (own >> (4 * j)) & 15u;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (in_block)                   // wave-uniform
            philox4x32_10(c0, c1, 0u, kPurposePrior | (uint32_t)j, seed_lo, seed_hi, w[0], w[1], w[2], w[3]);
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            const int d = 4 * j + k;
            if (d >= n) continue;
            double t = 0.0;
            if ((in_block >> k) & 1u) t = p->sigma_own[d] * (double)normal_from_u32(w[k], norm);
            if ((grouped >> d) & 1u) t = t + p->sigma_grp[d] * (double)x[(int)p->low_of[d] * B];
            const float xd = (float)t;
            x[d * B] = xd;
            uint32_t bin = 0u;
            for (uint32_t e = 0; e < n_edges; ++e) bin += p->edges[e] <= (double)xd;
            bins[d] = (uint8_t)bin;
            if (offs) offs[d] = xd;
        }
    }
}

// From the staged bytes of m simulations, for scenario s = blockIdx.y: a block with blockIdx.z = 0 adds the paired changes
// of position against scenario 0 to delta [S][n][2n - 1] (s >= 1, the centre left out; delta may be NULL); a block with
// blockIdx.z = 1 + d adds driver d's (bin, position) to draws_out [S][n][n_bins][n] (may be NULL, and gridDim.z 1 then).
// u32 LDS bins per block, one u64 global atomic per non-zero bin; any block size.
__global__ void __launch_bounds__(kPriorsCountBlock)
priors_count(const uint8_t *__restrict__ stage, const uint8_t *__restrict__ bin_stage, uint64_t m, uint32_t n, uint32_t n_bins,
             unsigned long long *__restrict__ delta, unsigned long long *__restrict__ draws_out)
{
    __shared__ uint32_t bins[kPriorDeltaBins];
    const uint32_t t = threadIdx.x, nt = blockDim.x, s = blockIdx.y, w = 2u * n - 1u;
    const bool deltas = blockIdx.z == 0u;
    const uint32_t d = deltas ? 0u : blockIdx.z - 1u;
    if (deltas ? (delta == nullptr || s == 0u) : (draws_out == nullptr || d >= n)) return;
    const uint32_t cells = deltas ? n * w : n_bins * n;
    for (uint32_t i = t; i < cells; i += nt) bins[i] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)s * m * n;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt) {
        if (deltas) {
            count_position_deltas(stage + i * n, stage + base + i * n, n, 0xFFu, bins);
        } else {
            const uint32_t b = bin_stage[base + i * n + d], pos = stage[base + i * n + d];
            if (b < n_bins && pos < n) atomicAdd(&bins[b * n + pos], 1u);       // (always: the race kernel wrote both)
        }
    }
    __syncthreads();
    flush_bins(bins, cells, deltas ? delta + (uint64_t)s * cells : draws_out + ((uint64_t)s * n + d) * cells, t, nt);
}

}  // namespace mcgp
