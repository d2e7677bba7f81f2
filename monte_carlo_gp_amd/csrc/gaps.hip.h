// gaps.hip.h -- the time gaps of a race, counted on the device (mcgp_run_gaps, include/mcgp.h).
//
// race_gaps_kernel runs mcgp_run's simulations (from the grid, kFromState false) or mcgp_run_from_state's (from one
// state) with the generic kernel's code -- run_observed (resume.hip.h), the analysis kernels' shared lane body -- and
// a per-lap observer (GapObserver) that sees the rows after update_positions of every recorded lap: laps 1..L from the
// grid, laps k + 1 .. L from a state after lap k.  Simulation i draws exactly what those calls' simulation i draws, so
// the position histogram is theirs.  Read at that point of a lap (the state the CPU oracle's per-lap trace records):
//
//   running order     the cars not retired, in `ord` order (cumulative time, grid slot), as race_trace_kernel reads it;
//   gap to the leader Cum(d) - Cum(leader) of a running car d: one binary64 subtraction, >= 0, 0 for the leader;
//   lead              Cum(second) - Cum(leader), the same subtraction the second car's own gap is;
//   pair (a, b)       both running: Cum(b) - Cum(a) if a is ahead of b in the running order, else Cum(a) - Cum(b).
//                     "Ahead" is decided by the order's own key, (cumulative time, grid slot), on the two cars; `ord`
//                     is sorted by that key when the observer runs (run_laps sorts before update_positions).
//
// Bins: B = n_edges + 1; bin(x) = the number of edges <= x.  The edges are wave-uniform and read with scalar loads from
// device memory (a const __restrict__ kernel argument at a uniform index), eight at a time from a table padded with +inf
// to 64 entries; the search is the branch-free count itself, one compare and one add per edge, not a six-step
// bisection: a bisection's index differs from lane to lane, so its reads would be LDS or vector-memory gathers, six
// dependent ones per value, and the block's LDS is the rows' (it decides how many waves a CU holds), while at the 14
// default edges the count is two scalar loads and 32 VALU instructions on SGPR operands.
//
// Staging: one byte per (recorded lap, row, simulation), [(lap - first_lap) R + row][simulation], R = n + 1 + n_pairs,
// with a row stride of `stride` bytes so that a wave's lanes (adjacent simulations) write adjacent bytes of a row:
//   row d < n          bin of driver d's gap to the leader, or B = retired
//   row n              bin of the lead, or B = fewer than two cars running
//   row n + 1 + p      pair p = (a, b): bin(b - a) if a is ahead, B + bin(a - b) if b is ahead, 2B if either has retired
// Values fit a byte: 2B <= 128.  The host sizes a chunk of simulations to a fixed staging budget (mcgp_hip.hip:
// kGapsStageBytes / (recorded laps x R)), launches the race kernel on it, then gaps_count_rows: a block per staged row,
// every thread counting its words of the row into its own column of u32 bins in dynamic LDS ([value][thread]: no
// atomics, no bank conflicts; 4 x 256 x values bytes, 16 KiB at the default 16 values, 129 KiB at the most, 129), then
// a reduction per bin and one u64 global atomic per non-zero bin into the row's place in lap_gap / lead / pair.
//
// Overflow: a chunk is at most max_sims_per_launch() < 2^32 simulations and a thread's bin receives at most one count
// per simulation of one row, so no u32 counter can wrap.
#pragma once
#include "resume.hip.h"

namespace mcgp {

constexpr uint32_t kMaxGapEdges = 63;
constexpr uint32_t kMaxGapPairs = 64;
constexpr uint32_t kGapEdgeGroup = 8;            // edges per scalar load
constexpr uint32_t kGapEdgeSlots = 64;           // the device's edge table: kMaxGapEdges rounded up to whole groups
constexpr int kGapsCountBlock = 256;             // threads of a counting block

// bin(x): the number of edges <= x (edges strictly increasing).  `edges` is the device's table of kGapEdgeSlots
// doubles: the call's n_edges, then +inf (never <= a finite x), so that the count goes in whole groups of kGapEdgeGroup:
// one scalar load of eight edges, then eight compares on SGPR operands, instead of a load and a wait per edge.
__device__ __forceinline__ uint32_t gap_bin(const double *__restrict__ edges, uint32_t n_edges, double x)
{
    uint32_t b = 0u;
    for (uint32_t g = 0; g < n_edges; g += kGapEdgeGroup) {
        double e[kGapEdgeGroup];
#pragma unroll
        for (uint32_t i = 0; i < kGapEdgeGroup; ++i) e[i] = edges[g + i];
#pragma unroll
        for (uint32_t i = 0; i < kGapEdgeGroup; ++i) b += e[i] <= x ? 1u : 0u;
    }
    return b;
}

// The gaps kernel's per-lap observer: one lane's race.
struct GapObserver {
    uint8_t *lane;                          // this lane's byte of the first recorded lap's row 0 (stage + local)
    uint64_t lap_bytes;                     // bytes from one lap's rows to the next: R x stride
    uint64_t stride;                        // bytes from one row to the next
    const double *__restrict__ edges;
    const uint8_t *__restrict__ pairs;      // [n_pairs][2]
    uint32_t n_edges, n_pairs;
    int n, first_lap;

    __device__ __forceinline__ void operator()(const Rows &s, int lap, int /*event*/)
    {
        uint8_t *row = lane + (uint64_t)(lap - first_lap) * lap_bytes;
        const uint32_t B = n_edges + 1u;
        uint32_t r = 0u, lead = B;
        double leader = 0.0;
        for (int i = 0; i < n; ++i) {
            const uint32_t d = s.Ord(i);
            uint32_t b = B;
            if (!(s.Pk(d) & kDnf)) {
                const double t = s.Cum(d);
                if (r == 0u) leader = t;
                b = gap_bin(edges, n_edges, t - leader);
                if (r == 1u) lead = b;
                ++r;
            }
            row[(uint64_t)d * stride] = (uint8_t)b;
        }
        row[(uint64_t)n * stride] = (uint8_t)lead;
        for (uint32_t p = 0; p < n_pairs; ++p) {
            const uint32_t a = pairs[2u * p], c = pairs[2u * p + 1u];
            const uint32_t pka = s.Pk(a), pkc = s.Pk(c);
            uint32_t v = 2u * B;
            if (!((pka | pkc) & kDnf)) {
                const double ta = s.Cum(a), tc = s.Cum(c);
                const bool a_ahead = ta < tc || (ta == tc && gpos_of(pka) < gpos_of(pkc));
                v = a_ahead ? gap_bin(edges, n_edges, tc - ta) : B + gap_bin(edges, n_edges, ta - tc);
            }
            row[(uint64_t)(n + 1 + (int)p) * stride] = (uint8_t)v;
        }
    }
};

// Simulations sim_offset + [0, m) (m <= the chunk the staging holds) from the grid (kFromState false) or from `state`,
// with race_kernel's block shape and LDS.  hist [n][n] is ACCUMULATED into; stage [(L - first_lap + 1) R][stride] is
// written, first_lap = 1 from the grid, state->lap + 1 from a state.  edges [kGapEdgeSlots]: n_edges values, then +inf.
template <bool kFromState>
__global__ void __launch_bounds__(512)
race_gaps_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state, const double *__restrict__ edges,
                 uint32_t n_edges, const uint8_t *__restrict__ pairs, uint32_t n_pairs, uint64_t m, uint64_t sim_offset,
                 uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist, uint8_t *__restrict__ stage,
                 uint64_t stride, uint32_t n_batches)
{
    run_observed<kFromState>(P, state, m, sim_offset, seed_lo, seed_hi, hist, n_batches,
        [=](const Rows &s, const LapEnv &e, const RaceStart &at, uint64_t local) {
            GapObserver obs = {stage + local, (uint64_t)(e.n + 1 + (int)n_pairs) * stride, stride, edges, pairs, n_edges, n_pairs,
                               e.n, kFromState ? at.first_lap : 1};
            if (!kFromState) obs(s, 1, kEventNone);
            return obs;
        },
        [](const Rows &, const LapEnv &, const GapObserver &, uint64_t) {});
}

// One staged row's counts, added into out[width]: every thread of the block (blockDim.x = kGapsCountBlock) counts its
// words of the row's m bytes into its own column of `bins` ([value][thread] u32, width x kGapsCountBlock of them), then a
// reduction per value and one u64 atomic per non-zero one.  A value past the width counts in the last column.  Every
// thread of the block calls it (two barriers); the counting kernels of the gaps and pit-window calls are loops over it.
__device__ __forceinline__ void count_staged_row(uint32_t *bins, const uint8_t *__restrict__ bytes, uint64_t m, uint32_t width,
                                                 unsigned long long *__restrict__ out)
{
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t words = (m + 3) / 4;
    for (uint32_t v = 0; v < width; ++v) bins[v * kGapsCountBlock + t] = 0u;
    const uint32_t *row = reinterpret_cast<const uint32_t *>(bytes);
    for (uint64_t i = t; i < words; i += kGapsCountBlock) {
        const uint32_t w = row[i];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            uint32_t v = (w >> (8 * k)) & 0xFFu;
            v = v < width ? v : width - 1u;
            if (4 * i + k < m) ++bins[v * kGapsCountBlock + t];
        }
    }
    __syncthreads();
    for (uint32_t v = wave; v < width; v += kGapsCountBlock / 64) {
        const uint32_t *b = bins + v * kGapsCountBlock;
        uint32_t c = b[lane] + b[lane + 64] + b[lane + 128] + b[lane + 192];
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (lane == 0 && c) atomicAdd(&out[v], (unsigned long long)c);
    }
    __syncthreads();
}

// The staged rows' counts of m simulations, added into their places: staged row q = lap_index R + j (lap_index = lap -
// first_lap, R = n + 1 + n_pairs, lap0 = first_lap - 1) goes to
//   j < n       lap_gap[(lap0 + lap_index) n + j][B + 1]
//   j == n      lead[lap0 + lap_index][B + 1]
//   j > n       pair[(lap0 + lap_index) n_pairs + (j - n - 1)][2B + 1]
// A value past its row's width (none is written) counts in the row's last column.  blockDim.x = kGapsCountBlock; blocks
// grid-stride over the rows.  Dynamic LDS: (n_pairs ? 2B + 1 : B + 1) x kGapsCountBlock u32.
__global__ void __launch_bounds__(kGapsCountBlock)
gaps_count_rows(const uint8_t *__restrict__ stage, uint64_t stride, uint64_t m, uint32_t rows, uint32_t n, uint32_t n_pairs,
                uint32_t B, uint32_t lap0, unsigned long long *__restrict__ lap_gap, unsigned long long *__restrict__ lead,
                unsigned long long *__restrict__ pair)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *bins = reinterpret_cast<uint32_t *>(smem);              // [value][thread]
    const uint32_t R = n + 1u + n_pairs;
    for (uint32_t q = blockIdx.x; q < rows; q += gridDim.x) {
        const uint32_t lap = lap0 + q / R, j = q % R;
        const uint32_t width = j <= n ? B + 1u : 2u * B + 1u;
        unsigned long long *out = j < n    ? lap_gap + ((uint64_t)lap * n + j) * width
                                  : j == n ? lead + (uint64_t)lap * width
                                           : pair + ((uint64_t)lap * n_pairs + (j - n - 1u)) * width;
        count_staged_row(bins, stage + (uint64_t)q * stride, m, width, out);
    }
}

}  // namespace mcgp
