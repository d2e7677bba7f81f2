// pit_window.hip.h -- where a car would rejoin if it stopped at the end of a lap, counted on the device
// (mcgp_run_pit_windows, include/mcgp.h).
//
// race_window_kernel runs mcgp_run's simulations (from the grid, kFromState false) or mcgp_run_from_state's (from one
// state) with the generic kernel's code -- run_observed (resume.hip.h) -- and a per-lap observer (WindowObserver) that
// sees the rows where the gaps observer sees them: after update_positions of every recorded lap, laps 1..L from the
// grid, laps k + 1 .. L from a state after lap k.  Simulation i draws exactly what those calls' simulation i draws, so
// the position histogram is theirs.  NOTHING IS RE-SIMULATED: the race goes on as if no window existed, and a window
// (driver a, loss) only asks, of the times the race has at that point,
//
//   t*               Cum(a) + loss: one binary64 addition, the model's own stop arithmetic (t = t + pit_loss);
//   ahead at rejoin  a running car d != a with (Cum(d), slot d) < (t*, slot a), the running order's own key; every
//                    other running car d != a is behind at rejoin;
//   rejoin position  the number of running cars ahead at rejoin, 0-based;
//   places lost      rejoin position - a's own running position, in [0, n - 1] (loss >= 0: every car ahead of a now is
//                    ahead at rejoin); 0 is a free stop;
//   car ahead        the last car in running order among those ahead at rejoin; car behind: the first among those behind;
//   gap ahead        t* - Cum(car ahead): one subtraction, >= 0;  gap behind: Cum(car behind) - t*, >= 0.
// The race after such a stop (fresh tyres, the traffic's reaction) is mcgp_run_strategies' question, not this one's.
//
// One walk per group of windows: `ord` is sorted by the key when the observer runs, so the cars ahead at rejoin are a
// prefix of the running order without a, "last ahead" is the last car seen ahead and "first behind" the first seen
// behind.  A group of kWindowGroup windows is held in registers -- per window t*, a's slot, the count ahead, a's own
// position, and time and index of the car ahead and of the car behind -- and the running order is walked ONCE per
// group, three LDS gathers per car (ord, pk, cum), not once per window: 8 walks at 64 windows, not 64.  The loops have
// wave-uniform lengths (n cars, W windows in whole groups); what a lane's own data decides are values, by selects.
// kWindowGroup = 8 by the build's resource report (<false> / <true>: 82 / 93 VGPRs at 2, 105 / 115 at 4, 150 / 160 at
// 8, no scratch and no spilled VGPR at any of them): the rows' LDS holds a field of 11 cars or more at two waves per
// SIMD or fewer whatever the registers, and two waves have 256 VGPRs each, so 8 costs such a field no resident wave and
// halves the walks of 4; 16 would not fit 256.  Smaller fields lose waves to it (3 per SIMD by registers) and are the
// cheap ones.  DESIGN.md has the table.
//
// The window tables (driver bytes, losses) and the edges are wave-uniform and read with scalar loads from const
// __restrict__ kernel arguments at uniform indices; the tables are padded to whole groups (driver 0, loss 0: computed,
// never written).  Bins: gap_bin of gaps.hip.h as it is.  No LDS beyond the rows.
//
// Staging: one byte per (recorded lap, window, row, simulation), [((lap - first_lap) W + w) 5 + row][simulation] with
// a row stride of `stride` bytes (adjacent lanes write adjacent bytes):
//   row 0  rejoin      position 0 .. n - 1; n = a has retired                                          width n + 1
//   row 1  lost        places lost 0 .. n - 1; n = retired                                             width n + 1
//   row 2  ahead       driver index of the car ahead; n = rejoins in the lead; n + 1 = retired         width n + 2
//   row 3  gap_ahead   bin; B = no car ahead, or retired                                               width B + 1
//   row 4  gap_behind  bin; B = no car behind, or retired                                              width B + 1
// n <= 32 and B <= 64: every value fits a byte.  The host sizes a chunk of simulations to a fixed staging budget
// (mcgp_hip.hip: kWindowStageBytes / (recorded laps x 5 W)), launches the race kernel on it, then window_count_rows: a
// block per staged row over count_staged_row (gaps.hip.h).
#pragma once
#include "gaps.hip.h"

namespace mcgp {

constexpr uint32_t kMaxPitWindows = 64;
constexpr uint32_t kWindowGroup = 8;             // windows held in registers per walk of the running order
constexpr uint32_t kWindowSlots = (kMaxPitWindows + kWindowGroup - 1) / kWindowGroup * kWindowGroup;   // the device's tables
constexpr uint32_t kWindowRows = 5;              // staged rows per window: rejoin, lost, ahead, gap_ahead, gap_behind

// The pit-window kernel's per-lap observer: one lane's race.
struct WindowObserver {
    uint8_t *lane;                          // this lane's byte of the first recorded lap's row 0 (stage + local)
    uint64_t lap_bytes;                     // bytes from one lap's rows to the next: 5 W x stride
    uint64_t stride;                        // bytes from one row to the next
    const double *__restrict__ edges;       // [kGapEdgeSlots]
    const uint8_t *__restrict__ drivers;    // [kWindowSlots]
    const double *__restrict__ losses;      // [kWindowSlots]
    uint32_t n_edges, n_windows;
    int n, first_lap;

    __device__ __forceinline__ void operator()(const Rows &s, int lap, int /*event*/)
    {
        constexpr uint32_t G = kWindowGroup, kNone = 0xFFu;
        uint8_t *rows = lane + (uint64_t)(lap - first_lap) * lap_bytes;
        const uint32_t B = n_edges + 1u;
        for (uint32_t w0 = 0; w0 < n_windows; w0 += G) {
            uint32_t a[G], slot[G], out[G], ahead_n[G], own[G], ahead_d[G], behind_d[G];
            double ts[G], ahead_t[G], behind_t[G];
#pragma unroll
            for (uint32_t g = 0; g < G; ++g) {
                a[g] = drivers[w0 + g];
                const uint32_t pk = s.Pk(a[g]);
                slot[g] = gpos_of(pk);
                out[g] = pk & kDnf;
                ts[g] = s.Cum(a[g]) + losses[w0 + g];
                ahead_n[g] = own[g] = 0u;
                ahead_d[g] = behind_d[g] = kNone;
                ahead_t[g] = behind_t[g] = ts[g];
            }
            for (int i = 0; i < n; ++i) {
                const uint32_t d = s.Ord(i);
                const uint32_t pk = s.Pk(d);
                if (pk & kDnf) continue;
                const double t = s.Cum(d);
                const uint32_t gd = gpos_of(pk);
#pragma unroll
                for (uint32_t g = 0; g < G; ++g) {
                    const bool self = d == a[g];
                    const bool ahead = !self && (t < ts[g] || (t == ts[g] && gd < slot[g]));
                    const bool first_behind = !self && !ahead && behind_d[g] == kNone;
                    own[g] = self ? ahead_n[g] : own[g];          // (every car before a in the order is ahead at rejoin)
                    ahead_n[g] += ahead ? 1u : 0u;
                    ahead_t[g] = ahead ? t : ahead_t[g];
                    ahead_d[g] = ahead ? d : ahead_d[g];
                    behind_t[g] = first_behind ? t : behind_t[g];
                    behind_d[g] = first_behind ? d : behind_d[g];
                }
            }
#pragma unroll
            for (uint32_t g = 0; g < G; ++g) {
                if (w0 + g >= n_windows) break;                   // (the padding of the last group)
                const uint32_t ga = gap_bin(edges, n_edges, ts[g] - ahead_t[g]);
                const uint32_t gb = gap_bin(edges, n_edges, behind_t[g] - ts[g]);
                const bool gone = out[g] != 0u;
                uint8_t *row = rows + (uint64_t)(w0 + g) * kWindowRows * stride;
                row[0] = (uint8_t)(gone ? (uint32_t)n : ahead_n[g]);
                row[stride] = (uint8_t)(gone ? (uint32_t)n : ahead_n[g] - own[g]);
                row[2 * stride] = (uint8_t)(gone ? (uint32_t)n + 1u : ahead_n[g] ? ahead_d[g] : (uint32_t)n);
                row[3 * stride] = (uint8_t)(gone || !ahead_n[g] ? B : ga);
                row[4 * stride] = (uint8_t)(gone || behind_d[g] == kNone ? B : gb);
            }
        }
    }
};

// Simulations sim_offset + [0, m) (m <= the chunk the staging holds) from the grid (kFromState false) or from `state`,
// with race_kernel's block shape and LDS.  hist [n][n] is ACCUMULATED into; stage [(L - first_lap + 1) 5 W][stride] is
// written, first_lap = 1 from the grid, state->lap + 1 from a state.  edges [kGapEdgeSlots]: n_edges values, then +inf;
// drivers, losses [kWindowSlots]: n_windows values, then 0.
template <bool kFromState>
__global__ void __launch_bounds__(512)
race_window_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state, const double *__restrict__ edges,
                   uint32_t n_edges, const uint8_t *__restrict__ drivers, const double *__restrict__ losses,
                   uint32_t n_windows, uint64_t m, uint64_t sim_offset, uint32_t seed_lo, uint32_t seed_hi,
                   unsigned long long *__restrict__ hist, uint8_t *__restrict__ stage, uint64_t stride, uint32_t n_batches)
{
    run_observed<kFromState>(P, state, m, sim_offset, seed_lo, seed_hi, hist, n_batches,
        [=](const Rows &s, const LapEnv &e, const RaceStart &at, uint64_t local) {
            WindowObserver obs = {stage + local, (uint64_t)(kWindowRows * n_windows) * stride, stride, edges, drivers, losses,
                                  n_edges, n_windows, e.n, kFromState ? at.first_lap : 1};
            if (!kFromState) obs(s, 1, kEventNone);
            return obs;
        },
        [](const Rows &, const LapEnv &, const WindowObserver &, uint64_t) {});
}

// The staged rows' counts of m simulations, added into their places: staged row q = (lap_index W + w) 5 + r (lap_index
// = lap - first_lap, lap0 = first_lap - 1) goes to
//   r == 0      rejoin[(lap0 + lap_index) W + w][n + 1]         r == 3      gap_ahead[(lap0 + lap_index) W + w][B + 1]
//   r == 1      lost[(lap0 + lap_index) W + w][n + 1]           r == 4      gap_behind[(lap0 + lap_index) W + w][B + 1]
//   r == 2      ahead[(lap0 + lap_index) W + w][n + 2]
// A value past its row's width (none is written) counts in the row's last column.  blockDim.x = kGapsCountBlock; blocks
// grid-stride over the rows.  Dynamic LDS: max(n + 2, B + 1) x kGapsCountBlock u32.
__global__ void __launch_bounds__(kGapsCountBlock)
window_count_rows(const uint8_t *__restrict__ stage, uint64_t stride, uint64_t m, uint32_t rows, uint32_t n, uint32_t W,
                  uint32_t B, uint32_t lap0, unsigned long long *__restrict__ rejoin, unsigned long long *__restrict__ lost,
                  unsigned long long *__restrict__ ahead, unsigned long long *__restrict__ gap_ahead,
                  unsigned long long *__restrict__ gap_behind)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *bins = reinterpret_cast<uint32_t *>(smem);              // [value][thread]
    for (uint32_t q = blockIdx.x; q < rows; q += gridDim.x) {
        const uint32_t r = q % kWindowRows;
        const uint64_t cell = (uint64_t)lap0 * W + q / kWindowRows;   // (lap, window)
        const uint32_t width = r < 2u ? n + 1u : r == 2u ? n + 2u : B + 1u;
        unsigned long long *base = r == 0u ? rejoin : r == 1u ? lost : r == 2u ? ahead : r == 3u ? gap_ahead : gap_behind;
        count_staged_row(bins, stage + (uint64_t)q * stride, m, width, base + cell * width);
    }
}

}  // namespace mcgp
