// moves.hip.h -- how the field moves in a race, counted on the device (mcgp_run_moves, include/mcgp.h).
//
// race_moves_kernel runs mcgp_run's simulations (from the grid, kFromState false) or mcgp_run_from_state's (from one
// state) with the generic kernel's code -- run_observed (resume.hip.h), the analysis kernels' shared lane body -- and the
// trace's own per-lap observer (TraceObserver, trace.hip.h), which sees the rows after update_positions of every lap.
// Simulation i draws exactly what those calls' simulation i draws, so the position histogram is theirs.  Definitions
// (include/mcgp.h has them in full), all read at that point of lap k:
//
//   run_k(d)   d is not retired after lap k;  pos_k(d) its running position among the running cars in `ord` order;
//   pit_k(d)   running after lap k with tyre age 0, k >= 2 (the trace's definition);
//   baseline   from the grid pos_0(d) = d's sampled grid slot, every car running; from a state after lap k0 the order
//              start_from_state leaves after its own update_positions (pos_k0);
//   start gain slot(d) - pos_1(d), from the grid only; a car that retires on lap 1 has none;
//   pass       on lap k (2..L from the grid, k0 + 1..L from a state), for a and b running after laps k - 1 and k: a was
//              behind b after lap k - 1 and is ahead of it after lap k.  Through the pits if pit_k(a) or pit_k(b), on
//              track otherwise.  A place gained because a car retired is not a pass.  This is the model's order change
//              between two lap ends, not a claim about a wheel-to-wheel move.
//
// Staging: one byte per (row, simulation), rows of `stride` bytes (a multiple of 256), a wave's lanes (adjacent
// simulations) on adjacent bytes:
//   rows (k - 1) n + d, k in 1..L    TraceObserver's byte of lap k: pos_k(d) or n (retired), | kTracePit.  From the grid
//                                    every lap is written; from a state the baseline row of lap k0 is written after the
//                                    start (its pit bit means nothing and is not read) and the rows before it are neither
//                                    written nor read
//   rows L n + d                     d's grid slot (from a state: the state's)
//   rows (L + 1) n + d               d's classified position, 0-based (classify_and_count's; retired cars behind)
// (L + 2) n bytes per simulation; the host sizes a chunk of simulations to a fixed budget (mcgp_hip.hip:
// kMovesStageBytes / ((L + 2) n)).  Pairwise work does not belong in the race kernel -- at 20 cars its block is 5 waves,
// one block per CU -- so two counting kernels that fill the machine read the staging afterwards:
//
//   moves_count_laps     a thread per simulation walks the laps once with the previous and the current lap's order.  A
//                        car's "cars ahead of me" set is one u32 mask (n <= 32): per lap the bytes give the running
//                        mask, the pit mask and car-by-position; one walk down the positions hands every running car
//                        its mask (the cars already passed by the walk), and
//                            made = ahead_prev[d] & ~ahead_cur[d] & both_running,   lost = ahead_cur[d] & ~ahead_prev[d]
//                        & both_running, each split by (pit_k(d) ? all : & pit mask): O(n) per lap.  A lap's bytes are
//                        loaded together, 32 loads in flight (one after the other each waits out a trip to memory, which
//                        made this kernel 7.2 ms of a 60 ms call at 10^6 S60 simulations).  Tables that are
//                        indexed at run time live in LDS, [car][thread] -- ahead_prev (u32), car-by-position (u8) and
//                        the car's four counts, saturating at 127, packed in one u32 -- 9 n bytes per thread and no
//                        scratch.  pair_passes and lap_passes are sums: u32 in LDS per block (pair: one LDS atomic per
//                        pass; lap: reduced over the wave first), one u64 global atomic per non-zero cell.  race_passes
//                        is a u32 LDS histogram [1024].  Each car's packed counts go to tot[d x stride + simulation] for
//                        the second kernel (4 n bytes per simulation beside the staging, only if passes are asked for).
//   moves_count_drivers  blockIdx.y = driver, blockIdx.x strides over the simulations, a thread per simulation: u32 LDS
//                        histograms of grid_fin [n][n] (slot, classified position), start_gain [2n] and passes [4][128],
//                        then one u64 global atomic per non-zero cell.  A count of 0 -- most simulations for the pit
//                        kinds -- is kept in four registers per thread and flushed once.
//
// Overflow.  Histograms receive at most one count per simulation and cell and a chunk is below 2^32 simulations.  The
// sums receive more: a lap_passes cell at most n (n - 1) / 2 <= 496 per simulation, a pair_passes cell at most L - 1 <=
// 999.  The host bounds a block of moves_count_laps to kMovesBlockShare = 2^21 simulations (the grid is at least tiles /
// 2^14), so a block's u32 cell stays below 2^21 x 999 < 2^31; the global cells are u64.
#pragma once
#include "resume.hip.h"
#include "trace.hip.h"

namespace mcgp {

constexpr uint32_t kMoveDriverCap = 127;         // a driver's passes of one kind in one race, saturating
constexpr uint32_t kMoveRaceCap = 1023;          // on-track passes in one race, saturating
constexpr int kMovesLapsBlock = 128;             // threads of a moves_count_laps block
constexpr int kMovesDriversBlock = 256;          // threads of a moves_count_drivers block
constexpr uint64_t kMovesBlockShare = 1ull << 21;   // simulations one moves_count_laps block may take

// Simulations sim_offset + [0, m) (m <= the chunk the staging holds) from the grid (kFromState false) or from `state`,
// with race_kernel's block shape and LDS.  hist [n][n] is ACCUMULATED into; stage [(L + 2) n][stride] is written.
template <bool kFromState>
__global__ void __launch_bounds__(512)
race_moves_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state, uint64_t m, uint64_t sim_offset,
                  uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist, uint8_t *__restrict__ stage,
                  uint64_t stride, uint32_t n_batches)
{
    run_observed<kFromState>(P, state, m, sim_offset, seed_lo, seed_hi, hist, n_batches,
        [=](const Rows &s, const LapEnv &e, const RaceStart &at, uint64_t local) {
            TraceObserver obs = TraceObserver::make(stage, stride, e.n, local);
            obs(s, at.first_lap - 1, kEventNone);                // lap 1 from the grid, the baseline row from a state
            return obs;
        },
        [=](const Rows &s, const LapEnv &e, const TraceObserver &obs, uint64_t local) {
            uint8_t *slot = stage + (uint64_t)e.L * obs.lap_bytes + local;
            uint8_t *pos = slot + obs.lap_bytes;
            for (int p = 0; p < e.n; ++p) {
                const uint32_t d = s.Ord(p);
                slot[(uint64_t)d * stride] = (uint8_t)gpos_of(s.Pk(d));
                pos[(uint64_t)d * stride] = (uint8_t)p;
            }
        });
}

// One saturating byte of a car's packed counts: ((w >> shift) & 255) + add, at most kMoveDriverCap.
__device__ __forceinline__ uint32_t move_sat(uint32_t w, int shift, uint32_t add)
{
    const uint32_t v = ((w >> shift) & 0xFFu) + add;             // (<= 127 + 31)
    return (v < kMoveDriverCap ? v : kMoveDriverCap) << shift;
}

// A car index read back from the car-by-position table (below n: a lap's bytes name every position once).
__device__ __forceinline__ uint32_t move_car(uint32_t d, uint32_t n) { return d < n ? d : n - 1u; }

// The passes of m simulations, lap by lap from the baseline row of lap `lap0` (1 from the grid): tot [n][stride] =
// every car's counts (made on track | lost on track << 8 | gained through the pits << 16 | lost through the pits << 24,
// each saturating at 127), race_passes [1024], lap_passes [L + 1][2] and pair_passes [n][n] are added into; each may be
// NULL and is then not counted.  blockDim.x = kMovesLapsBlock; blocks stride over the simulations.  Dynamic LDS:
// 9 n kMovesLapsBlock bytes of tables, then (n n + 2 (L + 1) + 1024) u32.
__global__ void __launch_bounds__(kMovesLapsBlock)
moves_count_laps(const uint8_t *__restrict__ stage, uint64_t stride, uint64_t m, uint32_t n, uint32_t L, uint32_t lap0,
                 uint32_t *__restrict__ tot, unsigned long long *__restrict__ race_passes,
                 unsigned long long *__restrict__ lap_passes, unsigned long long *__restrict__ pair_passes)
{
    constexpr uint32_t T = kMovesLapsBlock;
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *t_ahead = reinterpret_cast<uint32_t *>(smem);            // [car][thread]: the cars ahead after the last lap
    uint32_t *t_cnt = t_ahead + n * T;                                 // [car][thread]: the car's four counts
    uint32_t *s_pair = t_cnt + n * T;                                  // [n][n]
    uint32_t *s_lap = s_pair + n * n;                                  // [L + 1][2]
    uint32_t *s_race = s_lap + 2 * (L + 1);                            // [1024]
    uint8_t *t_car = reinterpret_cast<uint8_t *>(s_race + kMoveRaceCap + 1);   // [position][thread]
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < n * n + 2 * (L + 1) + kMoveRaceCap + 1; i += T) s_pair[i] = 0u;
    __syncthreads();

    const uint64_t lap_bytes = (uint64_t)n * stride;
    const uint64_t step = (uint64_t)gridDim.x * T;
    // wave-uniform loops (the lap sums are reduced over the wave): a lane without a simulation sees every car retired
    for (uint64_t base = (uint64_t)blockIdx.x * T; base < m; base += step) {
        const uint64_t i = base + t;
        const bool valid = i < m;
        const uint8_t *col = stage + (valid ? i : 0);
        uint32_t run_prev = 0u, race = 0u;
        for (uint32_t lap = lap0; lap <= L; ++lap) {
            const uint8_t *row = col + (uint64_t)(lap - 1) * lap_bytes;
            // the lap's bytes, all kMaxCars loads in flight before the first is used (a row past the field repeats the
            // last car's: the same cache line, and never used)
            uint32_t bytes[kMaxCars];
#pragma unroll
            for (uint32_t d = 0; d < (uint32_t)kMaxCars; ++d) bytes[d] = row[(uint64_t)(d < n ? d : n - 1u) * stride];
            uint32_t run = 0u, pit = 0u;
#pragma unroll
            for (uint32_t d = 0; d < (uint32_t)kMaxCars; ++d) {
                const uint32_t b = bytes[d];
                const uint32_t p = b & kTracePosMask;
                if (valid && d < n && p < n) {
                    run |= 1u << d;
                    pit |= ((b >> 7) & 1u) << d;
                    t_car[p * T + t] = (uint8_t)d;
                }
            }
            const uint32_t r = (uint32_t)__popc(run);                  // positions 0 .. r - 1 are taken, each once
            uint32_t acc = 0u, lap_trk = 0u, lap_pit = 0u;
            uint32_t next = t_car[t];                                  // (read one position ahead of its use)
            if (lap == lap0) {
                for (uint32_t q = 0; q < r; ++q) {
                    const uint32_t d = move_car(next, n);
                    next = t_car[(q + 1u < n ? q + 1u : q) * T + t];
                    t_ahead[d * T + t] = acc;
                    acc |= 1u << d;
                }
                for (uint32_t d = 0; d < n; ++d) t_cnt[d * T + t] = 0u;
            } else {
                const uint32_t both = run_prev & run;
                for (uint32_t q = 0; q < r; ++q) {
                    const uint32_t d = move_car(next, n);
                    next = t_car[(q + 1u < n ? q + 1u : q) * T + t];
                    const uint32_t bit = 1u << d;
                    const uint32_t before = t_ahead[d * T + t];
                    const uint32_t mine = (run_prev & bit) ? both & ~bit : 0u;    // (a running car ran the lap before)
                    const uint32_t made = before & ~acc & mine, lost = acc & ~before & mine;
                    const uint32_t through = (pit & bit) ? 0xFFFFFFFFu : pit;
                    const uint32_t made_trk = made & ~through, lost_trk = lost & ~through;
                    const uint32_t c_mt = (uint32_t)__popc(made_trk), c_mp = (uint32_t)__popc(made & through);
                    const uint32_t c_lt = (uint32_t)__popc(lost_trk), c_lp = (uint32_t)__popc(lost & through);
                    if (made | lost) {
                        const uint32_t w = t_cnt[d * T + t];
                        t_cnt[d * T + t] = move_sat(w, 0, c_mt) | move_sat(w, 8, c_lt) | move_sat(w, 16, c_mp) |
                                           move_sat(w, 24, c_lp);
                    }
                    lap_trk += c_mt;
                    lap_pit += c_mp;
                    if (pair_passes)
                        for (uint32_t rest = made_trk; rest; rest &= rest - 1u)
                            atomicAdd(&s_pair[d * n + (uint32_t)(__ffs((int)rest) - 1)], 1u);
                    t_ahead[d * T + t] = acc;
                    acc |= bit;
                }
                race += lap_trk;
                if (lap_passes) {
                    // at most 64 x 496 of either kind in a wave: both fit one u32, 16 bits each
                    uint32_t both_sums = lap_trk | (lap_pit << 16);
                    for (int off = 32; off > 0; off >>= 1) both_sums += __shfl_down(both_sums, off, 64);
                    if ((t & 63u) == 0u) {
                        if (both_sums & 0xFFFFu) atomicAdd(&s_lap[2 * lap], both_sums & 0xFFFFu);
                        if (both_sums >> 16) atomicAdd(&s_lap[2 * lap + 1], both_sums >> 16);
                    }
                }
            }
            run_prev = run;
        }
        if (valid) {
            if (race_passes) atomicAdd(&s_race[race < kMoveRaceCap ? race : kMoveRaceCap], 1u);
            if (tot)
                for (uint32_t d = 0; d < n; ++d) tot[(uint64_t)d * stride + i] = t_cnt[d * T + t];
        }
    }
    __syncthreads();

    if (pair_passes)
        for (uint32_t i = t; i < n * n; i += T)
            if (s_pair[i]) atomicAdd(&pair_passes[i], (unsigned long long)s_pair[i]);
    if (lap_passes)
        for (uint32_t i = t; i < 2 * (L + 1); i += T)
            if (s_lap[i]) atomicAdd(&lap_passes[i], (unsigned long long)s_lap[i]);
    if (race_passes)
        for (uint32_t i = t; i <= kMoveRaceCap; i += T)
            if (s_race[i]) atomicAdd(&race_passes[i], (unsigned long long)s_race[i]);
}

// Per driver (blockIdx.y) the counts of m simulations, added into grid_fin [n][n][n] and, unless NULL, start_gain
// [n][2n] (from the grid only: it reads lap 1's row) and passes [n][4][128] (from tot).  blockDim.x =
// kMovesDriversBlock; the blocks of a driver stride over the simulations.
__global__ void __launch_bounds__(kMovesDriversBlock)
moves_count_drivers(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ tot, uint64_t stride, uint64_t m,
                    uint32_t n, uint32_t L, unsigned long long *__restrict__ grid_fin,
                    unsigned long long *__restrict__ start_gain, unsigned long long *__restrict__ passes)
{
    __shared__ uint32_t s_gf[kMaxCars * kMaxCars];                     // [slot][position]
    __shared__ uint32_t s_gain[2 * kMaxCars];
    __shared__ uint32_t s_pass[4 * (kMoveDriverCap + 1)];
    const uint32_t t = threadIdx.x, d = blockIdx.y;
    for (uint32_t i = t; i < n * n; i += kMovesDriversBlock) s_gf[i] = 0u;
    for (uint32_t i = t; i < 2 * n; i += kMovesDriversBlock) s_gain[i] = 0u;
    for (uint32_t i = t; i < 4 * (kMoveDriverCap + 1); i += kMovesDriversBlock) s_pass[i] = 0u;
    __syncthreads();

    const uint64_t lap_bytes = (uint64_t)n * stride;
    const uint8_t *__restrict__ lap1 = stage + (uint64_t)d * stride;
    const uint8_t *__restrict__ slots = lap1 + (uint64_t)L * lap_bytes;
    const uint8_t *__restrict__ finish = slots + lap_bytes;
    const uint32_t *__restrict__ trow = tot + (uint64_t)d * stride;
    uint32_t zero[4] = {0u, 0u, 0u, 0u};                               // simulations without a pass of that kind
    for (uint64_t i = (uint64_t)blockIdx.x * kMovesDriversBlock + t; i < m; i += (uint64_t)gridDim.x * kMovesDriversBlock) {
        uint32_t slot = slots[i], p = finish[i];
        slot = slot < n ? slot : n - 1u;                               // (below n: the race kernel writes no other)
        p = p < n ? p : n - 1u;
        atomicAdd(&s_gf[slot * n + p], 1u);
        if (start_gain) {
            const uint32_t p1 = lap1[i] & kTracePosMask;
            atomicAdd(&s_gain[p1 < n ? slot + n - 1u - p1 : 2u * n - 1u], 1u);
        }
        if (passes) {
            const uint32_t w = trow[i];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                uint32_t c = (w >> (8 * k)) & 0xFFu;
                c = c < kMoveDriverCap ? c : kMoveDriverCap;
                if (c) atomicAdd(&s_pass[k * (kMoveDriverCap + 1) + c], 1u);
                else ++zero[k];
            }
        }
    }
    if (passes) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (zero[k]) atomicAdd(&s_pass[k * (kMoveDriverCap + 1)], zero[k]);
    }
    __syncthreads();

    for (uint32_t i = t; i < n * n; i += kMovesDriversBlock)
        if (s_gf[i]) atomicAdd(&grid_fin[(uint64_t)d * n * n + i], (unsigned long long)s_gf[i]);
    if (start_gain)
        for (uint32_t i = t; i < 2 * n; i += kMovesDriversBlock)
            if (s_gain[i]) atomicAdd(&start_gain[(uint64_t)d * 2 * n + i], (unsigned long long)s_gain[i]);
    if (passes)
        for (uint32_t i = t; i < 4 * (kMoveDriverCap + 1); i += kMovesDriversBlock)
            if (s_pass[i]) atomicAdd(&passes[(uint64_t)d * 4 * (kMoveDriverCap + 1) + i], (unsigned long long)s_pass[i]);
}

}  // namespace mcgp
