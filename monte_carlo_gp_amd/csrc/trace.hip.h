// trace.hip.h -- what happened lap by lap in a race, counted on the device (mcgp_run_trace, include/mcgp.h).
//
// race_trace_kernel runs mcgp_run's simulations with the generic kernel's code -- start_from_grid for the grid and
// lap 1, run_laps for laps 2..L, classify_and_count: run_observed (resume.hip.h), the lane body the five analysis
// kernels share -- and a per-lap observer (TraceObserver) that sees the rows after update_positions of every lap, lap 1
// included.  Simulation i draws exactly what race_kernel's simulation i draws, so
// its position histogram is mcgp_run's.  Read at that point of lap k (the state the CPU oracle's per-lap trace records):
//
//   running position  rank of a car among the cars not retired, in `ord` order (cumulative time, grid slot); a retired
//                     car has none and is recorded as n.  After lap L these are the classified positions of the runners.
//   pit stop          laps k in 2..L on which the car took run_laps' pit branch (age = 0u there).  The observer uses the
//                     equivalent form "running after lap k with tyre age 0": a red flag or safety car never leaves a
//                     running car at age 0, because its own lap adds 1 after the event, so only the pit branch can.
//   fastest lap       the smallest Last(d) of a car running after lap k, over laps 2..L (lap 1 records no lap time: the
//                     reference leaves last_lap_time at 0 there); a tie goes to the earlier lap, then to the better
//                     running position on that lap (strict <, laps in order, cars in running order).  A race in which
//                     no car completes a lap >= 2 has none.
//   race events       laps 2..L whose event draw gave a red flag, a safety car or a VSC (run_laps' short-circuit chain,
//                     drawn whether or not any car still runs).
//
// Staging: one byte per (lap, driver, simulation), [row = (lap - 1) n + driver][simulation] with a row stride of
// `stride` bytes, so that a wave's lanes (adjacent simulations) write adjacent bytes of a row: running position or n,
// | kTracePit.  Per simulation one u64 record: fastest-lap driver (kNoFastest: none) | red flags << 16 | safety cars
// << 32 | VSCs << 48, held in registers during the race.  The host sizes a chunk of simulations to a fixed staging
// budget (mcgp_hip.hip: kTraceStageBytes / (L n)), launches the race kernel on it, then the three counting kernels:
//
//   trace_count_positions  lap_pos[lap][driver][position | n]: a block per row, every thread counting its words of the
//                          row into its own column of u32 bins in LDS (no atomics, no bank conflicts), then a
//                          reduction per bin and one u64 global atomic per non-zero bin;
//   trace_count_laps       laps led and pit stops: a block column per driver (blockIdx.y), every thread taking 4
//                          simulations (one u32 per row) through the L rows, counting in registers, then a u32 LDS
//                          histogram [L + 1] of each and u64 global atomics;
//   trace_count_records    fastest lap [n] and events [3][L + 1] from the records, u32 LDS histograms, u64 atomics.
//
// Overflow: a chunk is at most max_sims_per_launch() < 2^32 simulations, so no u32 counter can wrap.
#pragma once
#include "resume.hip.h"

namespace mcgp {

constexpr uint32_t kTracePit = 0x80u;            // staging byte: the car pitted on this lap
constexpr uint32_t kTracePosMask = 0x3Fu;        // staging byte: running position, or n (retired)
constexpr uint32_t kNoFastest = 0xFFFFu;         // record: no car completed a lap >= 2
constexpr int kTraceCountBlock = 256;            // threads of a counting block

// The trace kernel's per-lap observer: one lane's race.
struct TraceObserver {
    uint8_t *lane;          // this lane's byte of row 0 (stage + local)
    uint64_t lap_bytes;     // bytes from one lap's rows to the next: n x stride
    uint64_t stride;        // bytes from one driver's row to the next
    int n;
    double best;            // fastest lap so far, and its driver (kNoFastest: none yet)
    uint32_t best_d;
    uint32_t red, sc, vsc;  // events so far

    // the observer of lane `local` over a staging of n rows of `stride` bytes per lap: nothing seen yet
    static __device__ __forceinline__ TraceObserver make(uint8_t *stage, uint64_t stride, int n, uint64_t local)
    {
        return {stage + local, (uint64_t)n * stride, stride, n, __builtin_inf(), kNoFastest, 0u, 0u, 0u};
    }

    __device__ __forceinline__ void operator()(const Rows &s, int lap, int event)
    {
        red += event == kEventRed;
        sc += event == kEventSc;
        vsc += event == kEventVsc;
        uint8_t *row = lane + (uint64_t)(lap - 1) * lap_bytes;
        uint32_t r = 0;
        for (int i = 0; i < n; ++i) {
            const uint32_t d = s.Ord(i);
            const uint32_t pk = s.Pk(d);
            uint32_t b = (uint32_t)n;
            if (!(pk & kDnf)) {
                b = r++;
                if (lap >= 2) {
                    if ((pk & kAgeMask) == 0u) b |= kTracePit;
                    const double t = s.Last(d);
                    if (t < best) { best = t; best_d = d; }
                }
            }
            row[(uint64_t)d * stride] = (uint8_t)b;
        }
    }
};

// mcgp_run's simulations sim_offset + [0, n_sims) (n_sims <= the chunk the staging holds), with race_kernel's block
// shape and LDS.  hist [n][n] is ACCUMULATED into; stage [L n][stride] and rec [n_sims] are written.
__global__ void __launch_bounds__(512)
race_trace_kernel(const KParams *__restrict__ P, uint64_t n_sims, uint64_t sim_offset, uint32_t seed_lo,
                  uint32_t seed_hi, unsigned long long *__restrict__ hist, uint8_t *__restrict__ stage, uint64_t stride,
                  uint64_t *__restrict__ rec, uint32_t n_batches)
{
    run_observed<false>(P, nullptr, n_sims, sim_offset, seed_lo, seed_hi, hist, n_batches,
        [=](const Rows &s, const LapEnv &e, const RaceStart &, uint64_t local) {
            TraceObserver obs = TraceObserver::make(stage, stride, e.n, local);
            obs(s, 1, kEventNone);
            return obs;
        },
        [=](const Rows &, const LapEnv &, const TraceObserver &obs, uint64_t local) {
            rec[local] = (uint64_t)obs.best_d | ((uint64_t)obs.red << 16) | ((uint64_t)obs.sc << 32) | ((uint64_t)obs.vsc << 48);
        });
}

// lap_pos [L n][n + 1] += the staged rows' counts: row r (= (lap - 1) n + driver) of m simulations, value v at
// lap_pos[r][v].  blockDim.x = kTraceCountBlock; blocks grid-stride over the rows.
__global__ void __launch_bounds__(kTraceCountBlock)
trace_count_positions(const uint8_t *__restrict__ stage, uint64_t stride, uint64_t m, uint32_t rows, uint32_t n,
                      unsigned long long *__restrict__ lap_pos)
{
    __shared__ uint32_t bins[(kMaxCars + 1) * kTraceCountBlock];      // [value][thread]
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t words = (m + 3) / 4;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        for (uint32_t v = 0; v <= n; ++v) bins[v * kTraceCountBlock + t] = 0u;
        const uint32_t *row = reinterpret_cast<const uint32_t *>(stage + (uint64_t)r * stride);
        for (uint64_t j = t; j < words; j += kTraceCountBlock) {
            const uint32_t w = row[j];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                uint32_t v = (w >> (8 * k)) & kTracePosMask;
                v = v < n ? v : n;
                if (4 * j + k < m) ++bins[v * kTraceCountBlock + t];
            }
        }
        __syncthreads();
        for (uint32_t v = wave; v <= n; v += kTraceCountBlock / 64) {
            const uint32_t *b = bins + v * kTraceCountBlock;
            uint32_t c = b[lane] + b[lane + 64] + b[lane + 128] + b[lane + 192];
            for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
            if (lane == 0 && c) atomicAdd(&lap_pos[(uint64_t)r * (n + 1) + v], (unsigned long long)c);
        }
        __syncthreads();
    }
}

// laps_led / stops [n][L + 1] += the number of simulations whose driver led / pitted on that many laps (either NULL:
// not written).  blockIdx.y = driver; each thread takes 4 simulations at a time.  Dynamic LDS: 2 (L + 1) u32.
__global__ void __launch_bounds__(kTraceCountBlock)
trace_count_laps(const uint8_t *__restrict__ stage, uint64_t stride, uint64_t m, uint32_t n, uint32_t L,
                 unsigned long long *__restrict__ laps_led, unsigned long long *__restrict__ stops)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *s_led = reinterpret_cast<uint32_t *>(smem);
    uint32_t *s_stop = s_led + (L + 1);
    const uint32_t t = threadIdx.x, d = blockIdx.y;
    for (uint32_t i = t; i < 2 * (L + 1); i += kTraceCountBlock) s_led[i] = 0u;
    __syncthreads();
    const uint64_t words = (m + 3) / 4;
    const uint64_t lap_bytes = (uint64_t)n * stride;
    const uint8_t *base = stage + (uint64_t)d * stride;
    for (uint64_t j = (uint64_t)blockIdx.x * kTraceCountBlock + t; j < words; j += (uint64_t)gridDim.x * kTraceCountBlock) {
        uint32_t led[4] = {0u, 0u, 0u, 0u}, stop[4] = {0u, 0u, 0u, 0u};
        for (uint32_t lap = 0; lap < L; ++lap) {
            const uint32_t w = reinterpret_cast<const uint32_t *>(base + (uint64_t)lap * lap_bytes)[j];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                led[k] += ((w >> (8 * k)) & kTracePosMask) == 0u;
                stop[k] += (w >> (8 * k + 7)) & 1u;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (4 * j + k < m) {
                atomicAdd(&s_led[led[k] < L ? led[k] : L], 1u);
                atomicAdd(&s_stop[stop[k] < L ? stop[k] : L], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = t; i <= L; i += kTraceCountBlock) {
        if (laps_led && s_led[i]) atomicAdd(&laps_led[(uint64_t)d * (L + 1) + i], (unsigned long long)s_led[i]);
        if (stops && s_stop[i]) atomicAdd(&stops[(uint64_t)d * (L + 1) + i], (unsigned long long)s_stop[i]);
    }
}

// fastest [n] and events [3][L + 1] += the records' counts (either NULL: not written).  Dynamic LDS: (kMaxCars +
// 3 (L + 1)) u32.
__global__ void __launch_bounds__(kTraceCountBlock)
trace_count_records(const uint64_t *__restrict__ rec, uint64_t m, uint32_t n, uint32_t L,
                    unsigned long long *__restrict__ fastest, unsigned long long *__restrict__ events)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *s_fast = reinterpret_cast<uint32_t *>(smem);
    uint32_t *s_ev = s_fast + kMaxCars;
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < kMaxCars + 3 * (L + 1); i += kTraceCountBlock) s_fast[i] = 0u;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kTraceCountBlock + t; i < m; i += (uint64_t)gridDim.x * kTraceCountBlock) {
        const uint64_t r = rec[i];
        const uint32_t f = (uint32_t)(r & 0xFFFFu);
        if (f < n) atomicAdd(&s_fast[f], 1u);
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t c = (uint32_t)(r >> (16 * (k + 1))) & 0xFFFFu;
            atomicAdd(&s_ev[k * (L + 1) + (c < L ? c : L)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = t; i < n; i += kTraceCountBlock)
        if (fastest && s_fast[i]) atomicAdd(&fastest[i], (unsigned long long)s_fast[i]);
    for (uint32_t i = t; i < 3 * (L + 1); i += kTraceCountBlock)
        if (events && s_ev[i]) atomicAdd(&events[i], (unsigned long long)s_ev[i]);
}

}  // namespace mcgp
