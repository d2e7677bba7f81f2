// stints.hip.h -- tyre stints of a race, counted on the device (mcgp_run_stints, include/mcgp.h).
//
// race_stints_kernel runs mcgp_run's simulations (from the grid, kFromState false) or mcgp_run_from_state's (from one
// state) with the generic kernel's code -- run_observed (resume.hip.h), the analysis kernels' shared lane body -- and a
// per-lap observer (StintObserver) that sees the rows after update_positions of every lap run_laps runs: laps 2..L from
// the grid (lap 1 has no pit step and no event), laps k + 1 .. L from a state after lap k.  Simulation i draws exactly
// what those calls' simulation i draws, so the position histogram is theirs.  Read at that point of lap k (the state the
// CPU oracle's per-lap trace records):
//
//   pit stop          the car is running after lap k with tyre age 0 (trace.hip.h's definition: only run_laps' pit branch
//                     leaves a running car at age 0, every other path adds the car's own lap);
//   red-flag change   lap k's event is a red flag and the car is running after lap k (the red flag hands every running
//                     car a new set before the lap; a car that retires on the lap never runs on it);
//   new stint         a pit stop or a red-flag change on lap k, one stint for both together (the set fitted under the red
//                     flag never completes a lap); its compound is the car's after lap k.
//   stint 0           the compound the start leaves in pk: _initialize_cars' after any start hook from the grid (a car
//                     that retires on lap 1 keeps it), the state's own from a state, for retired cars too.
// A retired car is never running again, so its stops and stints count up to its retirement.
//
// Record: one u64 per (driver, simulation), kept in the staging itself, rec[driver x stride + simulation]: rows by
// driver, a wave's lanes (adjacent simulations) on adjacent u64, 512 contiguous bytes per access.  Only the lane that
// owns the simulation touches it (no atomics): written once after the start, then read, changed and written back on the
// rare (lap, car) that begins a stint.
//   bits  0 ..  3   stints so far, 1 .. 15 (saturating: 15 = 15 or more; a sequence code needs only "more than 4")
//   bits  4 .. 15   the compounds of stints 0 .. 3, 3 bits each (stint j at bit 4 + 3 j); later stints are not kept
//   bits 16 .. 19   pit stops so far, 0 .. 15 (saturating; the counts cap it at kStintStops)
//   bits 20 .. 59   the laps of stops 1 .. 4, 10 bits each (stop k + 1 at bit 20 + 10 k; laps <= 1000); later stops
//                   are not kept; a field of a stop that did not happen is 0
// After classification the lane writes every driver's classified position (0-based) as a byte, pos[driver x stride +
// simulation], behind the records (at byte 8 n stride; stride is a multiple of 256).  9 n bytes per simulation.  The host
// sizes a chunk of simulations to a fixed staging budget (mcgp_hip.hip: kStintsStageBytes / (9 n)), launches the race
// kernel on it, then stints_count.
//
// stints_count: blockIdx.y = driver, blockIdx.x strides over the simulations, a thread per simulation, u32 histograms in
// dynamic LDS -- [4][L + 1] stop laps, [5][n] stops x position, [1296] sequences, (4 (L + 1) + 5 n + 1296) x 4 bytes: 6.4
// KiB at 60 laps and 20 cars, 21 KiB at 1000 laps -- then one u64 global atomic per non-zero cell.  What nearly every
// simulation of a driver shares does not go to LDS one lane at a time: "no such stop" (column 0 of a stop-lap row) is
// counted in four registers per thread and flushed once; the sequence code -- two or three codes hold most simulations
// of a driver -- is aggregated per wave (wave_count: one LDS atomic per distinct code of the wave's 64 lanes).  Stop laps
// and (stops, position) cells spread over tens of bins and take one LDS atomic each.
//
// Overflow: a chunk is at most max_sims_per_launch() < 2^32 simulations and a cell receives at most one count per
// simulation, so no u32 counter can wrap.
#pragma once
#include "resume.hip.h"

namespace mcgp {

constexpr uint32_t kStintStops = 4;              // stops whose lap is recorded; stop counts are capped here
constexpr uint32_t kStintSeq = 4;                // stints a sequence code holds
constexpr uint32_t kStintSeqCodes = 1296;        // 6^4
constexpr int kStintsCountBlock = 256;           // threads of a counting block

// the record's fields
constexpr uint32_t kStintCountMask = 15u;
constexpr int kStintCompShift = 4;               // + 3 j
constexpr int kStintStopsShift = 16;
constexpr int kStintLapShift = 20;               // + 10 k

// The stints kernel's per-lap observer: one lane's race.
struct StintObserver {
    uint64_t *lane;         // this lane's record of driver 0 (rec + local)
    uint64_t stride;        // u64 from one driver's row to the next
    int n;

    __device__ __forceinline__ void start(const Rows &s) const
    {
        for (int d = 0; d < n; ++d)
            lane[(uint64_t)d * stride] = 1ull | ((uint64_t)((s.Pk((uint32_t)d) >> kCompShift) & 7u) << kStintCompShift);
    }

    __device__ __forceinline__ void operator()(const Rows &s, int lap, int event)
    {
        const bool red = event == kEventRed;
        for (int i = 0; i < n; ++i) {
            const uint32_t d = s.Ord(i);
            const uint32_t pk = s.Pk(d);
            const bool stop = (pk & kAgeMask) == 0u;
            if ((pk & kDnf) || !(stop || red)) continue;
            uint64_t r = lane[(uint64_t)d * stride];
            const uint32_t stints = (uint32_t)r & kStintCountMask;
            if (stints < kStintSeq) r |= (uint64_t)((pk >> kCompShift) & 7u) << (kStintCompShift + 3 * (int)stints);
            if (stints < kStintCountMask) r += 1ull;
            if (stop) {
                const uint32_t stops = (uint32_t)(r >> kStintStopsShift) & 15u;
                if (stops < kStintStops) r |= (uint64_t)(uint32_t)lap << (kStintLapShift + 10 * (int)stops);
                if (stops < 15u) r += 1ull << kStintStopsShift;
            }
            lane[(uint64_t)d * stride] = r;
        }
    }
};

// Simulations sim_offset + [0, m) (m <= the chunk the staging holds) from the grid (kFromState false) or from `state`,
// with race_kernel's block shape and LDS.  hist [n][n] is ACCUMULATED into; rec [n][stride] u64 and pos [n][stride]
// bytes are written.
template <bool kFromState>
__global__ void __launch_bounds__(512)
race_stints_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state, uint64_t m, uint64_t sim_offset,
                   uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist, uint64_t *__restrict__ rec,
                   uint8_t *__restrict__ pos, uint64_t stride, uint32_t n_batches)
{
    run_observed<kFromState>(P, state, m, sim_offset, seed_lo, seed_hi, hist, n_batches,
        [=](const Rows &s, const LapEnv &e, const RaceStart &, uint64_t local) {
            const StintObserver obs = {rec + local, stride, e.n};
            obs.start(s);
            return obs;
        },
        [=](const Rows &s, const LapEnv &e, const StintObserver &, uint64_t local) {
            uint8_t *out = pos + local;
            for (int p = 0; p < e.n; ++p) out[(uint64_t)s.Ord(p) * stride] = (uint8_t)p;
        });
}

// The sequence code of a record: sum over the stints j < m of (compound_j + 1) 6^j for m <= 4 stints, 0 for more.
__device__ __forceinline__ uint32_t stint_code(uint64_t r)
{
    const uint32_t stints = (uint32_t)r & kStintCountMask;
    if (stints > kStintSeq) return 0u;
    uint32_t code = 0u, scale = 1u;
    for (uint32_t j = 0; j < stints; ++j) {
        code += (((uint32_t)(r >> (kStintCompShift + 3 * (int)j)) & 7u) + 1u) * scale;
        scale *= 6u;
    }
    return code < kStintSeqCodes ? code : 0u;                          // (compounds are 0 .. 4: no code reaches 6^4)
}

// bins[key] += the number of the wave's lanes with `valid` and that key: one LDS atomic per distinct key of the wave
// instead of one per lane.  Every lane of the wave must call it (wave-uniform control flow).
__device__ __forceinline__ void wave_count(uint32_t *bins, uint32_t key, bool valid)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll(todo) - 1;
        const uint32_t k = (uint32_t)__shfl((int)key, leader, 64);
        const unsigned long long same = __ballot(valid && key == k);
        if (lane == (uint32_t)leader) atomicAdd(&bins[k], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// The records' and positions' counts of m simulations, added into stop_lap [n][4][L + 1] and, unless NULL, stops_pos
// [n][5][n] and seq [n][1296].  gridDim.y = n (the driver); the blocks of a driver stride over the simulations.
// blockDim.x = kStintsCountBlock.  Dynamic LDS: (4 (L + 1) + 5 n + 1296) u32.
__global__ void __launch_bounds__(kStintsCountBlock)
stints_count(const uint64_t *__restrict__ rec, const uint8_t *__restrict__ pos, uint64_t stride, uint64_t m, uint32_t n,
             uint32_t L, unsigned long long *__restrict__ stop_lap, unsigned long long *__restrict__ stops_pos,
             unsigned long long *__restrict__ seq)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *s_lap = reinterpret_cast<uint32_t *>(smem);              // [4][L + 1]
    uint32_t *s_sp = s_lap + kStintStops * (L + 1);                    // [5][n]
    uint32_t *s_seq = s_sp + (kStintStops + 1) * n;                    // [1296]
    const uint32_t t = threadIdx.x, d = blockIdx.y;
    const uint32_t cells = kStintStops * (L + 1) + (kStintStops + 1) * n + kStintSeqCodes;
    for (uint32_t i = t; i < cells; i += kStintsCountBlock) s_lap[i] = 0u;
    __syncthreads();

    const uint64_t *__restrict__ row = rec + (uint64_t)d * stride;
    const uint8_t *__restrict__ prow = pos + (uint64_t)d * stride;
    uint32_t none[kStintStops] = {0u, 0u, 0u, 0u};                     // simulations without a (k + 1)-th stop
    const uint64_t step = (uint64_t)gridDim.x * kStintsCountBlock;
    // the loop is wave-uniform (wave_count): every lane runs it as long as any simulation is left for the block
    for (uint64_t base = (uint64_t)blockIdx.x * kStintsCountBlock; base < m; base += step) {
        const uint64_t i = base + t;
        const bool valid = i < m;
        const uint64_t r = valid ? row[i] : 0ull;
        uint32_t stops = (uint32_t)(r >> kStintStopsShift) & 15u;
        stops = stops < kStintStops ? stops : kStintStops;
        if (valid) {
#pragma unroll
            for (uint32_t k = 0; k < kStintStops; ++k) {
                uint32_t lap = (uint32_t)(r >> (kStintLapShift + 10 * (int)k)) & 0x3FFu;
                lap = lap <= L ? lap : L;                              // (no lap above L is written)
                if (k < stops) atomicAdd(&s_lap[k * (L + 1) + lap], 1u);
                else ++none[k];
            }
            if (stops_pos) {
                uint32_t p = prow[i];
                p = p < n ? p : n - 1u;                                // (a position below n: the race kernel writes no other)
                atomicAdd(&s_sp[stops * n + p], 1u);
            }
        }
        if (seq) wave_count(s_seq, stint_code(r), valid);
    }
#pragma unroll
    for (uint32_t k = 0; k < kStintStops; ++k)
        if (none[k]) atomicAdd(&s_lap[k * (L + 1)], none[k]);
    __syncthreads();

    for (uint32_t i = t; i < kStintStops * (L + 1); i += kStintsCountBlock)
        if (s_lap[i]) atomicAdd(&stop_lap[(uint64_t)d * kStintStops * (L + 1) + i], (unsigned long long)s_lap[i]);
    if (stops_pos)
        for (uint32_t i = t; i < (kStintStops + 1) * n; i += kStintsCountBlock)
            if (s_sp[i]) atomicAdd(&stops_pos[(uint64_t)d * (kStintStops + 1) * n + i], (unsigned long long)s_sp[i]);
    if (seq)
        for (uint32_t i = t; i < kStintSeqCodes; i += kStintsCountBlock)
            if (s_seq[i]) atomicAdd(&seq[(uint64_t)d * kStintSeqCodes + i], (unsigned long long)s_seq[i]);
}

}  // namespace mcgp
