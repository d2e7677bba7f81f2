// conditions.hip.h -- combination and conditional odds, counted on the device (mcgp_run_conditions, include/mcgp.h).
//
// race_conditions_kernel runs mcgp_run's simulations (from the grid, kFromState false) or mcgp_run_from_state's (from one
// state) with the generic kernel's code -- run_observed (resume.hip.h), the analysis kernels' shared lane body -- and a
// per-lap observer that only counts the lap's event (EventCounter: three registers, no store).  Simulation i draws
// exactly what those calls' simulation i draws, so the position histogram is theirs.  At the flag the lane holds every
// fact a condition may ask for, all integers:
//
//   POSITION(a)      classified position of driver a, 1 .. n: the inverse of `ord` after classify_and_count, built once
//                    per race in the `out` row (the retirement laps drawn before the race are no longer needed);
//   GRID(a)          gpos_of(pk[a]) + 1;
//   RETIRED_LAP(a)   pk[a] & kAgeMask if kDnf is set (the lap of retirement, lap 1 and a state's own included), else 0;
//   AHEAD_BY(a, b)   POSITION(b) - POSITION(a);      GAINED(a)   GRID(a) - POSITION(a);
//   FINISHERS        the cars without kDnf;
//   RED_FLAGS, SAFETY_CARS, VSCS   the laps run_laps ran (2 .. L from the grid, state->lap + 1 .. L from a state) whose
//                    event was that one, as race_trace_kernel counts them.
//
// Evaluation: the condition table (the call's mcgp_condition array as it is: Cond below) lives in device memory and
// is the same for every lane: it is read through a const __restrict__ kernel argument at loop counters whose bounds are
// kernel arguments or table entries, so the loads are scalar and the loops over conditions and atoms have wave-uniform
// trip counts; the fact is a wave-uniform switch.  Only the value differs from lane to lane.  An atom holds iff
// (lo <= value <= hi) != (negate != 0), a condition iff all its atoms do (none: always); bit c of the lane's u64 mask is
// condition c.
//
// Staging, rows by simulation so that a wave's lanes (adjacent simulations) write adjacent addresses:
//   row p < n   [stride bytes]  the driver classified p-th (what orders_out holds, transposed)
//   then        [stride u64]    the masks, at byte n x stride (stride is a multiple of 256: aligned)
// n + 8 bytes per simulation.  The host sizes a chunk of simulations to a fixed staging budget (mcgp_hip.hip:
// kConditionsStageBytes / (n + 8)), launches the race kernel on it, then conditions_count.
//
// conditions_count: the conditions are split over blockIdx.y in groups of kCondGroup = 8, because [C][n][n] u32 does not
// fit one block's LDS at C = 64, n = 32 (256 KiB) while a group's does (32 KiB).  blockIdx.x strides over the
// simulations, a thread per simulation: it reads the mask, takes its group's byte, adds each bit to a register counter
// and -- only for the bits that are set, and only when the caller wants the conditional histograms -- walks the staged
// order once, one u32 LDS atomic per (set condition, position).  A simulation that meets none of the group's conditions
// reads one u64 and touches no LDS.  At the end: one LDS atomic per thread and non-zero counter, then one u64 global
// atomic per non-zero cell of count [C] and cond_hist [C][n][n].  No cross-lane operation: a block of any size, down to
// one thread, computes the same.
//
// Overflow: a chunk is at most max_sims_per_launch() < 2^32 simulations and a cell receives at most one count per
// simulation, so no u32 counter can wrap.
#pragma once
#include "resume.hip.h"

namespace mcgp {

constexpr uint32_t kMaxConditions = 64;
constexpr uint32_t kMaxConditionAtoms = 8;
constexpr uint32_t kCondGroup = 8;               // conditions per counting block (blockIdx.y)
constexpr int kCondCountBlock = 256;             // threads of a counting block

// facts (MCGP_FACT_* of include/mcgp.h)
constexpr int32_t kFactPosition = 0, kFactGrid = 1, kFactRetiredLap = 2, kFactAheadBy = 3, kFactGained = 4,
                  kFactFinishers = 5, kFactRedFlags = 6, kFactSafetyCars = 7, kFactVscs = 8, kFactCount = 9;

// The condition table in device memory: mcgp_condition_atom / mcgp_condition of the C ABI, field for field.
struct CondAtom {
    int32_t fact, a, b, lo, hi, negate;
};
struct Cond {
    uint32_t n_atoms;
    CondAtom atom[kMaxConditionAtoms];
};

// The conditions kernel's per-lap observer: the race events of the laps run_laps runs.
struct EventCounter {
    uint32_t red, sc, vsc;
    __device__ __forceinline__ void operator()(const Rows &, int /*lap*/, int event)
    {
        red += event == kEventRed;
        sc += event == kEventSc;
        vsc += event == kEventVsc;
    }
};

// One lane's finished race against the table: `out` holds every driver's classified position (1 .. n).
__device__ __forceinline__ uint64_t evaluate_conditions(const Rows &s, const Cond *__restrict__ conds, uint32_t n_conditions,
                                                        int32_t finishers, const EventCounter &ev)
{
    uint64_t mask = 0ull;
    for (uint32_t c = 0; c < n_conditions; ++c) {
        const uint32_t n_atoms = conds[c].n_atoms;
        bool ok = true;
        for (uint32_t k = 0; k < n_atoms; ++k) {
            const CondAtom at = conds[c].atom[k];
            int32_t v;
            switch (at.fact) {
            case kFactPosition: v = (int32_t)s.Out((uint32_t)at.a); break;
            case kFactGrid: v = (int32_t)gpos_of(s.Pk((uint32_t)at.a)) + 1; break;
            case kFactRetiredLap: {
                const uint32_t pk = s.Pk((uint32_t)at.a);
                v = (pk & kDnf) ? (int32_t)(pk & kAgeMask) : 0;
                break;
            }
            case kFactAheadBy: v = (int32_t)s.Out((uint32_t)at.b) - (int32_t)s.Out((uint32_t)at.a); break;
            case kFactGained: v = (int32_t)gpos_of(s.Pk((uint32_t)at.a)) + 1 - (int32_t)s.Out((uint32_t)at.a); break;
            case kFactFinishers: v = finishers; break;
            case kFactRedFlags: v = (int32_t)ev.red; break;
            case kFactSafetyCars: v = (int32_t)ev.sc; break;
            default: v = (int32_t)ev.vsc; break;
            }
            ok &= (at.lo <= v && v <= at.hi) != (at.negate != 0);
        }
        mask |= (uint64_t)ok << c;
    }
    return mask;
}

// Simulations sim_offset + [0, m) (m <= the chunk the staging holds) from the grid (kFromState false) or from `state`,
// with race_kernel's block shape and LDS.  hist [n][n] is ACCUMULATED into; stage ([n][stride] bytes, then [stride] u64)
// is written.  conds [n_conditions].
template <bool kFromState>
__global__ void __launch_bounds__(512)
race_conditions_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ state, const Cond *__restrict__ conds,
                       uint32_t n_conditions, uint64_t m, uint64_t sim_offset, uint32_t seed_lo, uint32_t seed_hi,
                       unsigned long long *__restrict__ hist, uint8_t *__restrict__ stage, uint64_t stride,
                       uint32_t n_batches)
{
    run_observed<kFromState>(P, state, m, sim_offset, seed_lo, seed_hi, hist, n_batches,
        [](const Rows &, const LapEnv &, const RaceStart &, uint64_t) { return EventCounter{0u, 0u, 0u}; },
        [=](const Rows &s, const LapEnv &e, const EventCounter &ev, uint64_t local) {
            // the staged order, the inverse of `ord` and the finishers
            uint8_t *lane = stage + local;
            int32_t finishers = 0;
            for (int p = 0; p < e.n; ++p) {
                const uint32_t d = s.Ord(p);
                lane[(uint64_t)p * stride] = (uint8_t)d;
                s.Out(d) = (uint16_t)(p + 1);
                finishers += (s.Pk(d) & kDnf) ? 0 : 1;
            }
            reinterpret_cast<uint64_t *>(stage + (uint64_t)e.n * stride)[local] =
                evaluate_conditions(s, conds, n_conditions, finishers, ev);
        });
}

// The staged orders' and masks' counts of m simulations, added into count [C] and, unless NULL, cond_hist [C][n][n]
// ([condition][driver][position - 1] over the simulations that met it).  gridDim.y = the groups of kCondGroup conditions;
// the blocks of a group stride over the simulations.
__global__ void __launch_bounds__(kCondCountBlock)
conditions_count(const uint8_t *__restrict__ stage, uint64_t stride, uint64_t m, uint32_t n, uint32_t n_conditions,
                 unsigned long long *__restrict__ count, unsigned long long *__restrict__ cond_hist)
{
    __shared__ uint32_t cells[kCondGroup * kMaxCars * kMaxCars];      // [condition of the group][driver][position]
    __shared__ uint32_t met[kCondGroup];
    const uint32_t t = threadIdx.x, nt = blockDim.x;
    const uint32_t first = blockIdx.y * kCondGroup;
    const uint32_t G = n_conditions - first < kCondGroup ? n_conditions - first : kCondGroup;
    const uint32_t group_cells = G * n * n;
    if (cond_hist)
        for (uint32_t i = t; i < group_cells; i += nt) cells[i] = 0u;
    for (uint32_t g = t; g < kCondGroup; g += nt) met[g] = 0u;
    __syncthreads();

    const uint64_t *__restrict__ masks = reinterpret_cast<const uint64_t *>(stage + (uint64_t)n * stride);
    const uint32_t group_bits = G == kCondGroup ? 0xFFu : (1u << G) - 1u;
    uint32_t cnt[kCondGroup];
#pragma unroll
    for (uint32_t g = 0; g < kCondGroup; ++g) cnt[g] = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * nt + t; i < m; i += (uint64_t)gridDim.x * nt) {
        const uint32_t bits = (uint32_t)(masks[i] >> first) & group_bits;
#pragma unroll
        for (uint32_t g = 0; g < kCondGroup; ++g) cnt[g] += (bits >> g) & 1u;
        if (cond_hist && bits) {
            for (uint32_t p = 0; p < n; ++p) {
                const uint32_t d = stage[(uint64_t)p * stride + i];   // a driver index below n: the race kernel writes no other
                for (uint32_t b = bits; b; b &= b - 1u) {
                    const uint32_t g = (uint32_t)__ffs((int)b) - 1u;
                    atomicAdd(&cells[(g * n + d) * n + p], 1u);
                }
            }
        }
    }
#pragma unroll
    for (uint32_t g = 0; g < kCondGroup; ++g)
        if (cnt[g]) atomicAdd(&met[g], cnt[g]);
    __syncthreads();
    if (cond_hist) {
        unsigned long long *out = cond_hist + (uint64_t)first * n * n;
        for (uint32_t i = t; i < group_cells; i += nt) {
            const uint32_t c = cells[i];
            if (c) atomicAdd(&out[i], (unsigned long long)c);
        }
    }
    for (uint32_t g = t; g < G; g += nt) {
        const uint32_t c = met[g];
        if (c) atomicAdd(&count[first + g], (unsigned long long)c);
    }
}

}  // namespace mcgp
