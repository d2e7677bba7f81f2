// resume.hip.h -- the rest of a race from a mid-race state (mcgp_run_from_state, include/mcgp.h).
//
// A state is the race after lap k as race_kernel leaves it (update_positions of that lap done): per car its cumulative
// and last lap time, grid slot, compound, tyre age, compounds used and retirement lap, and the race's
// drs_disabled_until.  race_resume_kernel runs laps k + 1 .. L of it with race_kernel's own lap code (run_laps) and
// classification (classify_and_count), simulation id i drawing exactly what race_kernel's simulation i draws on those
// laps.  So a state that race_kernel itself produced for simulation i continues, as simulation i, bit for bit into the
// finishing order of the full race.
//
// Layout: one lane runs one (state, simulation) pair in race_kernel's LDS rows (Rows: cum, last, pk, ord, out).  A block
// serves one state (blockIdx.y) and grid-strides over its simulations in batches of blockDim.x (blockIdx.x); its counts
// go to the block's u32 LDS histogram and then, with u64 atomics, to hist[state][n][n].  The state is read from device
// memory (ResumeState, uploaded per call), the same addresses for every lane of the block.
//
// Per lane: the rows are loaded in driver order, `ord` is sorted by (cumulative time, grid slot) over all cars, and the
// DRS and dirty-air flags come from update_positions(k, k > 2 && k > drs_disabled_until) -- what race_kernel computes
// at the end of lap k.  Retirements: a running car keeps race_kernel's once-per-race lap L_d if it is 0 or after k; a
// draw of lap 2 .. k contradicts the state (the car runs) and is replaced by draw_retirement_lap_after
// (race_common.hip.h).  Overflow: the host splits a state's simulations at max_sims_per_launch() (< 2^32 per launch),
// so no u32 block count can wrap.
#pragma once
#include "race_kernel.hip.h"

namespace mcgp {

constexpr uint32_t kMaxResumeStates = 4096;

// One race state in device memory, in race_kernel's encoding; arrays in driver-index order.
struct ResumeState {
    double cum[kMaxCars];
    double last[kMaxCars];
    uint32_t pk[kMaxCars];      // tyre age (the retirement lap once kDnf is set) | compound | compounds used | grid slot | kDnf
    uint64_t sim_offset;        // first simulation id of this state
    int32_t lap;                // laps completed, 1 .. L
    int32_t drs_disabled_until;
};

// The start of one lane's race from a mid-race state: the rows, the field order, the DRS and dirty-air flags after lap
// st.lap, and the retirement laps after it.
__device__ __forceinline__ RaceStart start_from_state(const Rows &s, const LapEnv &e, const ResumeState &st, uint32_t c0,
                                                      uint32_t c1, uint32_t seed_lo, uint32_t seed_hi)
{
    const int n = e.n, L = e.L;
    const int k = st.lap;
    const int drs_disabled_until = st.drs_disabled_until;

    // ================= the state after lap k, as race_kernel leaves it =================
    for (int d = 0; d < n; ++d) {
        s.Cum(d) = st.cum[d];
        s.Last(d) = st.last[d];
        s.Pk(d) = st.pk[d];
        s.Ord(d) = (uint8_t)d;
    }
    sort_by_time(s, n);
    update_positions(s, n, k > 2 && k > drs_disabled_until, e.dirty_thr);

    // ================= retirements after lap k: race_kernel's draw, redrawn where the state contradicts it =================
    {
        uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
        for (int d = 0; d < n; ++d) {
            if ((d & 3) == 0)
                philox4x32_10(c0, c1, 0u, kPurposeRetire | (uint32_t)(d >> 2), seed_lo, seed_hi, r0, r1, r2, r3);
            const uint32_t rw = (d & 3) == 0 ? r0 : (d & 3) == 1 ? r1 : (d & 3) == 2 ? r2 : r3;
            uint32_t out = draw_retirement_lap(rw, e.dnf[d], L);
            if (out != 0u && (int)out <= k && !(s.Pk(d) & kDnf)) {
                uint32_t v0, v1, v2, v3;
                philox4x32_10(c0, c1, 0u, kPurposeRetire | (8u + (uint32_t)(d >> 2)), seed_lo, seed_hi, v0, v1, v2, v3);
                const uint32_t vw = (d & 3) == 0 ? v0 : (d & 3) == 1 ? v1 : (d & 3) == 2 ? v2 : v3;
                out = draw_retirement_lap_after(vw, e.dnf[d], k, L);
            }
            s.Out(d) = (uint16_t)out;
        }
    }
    return {k + 1, drs_disabled_until};
}

// One lane's body of the analysis kernels (trace, gaps, conditions, stints, moves): the unmodified race of simulation
// sim_offset + local, from the grid (kFromState false; `state` is not read and may be NULL) or from `state`, watched by
// a per-lap observer.  begin(s, e, at, local) builds the observer once the start has run (and records what the start
// itself left, where the kernel stages that); run_laps hands it every lap; end(s, e, obs, local) runs over the
// classified order.  m, hist and n_batches are run_block's.
template <bool kFromState, class Begin, class End>
__device__ __forceinline__ void run_observed(const KParams *__restrict__ P, const ResumeState *__restrict__ state, uint64_t m,
                                             uint64_t sim_offset, uint32_t seed_lo, uint32_t seed_hi,
                                             unsigned long long *__restrict__ hist, uint32_t n_batches, Begin begin, End end)
{
    run_block(P, m, n_batches, hist, [=](const Rows &s, const LapEnv &e, uint32_t *s_hist, uint64_t local) {
        const uint64_t sim = sim_offset + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);
        const RaceStart at = kFromState ? start_from_state(s, e, *state, c0, c1, seed_lo, seed_hi)
                                        : start_from_grid(s, e, c0, c1, seed_lo, seed_hi, nullptr);
        auto obs = begin(s, e, at, local);
        run_laps(s, e, c0, c1, seed_lo, seed_hi, at.first_lap, at.drs_disabled_until, obs);         // reference :166-228
        classify_and_count(s, e.n, s_hist, nullptr);                                                // reference :230-242
        end(s, e, obs, local);
    });
}

// n_sims simulations per state, ids states[s].sim_offset + sim_base + [0, n_sims); gridDim.y = number of states.
// hist [states][n][n] is ACCUMULATED into; orders (NULL: none) = [states][n_sims][n].
__global__ void __launch_bounds__(512)
race_resume_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ states, uint64_t n_sims,
                   uint64_t sim_base, uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist,
                   uint8_t *__restrict__ orders, uint32_t n_batches)
{
    const uint32_t si = blockIdx.y;
    const ResumeState *__restrict__ st = states + si;
    run_block(P, n_sims, n_batches, hist + (size_t)si * (size_t)(P->n * P->n),
              [=](const Rows &s, const LapEnv &e, uint32_t *s_hist, uint64_t local) {
        const uint64_t sim = st->sim_offset + sim_base + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);
        const RaceStart at = start_from_state(s, e, *st, c0, c1, seed_lo, seed_hi);
        NoLapObserver none;
        run_laps(s, e, c0, c1, seed_lo, seed_hi, at.first_lap, at.drs_disabled_until, none);        // reference :166-228
        classify_and_count(s, e.n, s_hist,                                                          // reference :230-242
                           orders ? orders + ((uint64_t)si * n_sims + local) * (uint64_t)e.n : nullptr);
    });
}

}  // namespace mcgp
