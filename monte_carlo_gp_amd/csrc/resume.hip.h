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

// n_sims simulations per state, ids states[s].sim_offset + sim_base + [0, n_sims); gridDim.y = number of states.
// hist [states][n][n] is ACCUMULATED into; orders (NULL: none) = [states][n_sims][n].
__global__ void __launch_bounds__(512)
race_resume_kernel(const KParams *__restrict__ P, const ResumeState *__restrict__ states, uint64_t n_sims,
                   uint64_t sim_base, uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist,
                   uint8_t *__restrict__ orders, uint32_t n_batches)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int B = blockDim.x;
    uint32_t *s_hist;
    Rows s;
    const LapEnv e = load_block(smem, P, s_hist, s);
    __syncthreads();
    const int n = e.n;
    const int L = e.L;
    const ResumeState &st = states[blockIdx.y];
    const int k = st.lap;
    const int drs_disabled_until = st.drs_disabled_until;

    for (uint32_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
        const uint64_t local = (uint64_t)batch * (uint64_t)B + (uint64_t)tid;
        if (local >= n_sims) continue;      // tail lanes idle; no barrier inside the loop
        const uint64_t sim = st.sim_offset + sim_base + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);

#include "resume_start.inc.h"

        // ================= laps k+1..L, reference :166-228 =================
        NoLapObserver none;
        run_laps(s, e, c0, c1, seed_lo, seed_hi, k + 1, drs_disabled_until, none);

        // ================= classification, reference :230-242 =================
        classify_and_count(s, n, s_hist,
                           orders ? orders + ((uint64_t)blockIdx.y * n_sims + local) * (uint64_t)n : nullptr);
    }

    __syncthreads();
    unsigned long long *h = hist + (size_t)blockIdx.y * (size_t)(n * n);
    for (int i = tid; i < n * n; i += B) {
        const uint32_t c = s_hist[i];
        if (c) atomicAdd(&h[i], (unsigned long long)c);
    }
}

}  // namespace mcgp
