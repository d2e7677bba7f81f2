// fastest.hip.h -- the fastest-lap bonus point of a championship race, scored and counted on the device
// (mcgp_run_championship_bonus, include/mcgp.h).
//
// The 2019-2024 rule gives a point to the driver who sets the race's fastest lap, if classified in the top ten.  The
// register kernels keep no lap time, so a race WITH a bonus runs on race_fastest_kernel: the generic kernel's code --
// start_from_grid, run_laps, classify_and_count -- with a per-lap observer (FastestObserver) that keeps the fastest lap
// so far and its driver, by race_trace_kernel's definition (trace.hip.h): the smallest Last(d) of a car running after lap
// k, over laps 2..L; strict <, laps in order, cars in `ord` order, so a tie goes to the earlier lap, then to the better
// running position; a race in which no car completes a lap >= 2 (every race of one lap) has none.  Simulation i draws
// exactly what race_kernel's simulation i draws, so its finishing order and position histogram are mcgp_run's.
//
// Price: the generic kernel, about 52 ms per 10^6 simulations of a 20-car, 60-lap race on an MI355X against 6.7 ms on
// the register kernel.  A race without a bonus keeps mcgp_run's launch path.
//
// Per simulation the kernel writes the finishing order ([sim][n] bytes, the staging champ_accumulate reads) and two
// bytes, in two rows of the chunk's capacity so that a wave's lanes write adjacent bytes:
//
//     fl_driver[sim]   the fastest-lap driver, kNoFastestByte for none
//     fl_pos[sim]      that driver's classified position (0-based), kNoFastestByte for none
//
// champ_bonus (champ_bonus.hip.h) reads the two rows behind the race's champ_accumulate.
#pragma once
#include "race_kernel.hip.h"

namespace mcgp {

constexpr uint32_t kNoFastestByte = 0xFFu;      // fl_driver / fl_pos: no car completed a lap >= 2

// The per-lap observer of race_fastest_kernel: the fastest lap so far and its driver.  run_laps calls it for laps >= 2
// only (a race from the grid starts run_laps at lap 2; lap 1 records no lap time).
struct FastestObserver {
    int n;
    double best;
    uint32_t best_d;

    __device__ __forceinline__ void operator()(const Rows &s, int /*lap*/, int /*event*/)
    {
        for (int i = 0; i < n; ++i) {
            const uint32_t d = s.Ord(i);
            if (s.Pk(d) & kDnf) continue;
            const double t = s.Last(d);
            if (t < best) { best = t; best_d = d; }
        }
    }
};

// mcgp_run's simulations sim_offset + [0, n_sims) (n_sims <= the chunk the staging holds), with race_kernel's block
// shape and LDS.  hist [n][n] is ACCUMULATED into; orders [n_sims][n], fl_driver [n_sims] and fl_pos [n_sims] are written.
__global__ void __launch_bounds__(512)
race_fastest_kernel(const KParams *__restrict__ P, uint64_t n_sims, uint64_t sim_offset, uint32_t seed_lo,
                    uint32_t seed_hi, unsigned long long *__restrict__ hist, uint8_t *__restrict__ orders,
                    uint8_t *__restrict__ fl_driver, uint8_t *__restrict__ fl_pos, uint32_t n_batches)
{
    run_block(P, n_sims, n_batches, hist, [=](const Rows &s, const LapEnv &e, uint32_t *s_hist, uint64_t local) {
        const uint64_t sim = sim_offset + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);
        const RaceStart at = start_from_grid(s, e, c0, c1, seed_lo, seed_hi, nullptr);

        FastestObserver obs;
        obs.n = e.n;
        obs.best = __builtin_inf();
        obs.best_d = kNoFastestByte;

        run_laps(s, e, c0, c1, seed_lo, seed_hi, at.first_lap, at.drs_disabled_until, obs);         // reference :166-228
        classify_and_count(s, e.n, s_hist, orders + local * (uint64_t)e.n);                         // reference :230-242
        // `ord` now holds the classification: the fastest-lap driver's place in it
        uint32_t pos = kNoFastestByte;
        for (int p = 0; p < e.n; ++p)
            if ((uint32_t)s.Ord(p) == obs.best_d) pos = (uint32_t)p;
        fl_driver[local] = (uint8_t)obs.best_d;
        fl_pos[local] = (uint8_t)pos;
    });
}

}  // namespace mcgp
