// champ_bonus.hip.h -- the fastest-lap bonus of a championship race added to the standing keys (championship.hip.h) and
// counted (mcgp_run_championship_bonus, include/mcgp.h).
//
// race_fastest_kernel (fastest.hip.h) leaves two bytes per simulation of a chunk: the fastest-lap driver and that
// driver's classified position (0-based), 0xFF each when the race has no fastest lap.  champ_bonus runs after the race's
// champ_accumulate (which starts the keys on a chunk's first race) and before champ_round: a thread per simulation,
// grid-striding over tiles of 256, reads the two bytes, counts the fastest lap, and where the position is inside the
// race's limit adds the bonus to the points field of that driver's key (a multi-word add with carry, like
// champ_accumulate's) and counts the bonus.  The bonus touches the points field only, never a countback count; team keys
// are built from the driver keys afterwards, so team points include it.  Counts go to two u32 LDS histograms (a block
// sees at most one chunk, 2^22 simulations) that are flushed with one u64 global atomic per non-zero cell.
#pragma once
#include "championship.hip.h"

namespace mcgp {

// The key increment of a race's bonus: its points at the points field (bit kChampCountBits n), in the words of a
// driver key (at most 3), built by the host with champ_piece.
struct ChampBonusAdd {
    uint64_t w[3];
};

// One bonus race of a chunk, after its champ_accumulate.  fl_driver, fl_pos: race_fastest_kernel's [m] bytes; keys:
// [words][n][stride]; add: the bonus' key increment; within: classified positions (1-based) that take the bonus.
// fastest [n] and bonus [n] are this race's rows and are ACCUMULATED into.
__global__ void __launch_bounds__(kChampAccBlock)
champ_bonus(const uint8_t *__restrict__ fl_driver, const uint8_t *__restrict__ fl_pos, uint64_t m, uint32_t n,
            uint32_t words, uint64_t stride, uint64_t *__restrict__ keys, ChampBonusAdd add, uint32_t within,
            unsigned long long *__restrict__ fastest, unsigned long long *__restrict__ bonus)
{
    __shared__ uint32_t s_fast[kMaxCars], s_bonus[kMaxCars];
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)kMaxCars) s_fast[t] = s_bonus[t] = 0u;
    __syncthreads();
    for (uint64_t s = (uint64_t)blockIdx.x * kChampAccBlock + t; s < m; s += (uint64_t)gridDim.x * kChampAccBlock) {
        const uint32_t d = fl_driver[s];
        if (d >= n) continue;                               // no fastest lap
        atomicAdd(&s_fast[d], 1u);
        if ((uint32_t)fl_pos[s] >= within) continue;
        uint64_t carry = 0;
#pragma unroll
        for (uint32_t w = 0; w < 3; ++w) {                  // (unrolled: add.w stays in the kernel's arguments)
            if (w >= words) break;
            uint64_t *k = keys + ((uint64_t)w * n + d) * stride + s;
            const uint64_t base = *k;
            const uint64_t x = base + add.w[w];
            const uint64_t y = x + carry;
            carry = (uint64_t)(x < base) | (uint64_t)(y < x);
            *k = y;
        }
        atomicAdd(&s_bonus[d], 1u);
    }
    __syncthreads();
    if (t < n) {
        if (s_fast[t]) atomicAdd(&fastest[t], (unsigned long long)s_fast[t]);
        if (s_bonus[t]) atomicAdd(&bonus[t], (unsigned long long)s_bonus[t]);
    }
}

}  // namespace mcgp
