// matchups.hip.h -- head-to-head and podium-combination counts of one race on the device (mcgp_run_matchups,
// include/mcgp.h).
//
// The race kernels stage a chunk of finishing orders ([sim][n] u8, driver classified p-th) and count the position
// histogram themselves; race_matchups then reads the chunk once and counts, per simulation,
//
//   ahead[i][j]    += 1 when driver i is classified ahead of driver j
//   podium[a][b][c] += 1 when the first three classified cars are a, b, c in that order (optional)
//
// Layout: one simulation per lane; a block of `block` threads (256, or 128 / 64 when LDS requires it) takes tiles of
// `block` simulations, grid-striding over the chunk.  The tile's orders are copied into LDS in whole words.  Each lane
// walks its order from the back and stores, for every driver d, the 32-bit mask of the drivers classified behind d in
// LDS as [driver][lane] (a mask array indexed at run time in registers would go to scratch).  Then, for each driver i,
// the wave counts bit j of the 64 lanes' masks with one 64-bit ballot and a popcount per j; lane j collects count j and
// adds it to the block's u32 [n][n] table with one LDS atomic per i.  The podium cell (o0 n + o1) n + o2 goes to a u32
// [n][n][n] LDS table when it fits the block's LDS budget, else straight to the u64 output with a global atomic.  At the
// end a block adds its non-zero cells to the u64 outputs with global atomics.
//
// Overflow: a u32 cell of a block receives at most one count per simulation the block takes, and one launch takes at
// most kMatchMaxSims = 2^22 simulations (the host's chunk), so no block counter can wrap.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "race_common.hip.h"

namespace mcgp {

constexpr uint32_t kMatchMaxSims = 1u << 22;       // most simulations of one race_matchups launch (u32 block counters)
constexpr int kMatchMaxBlock = 256;

// podium counting modes of race_matchups
constexpr uint32_t kPodiumNone = 0, kPodiumLds = 1, kPodiumGlobal = 2;

// LDS of race_matchups for a block of `block` threads: orders block x n bytes (padded to 16) | masks [n][block] u32 |
// ahead [n][n] u32 | podium [n][n][n] u32 (only when counted in LDS)
struct MatchLds {
    uint32_t o_mask, o_ahead, o_podium, bytes;
};
__host__ __device__ inline MatchLds match_lds(uint32_t n, uint32_t block, bool podium_in_lds)
{
    MatchLds L;
    L.o_mask = (block * n + 15) / 16 * 16;
    L.o_ahead = L.o_mask + n * block * 4;
    L.o_podium = L.o_ahead + n * n * 4;
    L.bytes = L.o_podium + (podium_in_lds ? n * n * n * 4 : 0);
    return L;
}

// orders: the race kernel's [m][n] u8 for m <= kMatchMaxSims simulations, allocation-aligned.  blockDim.x is a
// multiple of 64 and at most kMatchMaxBlock; the dynamic LDS is match_lds(n, blockDim.x, podium_mode == kPodiumLds).
// ahead [n][n] and podium [n][n][n] (read only when podium_mode != kPodiumNone) are ACCUMULATED into.
__global__ void __launch_bounds__(kMatchMaxBlock)
race_matchups(const uint8_t *__restrict__ orders, uint64_t m, uint32_t n, uint32_t podium_mode,
              unsigned long long *__restrict__ ahead, unsigned long long *__restrict__ podium)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t block = blockDim.x, t = threadIdx.x, lane = t & 63;
    const MatchLds L = match_lds(n, block, podium_mode == kPodiumLds);
    uint8_t *s_ord = smem;
    uint32_t *s_mask = reinterpret_cast<uint32_t *>(smem + L.o_mask);
    uint32_t *s_ahead = reinterpret_cast<uint32_t *>(smem + L.o_ahead);
    uint32_t *s_pod = reinterpret_cast<uint32_t *>(smem + L.o_podium);
    const uint32_t table_words = (L.bytes - L.o_ahead) / 4;         // ahead, then podium when it is in LDS
    for (uint32_t i = t; i < table_words; i += block) s_ahead[i] = 0;
    const uint32_t cells = n * n * n;
    for (uint64_t s0 = (uint64_t)blockIdx.x * block; s0 < m; s0 += (uint64_t)gridDim.x * block) {
        const uint32_t cnt = (m - s0) < (uint64_t)block ? (uint32_t)(m - s0) : block;
        const uint32_t bytes = cnt * n;
        // s0 * n is a multiple of 64 and the buffer is allocation-aligned: whole words, then the tail's bytes
        const uint8_t *src = orders + s0 * n;
        const uint32_t n4 = bytes >> 2;
        for (uint32_t i = t; i < n4; i += block)
            reinterpret_cast<uint32_t *>(s_ord)[i] = reinterpret_cast<const uint32_t *>(src)[i];
        if (t < (bytes & 3u)) s_ord[n4 * 4 + t] = src[n4 * 4 + t];
        __syncthreads();
        // masks of the drivers behind each driver; a tail lane's are 0, so it counts nothing below
        if (t < cnt) {
            const uint8_t *o = s_ord + t * n;
            uint32_t behind = 0;
            for (int p = (int)n - 1; p >= 0; --p) {
                const uint32_t d = o[p] & (kMaxCars - 1);
                s_mask[d * block + t] = behind;
                behind |= 1u << d;
            }
            if (podium_mode != kPodiumNone) {
                const uint32_t cell = ((uint32_t)o[0] * n + o[1]) * n + o[2];
                if (cell < cells) {
                    if (podium_mode == kPodiumLds) atomicAdd(&s_pod[cell], 1u);
                    else atomicAdd(&podium[cell], 1ull);
                }
            }
        } else {
            for (uint32_t d = 0; d < n; ++d) s_mask[d * block + t] = 0;
        }
        // (each lane reads back only its own masks: no barrier)  Pairs: every lane of the wave is active here.  j goes in
        // fours, four independent ballots in flight (j stays below 32 as n <= 32; bits at or above n are 0, so those
        // counts are 0 and their lanes add nothing)
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t mi = s_mask[i * block + t];
            uint32_t mine = 0;
            for (uint32_t j0 = 0; j0 < n; j0 += 4) {
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t j = j0 + k;
                    const uint32_t c = (uint32_t)__popcll(__ballot((mi >> j) & 1u));
                    mine = lane == j ? c : mine;
                }
            }
            if (lane < n && mine) atomicAdd(&s_ahead[i * n + lane], mine);
        }
        __syncthreads();
    }
    __syncthreads();
    for (uint32_t i = t; i < n * n; i += block)
        if (s_ahead[i]) atomicAdd(&ahead[i], (unsigned long long)s_ahead[i]);
    if (podium_mode == kPodiumLds)
        for (uint32_t i = t; i < cells; i += block)
            if (s_pod[i]) atomicAdd(&podium[i], (unsigned long long)s_pod[i]);
}

}  // namespace mcgp
