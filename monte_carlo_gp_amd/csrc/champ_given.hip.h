// champ_given.hip.h -- title odds by finishing position (mcgp_run_championship_live, include/mcgp.h).
//
// After champ_rank of a chunk, champ_given reads the chunk's final standing keys and the finishing orders of ONE race of
// the call (the "given" race, kept in a staging buffer of its own until the end of the chunk) and counts the joint table
//
//     given[d][p][e] += 1   when driver d is classified p + 1-th in the given race and driver e is champion
//
// Layout: one simulation per lane, a block of kChampGivenBlock threads over tiles of as many simulations, grid-striding
// over the chunk.
//
//   Champion.  A running maximum over the n keys.  The keys are [word][driver][sim] (championship.hip.h), so the 64
//   lanes of a wave load consecutive u64 for every (word, driver): each key word is read exactly once, straight from
//   global memory into registers (no LDS staging: nothing is read twice).  The order is champ_cmp's, most significant
//   word first, and the running key is replaced only on a strict "greater", so that of fully tied keys the lowest driver
//   index stays -- champ_rank's rule for position 0.
//
//   Orders.  [sim][n] bytes.  The tile goes through LDS in whole words plus the tail's bytes, as champ_accumulate's does:
//   a tile starts at simulation s0, a multiple of kChampGivenBlock = 256, so s0 * n is a multiple of 4 and the buffer is
//   allocation-aligned.  A lane then reads its own n bytes.
//
//   Histogram.  A per-block u32 table in LDS, flushed with global u64 atomics at the end, when the table fits the
//   launch's LDS budget next to the tile (the host decides: champ_given_lds); else every count is a global u64 atomic.
//   A block's u32 cell takes at most one count per simulation and a launch has at most 2^22 simulations (the host's
//   chunk), so it cannot wrap.
//
//   LDS layout of the table.  In one step of p the 64 atomics of a wave share p, mostly share e (the champion is the
//   same driver in most simulations) and differ in d.  In the output's layout (d n + p) n + e two lanes would differ by
//   multiples of n^2 words: at 20 cars 400 = 16 (mod 64), so with 64 banks of 4 bytes the whole wave would fall on four
//   banks.  The LDS copy is therefore kept [e][p][d], d fastest -- the distinct d of a step are then distinct banks
//   (n <= 32) -- and transposed on the flush.  This rests on the documented bank count, not on a measurement.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "championship.hip.h"

namespace mcgp {

constexpr int kChampGivenBlock = 256;       // 256 n is a multiple of 4 for every n: a tile's orders start on a word
constexpr int kChampGivenWords = 3;         // driver keys: 16 + 5 n bits, at most 3 words at 32 cars
static_assert(kChampPointsBits + kChampCountBits * kMaxCars <= 64 * kChampGivenWords, "a driver key has at most 3 words");

// LDS of champ_given: the tile's orders, kChampGivenBlock x n bytes (padded to 16) | table [e][p][d] u32 (only when
// counted in LDS)
struct ChampGivenLds {
    uint32_t o_table, bytes;
};
__host__ __device__ inline ChampGivenLds champ_given_lds(uint32_t n, bool table_in_lds)
{
    ChampGivenLds L;
    L.o_table = ((uint32_t)kChampGivenBlock * n + 15) / 16 * 16;
    L.bytes = L.o_table + (table_in_lds ? n * n * n * 4 : 0);
    return L;
}

// keys: [words][n][stride] after the last race (and bonus) of the chunk; orders: the given race's [m][n] u8,
// allocation-aligned; m <= 2^22.  The dynamic LDS is champ_given_lds(n, table_in_lds != 0).  given [n][n][n]
// ([driver][position][champion]) is ACCUMULATED into.
__global__ void __launch_bounds__(kChampGivenBlock)
champ_given(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ orders, uint64_t m, uint64_t stride, uint32_t n,
            uint32_t words, uint32_t table_in_lds, unsigned long long *__restrict__ given)
{
    HIP_DYNAMIC_SHARED(__align__(16) unsigned char, smem)
    const ChampGivenLds L = champ_given_lds(n, table_in_lds != 0);
    uint32_t *s_ord = reinterpret_cast<uint32_t *>(smem);
    const uint8_t *s_ordb = smem;
    uint32_t *s_tab = reinterpret_cast<uint32_t *>(smem + L.o_table);
    const uint32_t t = threadIdx.x, cells = n * n * n;
    if (table_in_lds)
        for (uint32_t i = t; i < cells; i += kChampGivenBlock) s_tab[i] = 0;
    for (uint64_t s0 = (uint64_t)blockIdx.x * kChampGivenBlock; s0 < m; s0 += (uint64_t)gridDim.x * kChampGivenBlock) {
        const uint32_t cnt = (m - s0) < (uint64_t)kChampGivenBlock ? (uint32_t)(m - s0) : (uint32_t)kChampGivenBlock;
        const uint32_t bytes = cnt * n;
        // s0 * n is a multiple of 256 and the buffer is allocation-aligned: whole words, then the tail's bytes
        const uint8_t *src = orders + s0 * n;
        const uint32_t n4 = bytes >> 2;
        for (uint32_t i = t; i < n4; i += kChampGivenBlock) s_ord[i] = reinterpret_cast<const uint32_t *>(src)[i];
        if (t < (bytes & 3u)) smem[n4 * 4 + t] = src[n4 * 4 + t];
        // the champion of this lane's simulation, while the tile's loads are under way
        uint32_t e = 0;
        if (t < cnt) {
            const uint64_t *k = keys + s0 + t;
            uint64_t best[kChampGivenWords] = {0, 0, 0};
#pragma unroll
            for (int w = 0; w < kChampGivenWords; ++w)
                if ((uint32_t)w < words) best[w] = k[(uint64_t)w * n * stride];
            for (uint32_t d = 1; d < n; ++d) {
                uint64_t cur[kChampGivenWords] = {0, 0, 0};
#pragma unroll
                for (int w = 0; w < kChampGivenWords; ++w)
                    if ((uint32_t)w < words) cur[w] = k[((uint64_t)w * n + d) * stride];
                const bool greater = cur[2] != best[2] ? cur[2] > best[2]
                                   : cur[1] != best[1] ? cur[1] > best[1]
                                                       : cur[0] > best[0];
                if (greater) {
#pragma unroll
                    for (int w = 0; w < kChampGivenWords; ++w) best[w] = cur[w];
                    e = d;
                }
            }
        }
        __syncthreads();
        if (t < cnt) {
            const uint8_t *o = s_ordb + t * n;
            for (uint32_t p = 0; p < n; ++p) {
                const uint32_t d = o[p];
                if (d >= n) continue;                       // (no race kernel writes one; keeps the cell inside the table)
                if (table_in_lds) atomicAdd(&s_tab[(e * n + p) * n + d], 1u);
                else atomicAdd(&given[((uint64_t)d * n + p) * n + e], 1ull);
            }
        }
        __syncthreads();
    }
    if (table_in_lds) {
        __syncthreads();
        for (uint32_t i = t; i < cells; i += kChampGivenBlock) {
            const uint32_t c = s_tab[i];
            if (!c) continue;
            const uint32_t d = i % n, ep = i / n, p = ep % n, e = ep / n;
            atomicAdd(&given[((uint64_t)d * n + p) * n + e], (unsigned long long)c);
        }
    }
}

}  // namespace mcgp
