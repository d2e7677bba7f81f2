// championship.hip.h -- season standings on the device (mcgp_run_championship, include/mcgp.h).
//
// A championship is R races run on the same simulation ids: simulation s of the season is the tuple of the R finishing
// orders mcgp_run gives each race alone for id s.  The standing of a driver is ONE unsigned integer key, a big number
// of `words` u64 words (word 0 least significant):
//
//     key = points << (n * cbits)  +  sum over p of count(position p + 1) << ((n - 1 - p) * cbits)
//
// so that "more points, then more wins, then more seconds, ..." is exactly "larger key".  Every field is wide enough
// never to carry under the call's limits (drivers: cbits = 5, points 16 bits; teams: widths the host derives from the
// call's inputs), so accumulating a race is a plain multi-word add and ranking is an integer compare.
//
//   champ_accumulate  after each race of a chunk: reads the race kernel's orders ([sim][n] u8) and adds every driver's
//                     points and countback unit to its key.  Keys are laid out [word][driver][sim] (sim stride =
//                     the chunk capacity), so a wave's lanes touch consecutive simulations.  The first race of a chunk
//                     starts from the initial standings' keys instead of reading the buffer.
//   champ_rank        after the last race of a chunk: per simulation, the n drivers' and T teams' positions by O(n^2)
//                     compares (a full tie goes to the lower index) and every driver's points gained; counts go to
//                     per-block LDS u32 histograms that are flushed into the u64 outputs with global atomics (the
//                     gain histogram goes straight to global atomics when it does not fit the block's LDS budget).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "race_common.hip.h"

namespace mcgp {

constexpr int kChampCountBits = 5;          // driver keys: countback count per position <= 31
constexpr int kChampPointsBits = 16;        // driver keys: total points <= 65 535
constexpr int kChampMaxRaces = 64;
constexpr int kChampMaxTeamWords = 6;       // team keys at the widest (32 drivers in one team: 10-bit counts, 21-bit points)
constexpr int kChampAccBlock = 256;         // champ_accumulate: one simulation per thread
constexpr int kChampRankBlock = 256;        // champ_rank: 4 waves over a tile of 64 simulations (one per lane)
constexpr int kChampTile = 64;

// bits [off, off + width) of a field of value v, as they fall into word w of a key (v < 2^32, width <= 32)
__host__ __device__ inline uint64_t champ_piece(uint64_t v, int off, int w)
{
    const int s = off - 64 * w;
    if (s >= 64 || s <= -64) return 0;
    return s >= 0 ? v << s : v >> (-s);
}

// field [off, off + bits) of a key whose word i is at k[i * wstride]
__device__ inline uint32_t champ_field(const uint64_t *k, uint32_t wstride, uint32_t words, uint32_t off, uint32_t bits)
{
    const uint32_t w = off >> 6, b = off & 63;
    uint64_t x = k[w * wstride] >> b;
    if (b + bits > 64 && w + 1 < words) x |= k[(w + 1) * wstride] << (64 - b);
    return (uint32_t)(x & ((1ull << bits) - 1));
}

// >0, 0, <0 as key a is greater than, equal to, less than key b (both with word stride wstride)
__device__ inline int champ_cmp(const uint64_t *a, const uint64_t *b, uint32_t wstride, uint32_t words)
{
    for (int w = (int)words - 1; w >= 0; --w) {
        const uint64_t x = a[w * wstride], y = b[w * wstride];
        if (x != y) return x > y ? 1 : -1;
    }
    return 0;
}

// LDS of champ_rank: [driver keys: words][n][64] u64 | [team keys: team_words][T][64] u64 | champ n x n u32 |
// team T x T u32 | gain n x gain_cols u32 (only when gain_in_lds)
struct ChampRankLds {
    uint32_t o_tk, o_champ, o_team, o_gain, bytes;
};
__host__ __device__ inline ChampRankLds champ_rank_lds(uint32_t n, uint32_t words, uint32_t n_teams, uint32_t team_words,
                                                      uint32_t gain_cols, bool gain_in_lds)
{
    ChampRankLds L;
    L.o_tk = words * n * kChampTile * 8;
    L.o_champ = L.o_tk + team_words * n_teams * kChampTile * 8;
    L.o_team = L.o_champ + n * n * 4;
    L.o_gain = L.o_team + n_teams * n_teams * 4;
    L.bytes = L.o_gain + (gain_in_lds ? n * gain_cols * 4 : 0);
    L.bytes = (L.bytes + 15) / 16 * 16;
    return L;
}

// One race of a chunk.  orders: the race kernel's [m][n] u8 (driver classified p-th); keys: [words][n][stride];
// add: [n][words] the key increment of position p (its points at the points field, plus one unit of its count field for
// a countback race) -- the same for every simulation, built by the host; init: [words][n] initial keys, read instead
// of `keys` when `first` is set.
__global__ void __launch_bounds__(kChampAccBlock)
champ_accumulate(const uint8_t *__restrict__ orders, uint64_t m, uint32_t n, uint32_t words, uint64_t stride,
                 uint64_t *__restrict__ keys, const uint64_t *__restrict__ add, const uint64_t *__restrict__ init,
                 uint32_t first)
{
    __shared__ uint32_t s_ord[kChampAccBlock * kMaxCars / 4];     // the tile's orders, [sim][n] bytes
    __shared__ uint8_t s_pos[kMaxCars][kChampAccBlock];          // position of driver d in the tile's simulation t
    __shared__ uint64_t s_add[kMaxCars * 3];                     // driver keys have at most 3 words
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < n * words; i += kChampAccBlock) s_add[i] = add[i];
    const uint8_t *s_ordb = reinterpret_cast<const uint8_t *>(s_ord);
    for (uint64_t s0 = (uint64_t)blockIdx.x * kChampAccBlock; s0 < m; s0 += (uint64_t)gridDim.x * kChampAccBlock) {
        const uint32_t cnt = (m - s0) < (uint64_t)kChampAccBlock ? (uint32_t)(m - s0) : (uint32_t)kChampAccBlock;
        const uint32_t bytes = cnt * n;
        // s0 * n is a multiple of 256 and the buffer is allocation-aligned: whole words, then the tail's bytes
        const uint8_t *src = orders + s0 * n;
        const uint32_t n4 = bytes >> 2;
        for (uint32_t i = t; i < n4; i += kChampAccBlock) s_ord[i] = reinterpret_cast<const uint32_t *>(src)[i];
        if (t < (bytes & 3u)) reinterpret_cast<uint8_t *>(s_ord)[n4 * 4 + t] = src[n4 * 4 + t];
        __syncthreads();
        if (t < cnt)
            for (uint32_t p = 0; p < n; ++p) s_pos[s_ordb[t * n + p] & (kMaxCars - 1)][t] = (uint8_t)p;
        __syncthreads();
        if (t < cnt) {
            const uint64_t s = s0 + t;
            for (uint32_t d = 0; d < n; ++d) {
                const uint32_t p = s_pos[d][t];
                uint64_t carry = 0;
                for (uint32_t w = 0; w < words; ++w) {
                    uint64_t *k = keys + ((uint64_t)w * n + d) * stride + s;
                    const uint64_t base = first ? init[w * n + d] : *k;
                    const uint64_t a = s_add[p * words + w];
                    const uint64_t x = base + a;
                    const uint64_t y = x + carry;
                    carry = (uint64_t)(x < base) | (uint64_t)(y < x);
                    *k = y;
                }
            }
        }
        __syncthreads();
    }
}

// After the last race of a chunk.  team: [n] team index of each driver; members: [T][n] drivers of each team and
// n_members: [T] (built by the host); init_points: [n]; team_cbits: width of a team key's count fields (its points
// field is the rest of its team_words words).  Histograms are ACCUMULATED into.
__global__ void __launch_bounds__(kChampRankBlock)
champ_rank(const uint64_t *__restrict__ keys, uint64_t m, uint64_t stride, uint32_t n, uint32_t words, uint32_t n_teams,
           uint32_t team_words, uint32_t team_cbits, const uint8_t *__restrict__ members,
           const uint8_t *__restrict__ n_members, const int32_t *__restrict__ init_points, uint32_t gain_cols,
           uint32_t gain_in_lds, unsigned long long *__restrict__ champ_hist, unsigned long long *__restrict__ team_hist,
           unsigned long long *__restrict__ gain_hist)
{
    HIP_DYNAMIC_SHARED(__align__(16) unsigned char, smem)
    const ChampRankLds L = champ_rank_lds(n, words, n_teams, team_words, gain_cols, gain_in_lds != 0);
    uint64_t *dk = reinterpret_cast<uint64_t *>(smem);
    uint64_t *tk = reinterpret_cast<uint64_t *>(smem + L.o_tk);
    uint32_t *h_champ = reinterpret_cast<uint32_t *>(smem + L.o_champ);
    uint32_t *h_team = reinterpret_cast<uint32_t *>(smem + L.o_team);
    uint32_t *h_gain = reinterpret_cast<uint32_t *>(smem + L.o_gain);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = kChampRankBlock / 64;
    const uint32_t hist_words = (L.bytes - L.o_champ) / 4;
    for (uint32_t i = tid; i < hist_words; i += kChampRankBlock) h_champ[i] = 0;
    const uint32_t cb = kChampCountBits, tcb = team_cbits;
    const uint32_t dk_words = words * n * kChampTile, tk_words = team_words * n_teams * kChampTile;
    for (uint64_t s0 = (uint64_t)blockIdx.x * kChampTile; s0 < m; s0 += (uint64_t)gridDim.x * kChampTile) {
        const uint32_t cnt = (m - s0) < (uint64_t)kChampTile ? (uint32_t)(m - s0) : (uint32_t)kChampTile;
        for (uint32_t i = tid; i < dk_words; i += kChampRankBlock) {
            const uint32_t s = i & (kChampTile - 1), row = i / kChampTile;         // row = word * n + driver
            dk[i] = s < cnt ? keys[(uint64_t)row * stride + s0 + s] : 0ull;
        }
        for (uint32_t i = tid; i < tk_words; i += kChampRankBlock) tk[i] = 0ull;
        __syncthreads();
        // team keys: field by field, the sum over the team's drivers, placed at the team layout's offset (fields do
        // not overlap, so each one is OR-ed in once)
        for (uint32_t tm = wave; tm < n_teams; tm += n_waves) {
            const uint32_t nm = n_members[tm];
            uint64_t *key = tk + (uint64_t)tm * kChampTile + lane;
            const uint32_t tstride = n_teams * kChampTile;
            for (uint32_t f = 0; f <= n; ++f) {
                const uint32_t doff = f < n ? (n - 1 - f) * cb : n * cb, dbits = f < n ? cb : kChampPointsBits;
                uint32_t sum = 0;
                for (uint32_t j = 0; j < nm; ++j) {
                    const uint32_t d = members[tm * n + j];
                    sum += champ_field(dk + (uint64_t)d * kChampTile + lane, n * kChampTile, words, doff, dbits);
                }
                const uint32_t toff = f < n ? (n - 1 - f) * tcb : n * tcb;
                const uint32_t w0 = toff >> 6;
                key[(uint64_t)w0 * tstride] |= champ_piece(sum, (int)toff, (int)w0);
                if (w0 + 1 < team_words) key[(uint64_t)(w0 + 1) * tstride] |= champ_piece(sum, (int)toff, (int)w0 + 1);
            }
        }
        __syncthreads();
        if (lane < cnt) {
            const uint32_t dstride = n * kChampTile;
            for (uint32_t d = wave; d < n; d += n_waves) {
                const uint64_t *mine = dk + (uint64_t)d * kChampTile + lane;
                uint32_t pos = 0;
                for (uint32_t e = 0; e < n; ++e) {
                    if (e == d) continue;
                    const int c = champ_cmp(dk + (uint64_t)e * kChampTile + lane, mine, dstride, words);
                    pos += (c > 0 || (c == 0 && e < d)) ? 1u : 0u;
                }
                atomicAdd(&h_champ[d * n + pos], 1u);
                const uint32_t pts = champ_field(mine, dstride, words, n * cb, kChampPointsBits);
                const uint32_t gain = pts - (uint32_t)init_points[d];
                if (gain < gain_cols) {
                    if (gain_in_lds) atomicAdd(&h_gain[d * gain_cols + gain], 1u);
                    else atomicAdd(&gain_hist[(uint64_t)d * gain_cols + gain], 1ull);
                }
            }
            const uint32_t tstride = n_teams * kChampTile;
            for (uint32_t tm = wave; tm < n_teams; tm += n_waves) {
                const uint64_t *mine = tk + (uint64_t)tm * kChampTile + lane;
                uint32_t pos = 0;
                for (uint32_t e = 0; e < n_teams; ++e) {
                    if (e == tm) continue;
                    const int c = champ_cmp(tk + (uint64_t)e * kChampTile + lane, mine, tstride, team_words);
                    pos += (c > 0 || (c == 0 && e < tm)) ? 1u : 0u;
                }
                atomicAdd(&h_team[tm * n_teams + pos], 1u);
            }
        }
        __syncthreads();
    }
    for (uint32_t i = tid; i < n * n; i += kChampRankBlock)
        if (h_champ[i]) atomicAdd(&champ_hist[i], (unsigned long long)h_champ[i]);
    for (uint32_t i = tid; i < n_teams * n_teams; i += kChampRankBlock)
        if (h_team[i]) atomicAdd(&team_hist[i], (unsigned long long)h_team[i]);
    if (gain_in_lds)
        for (uint32_t i = tid; i < n * gain_cols; i += kChampRankBlock)
            if (h_gain[i]) atomicAdd(&gain_hist[i], (unsigned long long)h_gain[i]);
}

}  // namespace mcgp
