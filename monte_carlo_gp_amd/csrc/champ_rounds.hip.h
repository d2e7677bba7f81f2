// champ_rounds.hip.h -- the standings after EVERY race of a season (mcgp_run_championship_rounds, include/mcgp.h).
//
// champ_accumulate (championship.hip.h) leaves every simulation's driver keys as they stand after race r of a chunk and
// the next race overwrites them.  champ_round runs in between: once per race of a chunk, on the keys as they then stand.
// Like champ_rank it takes a tile of 64 simulations per block (one per lane, 4 waves), the keys in LDS, builds the team
// keys and finds every entrant's position by O(n^2) compares.  From the positions and the points fields it counts, per
// race, by the definitions of include/mcgp.h:
//
//   round_hist [n][n]   [driver][standings position after this race]
//   contend    [n]      the driver is in contention: it leads, or (not after the last race) lead - points <= rem
//   secure     [n]      the driver is the only one in contention
//
// and the same three for the teams, whose bound is per team (team_rem[e]).  The entrants of one simulation are spread
// over the block's waves (entrant e goes to wave e % 4), so what one simulation's entrants have to agree on goes
// through LDS between barriers: the leader's index and points (written by whoever finds itself in position 0), then the
// number of contenders (an LDS atomic per contender).  The phases of a tile:
//
//   load      driver keys -> LDS, team keys and contender counts zeroed
//   phase 1   team keys built (champ_rank's field-by-field sum); drivers ranked, the leader published
//   phase 2   teams ranked, their leader published; drivers tested against the leader's points, contenders counted
//   phase 3   teams tested and counted; a simulation with one driver in contention counts its leader as secure
//   phase 4   the same for the teams
//
// Counts go to per-block LDS u32 histograms (a block sees at most one chunk, 2^22 simulations) that are flushed into the
// u64 outputs of this race with global atomics when the block ends.  n_teams = 0: drivers only.
#pragma once

#include "championship.hip.h"

namespace mcgp {

constexpr int kChampRoundBlock = kChampRankBlock;      // 4 waves over a tile of kChampTile simulations

// LDS of champ_round: [driver keys: words][n][64] u64 | [team keys: team_words][T][64] u64 | per simulation: drivers'
// leader, lead, contenders; teams' leader, lead, contenders (6 x [64] u32) | round n x n | contend n | secure n |
// team round T x T | team contend T | team secure T (u32)
struct ChampRoundLds {
    uint32_t o_tk, o_sim, o_hist, o_contend, o_secure, o_tround, o_tcontend, o_tsecure, bytes;
};
__host__ __device__ inline ChampRoundLds champ_round_lds(uint32_t n, uint32_t words, uint32_t n_teams, uint32_t team_words)
{
    ChampRoundLds L;
    L.o_tk = words * n * kChampTile * 8;
    L.o_sim = L.o_tk + team_words * n_teams * kChampTile * 8;
    L.o_hist = L.o_sim + 6 * kChampTile * 4;
    L.o_contend = L.o_hist + n * n * 4;
    L.o_secure = L.o_contend + n * 4;
    L.o_tround = L.o_secure + n * 4;
    L.o_tcontend = L.o_tround + n_teams * n_teams * 4;
    L.o_tsecure = L.o_tcontend + n_teams * 4;
    L.bytes = L.o_tsecure + n_teams * 4;
    L.bytes = (L.bytes + 15) / 16 * 16;
    return L;
}

// Position of entrant `me` among the `count` keys at k[e * kChampTile] (word stride wstride): the entrants with a
// larger key, and on a full tie those with a lower index.
__device__ inline uint32_t champ_position(const uint64_t *k, uint32_t me, uint32_t count, uint32_t wstride, uint32_t words)
{
    const uint64_t *mine = k + (uint64_t)me * kChampTile;
    uint32_t pos = 0;
    for (uint32_t e = 0; e < count; ++e) {
        if (e == me) continue;
        const int c = champ_cmp(k + (uint64_t)e * kChampTile, mine, wstride, words);
        pos += (c > 0 || (c == 0 && e < me)) ? 1u : 0u;
    }
    return pos;
}

// After race r of a chunk (r = 0 .. R - 1; last: r == R - 1).  keys, m, stride, members, n_members, team_cbits: as
// champ_rank takes them.  rem: the most points a driver can still take after this race (M_r); team_rem: [T] the same
// for every team (B_r(e)), both 0 after the last race.  The six outputs are this race's rows and are ACCUMULATED into;
// the team ones are not touched when n_teams == 0.
__global__ void __launch_bounds__(kChampRoundBlock)
champ_round(const uint64_t *__restrict__ keys, uint64_t m, uint64_t stride, uint32_t n, uint32_t words, uint32_t n_teams,
            uint32_t team_words, uint32_t team_cbits, const uint8_t *__restrict__ members,
            const uint8_t *__restrict__ n_members, uint32_t rem, const uint32_t *__restrict__ team_rem, uint32_t last,
            unsigned long long *__restrict__ round_hist, unsigned long long *__restrict__ contend_out,
            unsigned long long *__restrict__ secure_out, unsigned long long *__restrict__ team_round_hist,
            unsigned long long *__restrict__ team_contend_out, unsigned long long *__restrict__ team_secure_out)
{
    HIP_DYNAMIC_SHARED(__align__(16) unsigned char, smem)
    const ChampRoundLds L = champ_round_lds(n, words, n_teams, team_words);
    uint64_t *dk = reinterpret_cast<uint64_t *>(smem);
    uint64_t *tk = reinterpret_cast<uint64_t *>(smem + L.o_tk);
    uint32_t *s_leader = reinterpret_cast<uint32_t *>(smem + L.o_sim), *s_lead = s_leader + kChampTile;
    uint32_t *s_cnt = s_lead + kChampTile, *s_tleader = s_cnt + kChampTile, *s_tlead = s_tleader + kChampTile;
    uint32_t *s_tcnt = s_tlead + kChampTile;
    uint32_t *h_round = reinterpret_cast<uint32_t *>(smem + L.o_hist);
    uint32_t *h_contend = reinterpret_cast<uint32_t *>(smem + L.o_contend);
    uint32_t *h_secure = reinterpret_cast<uint32_t *>(smem + L.o_secure);
    uint32_t *h_tround = reinterpret_cast<uint32_t *>(smem + L.o_tround);
    uint32_t *h_tcontend = reinterpret_cast<uint32_t *>(smem + L.o_tcontend);
    uint32_t *h_tsecure = reinterpret_cast<uint32_t *>(smem + L.o_tsecure);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = kChampRoundBlock / 64;
    const uint32_t hist_words = (L.bytes - L.o_hist) / 4;
    for (uint32_t i = tid; i < hist_words; i += kChampRoundBlock) h_round[i] = 0;
    const uint32_t cb = kChampCountBits, tcb = team_cbits;
    const uint32_t dk_words = words * n * kChampTile, tk_words = team_words * n_teams * kChampTile;
    const uint32_t dstride = n * kChampTile, tstride = n_teams * kChampTile;
    // a team's points field is the rest of its key above the n counts; a team's total is below 2^32
    const uint32_t tp_off = n * tcb;
    const uint32_t tp_bits = n_teams ? (team_words * 64 - tp_off < 32u ? team_words * 64 - tp_off : 32u) : 0u;
    for (uint64_t s0 = (uint64_t)blockIdx.x * kChampTile; s0 < m; s0 += (uint64_t)gridDim.x * kChampTile) {
        const uint32_t cnt = (m - s0) < (uint64_t)kChampTile ? (uint32_t)(m - s0) : (uint32_t)kChampTile;
        for (uint32_t i = tid; i < dk_words; i += kChampRoundBlock) {
            const uint32_t s = i & (kChampTile - 1), row = i / kChampTile;         // row = word * n + driver
            dk[i] = s < cnt ? keys[(uint64_t)row * stride + s0 + s] : 0ull;
        }
        for (uint32_t i = tid; i < tk_words; i += kChampRoundBlock) tk[i] = 0ull;
        if (tid < kChampTile) s_cnt[tid] = s_tcnt[tid] = 0;
        __syncthreads();
        // ---- phase 1.  Team keys: field by field, the sum over the team's drivers, placed at the team layout's offset
        // (fields do not overlap, so each one is OR-ed in once)
        for (uint32_t tm = wave; tm < n_teams; tm += n_waves) {
            const uint32_t nm = n_members[tm];
            uint64_t *key = tk + (uint64_t)tm * kChampTile + lane;
            for (uint32_t f = 0; f <= n; ++f) {
                const uint32_t doff = f < n ? (n - 1 - f) * cb : n * cb, dbits = f < n ? cb : kChampPointsBits;
                uint32_t sum = 0;
                for (uint32_t j = 0; j < nm; ++j) {
                    const uint32_t d = members[tm * n + j];
                    sum += champ_field(dk + (uint64_t)d * kChampTile + lane, dstride, words, doff, dbits);
                }
                const uint32_t toff = f < n ? (n - 1 - f) * tcb : n * tcb;
                const uint32_t w0 = toff >> 6;
                key[(uint64_t)w0 * tstride] |= champ_piece(sum, (int)toff, (int)w0);
                if (w0 + 1 < team_words) key[(uint64_t)(w0 + 1) * tstride] |= champ_piece(sum, (int)toff, (int)w0 + 1);
            }
        }
        if (lane < cnt)
            for (uint32_t d = wave; d < n; d += n_waves) {
                const uint32_t pos = champ_position(dk + lane, d, n, dstride, words);
                atomicAdd(&h_round[d * n + pos], 1u);
                if (pos == 0) {
                    s_leader[lane] = d;
                    s_lead[lane] = champ_field(dk + (uint64_t)d * kChampTile + lane, dstride, words, n * cb, kChampPointsBits);
                }
            }
        __syncthreads();
        // ---- phase 2
        if (lane < cnt) {
            for (uint32_t tm = wave; tm < n_teams; tm += n_waves) {
                const uint32_t pos = champ_position(tk + lane, tm, n_teams, tstride, team_words);
                atomicAdd(&h_tround[tm * n_teams + pos], 1u);
                if (pos == 0) {
                    s_tleader[lane] = tm;
                    s_tlead[lane] = champ_field(tk + (uint64_t)tm * kChampTile + lane, tstride, team_words, tp_off, tp_bits);
                }
            }
            const uint32_t leader = s_leader[lane], lead = s_lead[lane];
            for (uint32_t d = wave; d < n; d += n_waves) {
                const uint32_t pts = champ_field(dk + (uint64_t)d * kChampTile + lane, dstride, words, n * cb, kChampPointsBits);
                if (d == leader || (!last && lead - pts <= rem)) {          // the leader has the most points: lead >= pts
                    atomicAdd(&h_contend[d], 1u);
                    atomicAdd(&s_cnt[lane], 1u);
                }
            }
        }
        __syncthreads();
        // ---- phase 3
        if (lane < cnt) {
            if (n_teams) {
                const uint32_t leader = s_tleader[lane], lead = s_tlead[lane];
                for (uint32_t tm = wave; tm < n_teams; tm += n_waves) {
                    const uint32_t pts = champ_field(tk + (uint64_t)tm * kChampTile + lane, tstride, team_words, tp_off, tp_bits);
                    if (tm == leader || (!last && lead - pts <= team_rem[tm])) {
                        atomicAdd(&h_tcontend[tm], 1u);
                        atomicAdd(&s_tcnt[lane], 1u);
                    }
                }
            }
            if (wave == 0 && s_cnt[lane] == 1) atomicAdd(&h_secure[s_leader[lane]], 1u);
        }
        __syncthreads();
        // ---- phase 4
        if (n_teams && wave == 0 && lane < cnt && s_tcnt[lane] == 1) atomicAdd(&h_tsecure[s_tleader[lane]], 1u);
        __syncthreads();                    // the tile's LDS is read to the end before the next tile's load
    }
    for (uint32_t i = tid; i < n * n; i += kChampRoundBlock)
        if (h_round[i]) atomicAdd(&round_hist[i], (unsigned long long)h_round[i]);
    for (uint32_t i = tid; i < n; i += kChampRoundBlock) {
        if (h_contend[i]) atomicAdd(&contend_out[i], (unsigned long long)h_contend[i]);
        if (h_secure[i]) atomicAdd(&secure_out[i], (unsigned long long)h_secure[i]);
    }
    for (uint32_t i = tid; i < n_teams * n_teams; i += kChampRoundBlock)
        if (h_tround[i]) atomicAdd(&team_round_hist[i], (unsigned long long)h_tround[i]);
    for (uint32_t i = tid; i < n_teams; i += kChampRoundBlock) {
        if (h_tcontend[i]) atomicAdd(&team_contend_out[i], (unsigned long long)h_tcontend[i]);
        if (h_tsecure[i]) atomicAdd(&team_secure_out[i], (unsigned long long)h_tsecure[i]);
    }
}

}  // namespace mcgp
