// champ_pack.h -- host side of mcgp_run_championship: the key layouts of a call (championship.hip.h) and the tables the
// two standings kernels read -- the teams' members, the initial keys, the key increment of every race and position.
// Plain C++, no device code: mcgp_hip.hip includes it for the C ABI, and the host debugging build of the standings
// kernels (tools/emu/emu_champ.cpp) includes the same text, so that what a test packs on the CPU is what the library
// packs.  The argument checks (and G, awarded, n_cb, which they compute) stay with the C ABI.  champ_remaining builds
// the remaining-points tables of mcgp_run_championship_rounds (champ_rounds.hip.h).  A call with fastest-lap bonuses
// (mcgp_run_championship_bonus, champ_bonus.hip.h) hands both its bonus_points: the caller's G and awarded then include
// the bonuses, pack_championship adds every race's bonus increment and champ_remaining the bonuses still to come.
#pragma once
#include "champ_bonus.hip.h"
#include "championship.hip.h"

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

namespace mcgp {

// Bits needed to hold x (at least 1).
inline uint32_t champ_bits(uint64_t x)
{
    uint32_t b = 1;
    while (b < 64 && (x >> b) != 0) ++b;
    return b;
}

struct ChampPack {
    uint32_t words, team_cbits, team_words, gain_cols;
    std::vector<uint8_t> members, n_members;        // [T][n] drivers of each team, [T]
    std::vector<uint64_t> init_key, add;            // [words][n]; [R][n][words]
    std::vector<int32_t> init_pts;                  // [n]
    std::vector<ChampBonusAdd> bonus_add;           // [R]: the key increment of each race's bonus (zero without one)
};

// The layouts and tables of a call whose arguments passed mcgp_run_championship's checks.  G: the most points one driver
// can gain in these races; awarded: the points the races award in all; n_cb: the countback races (G and awarded with the
// bonuses, when the call has them).  bonus_points: [R] or NULL (no race has a bonus).  "" if the team keys fit, else the
// message.
inline std::string pack_championship(uint32_t n_races, uint32_t n, const int32_t *points, const uint8_t *countback,
                                     const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                                     uint32_t n_teams, uint64_t G, uint64_t awarded, uint32_t n_cb, ChampPack *out,
                                     const int32_t *bonus_points = nullptr)
{
    // ---- key layouts.  Drivers: 5-bit counts and 16-bit points (the limits checked above).  Teams: a team's count in a
    // position grows by at most one per countback race, its points by at most what its drivers can take; the fields
    // are as wide as those bounds need (at the limits: 10-bit counts, 21-bit points, 6 words).
    const uint32_t words = (mcgp::kChampPointsBits + mcgp::kChampCountBits * n + 63) / 64;
    std::vector<uint64_t> team_pts(n_teams, 0), team_cnt((size_t)n_teams * n, 0);
    std::vector<uint32_t> team_size(n_teams, 0);
    std::vector<uint8_t> members((size_t)n_teams * n, 0), n_members(n_teams, 0);
    for (uint32_t d = 0; d < n; ++d) {
        const uint32_t t = (uint32_t)team[d];
        members[(size_t)t * n + team_size[t]++] = (uint8_t)d;
        team_pts[t] += init_points ? (uint64_t)init_points[d] : 0;
        for (uint32_t p = 0; p < n; ++p) team_cnt[(size_t)t * n + p] += init_counts ? (uint64_t)init_counts[(size_t)d * n + p] : 0;
    }
    uint64_t max_tpts = 0, max_tcnt = 0;
    for (uint32_t t = 0; t < n_teams; ++t) {
        n_members[t] = (uint8_t)team_size[t];
        const uint64_t gain = std::min<uint64_t>((uint64_t)team_size[t] * G, awarded);
        max_tpts = std::max<uint64_t>(max_tpts, team_pts[t] + gain);
        for (uint32_t p = 0; p < n; ++p) max_tcnt = std::max<uint64_t>(max_tcnt, team_cnt[(size_t)t * n + p] + n_cb);
    }
    const uint32_t team_cbits = champ_bits(max_tcnt);
    const uint32_t team_words = (champ_bits(max_tpts) + team_cbits * n + 63) / 64;
    if (team_words > (uint32_t)mcgp::kChampMaxTeamWords) return "team standings too wide for a key";
    // initial keys [words][n] and the key increment of each race and position [R][n][words]
    std::vector<uint64_t> init_key((size_t)words * n, 0), add((size_t)n_races * n * words, 0);
    std::vector<int32_t> init_pts(n, 0);
    for (uint32_t d = 0; d < n; ++d) {
        init_pts[d] = init_points ? init_points[d] : 0;
        for (uint32_t w = 0; w < words; ++w) {
            uint64_t k = mcgp::champ_piece((uint64_t)init_pts[d], mcgp::kChampCountBits * (int)n, (int)w);
            for (uint32_t p = 0; p < n && init_counts; ++p)
                k |= mcgp::champ_piece((uint64_t)init_counts[(size_t)d * n + p], mcgp::kChampCountBits * (int)(n - 1 - p), (int)w);
            init_key[(size_t)w * n + d] = k;
        }
    }
    for (uint32_t r = 0; r < n_races; ++r)
        for (uint32_t p = 0; p < n; ++p)
            for (uint32_t w = 0; w < words; ++w)
                add[((size_t)r * n + p) * words + w] =
                    mcgp::champ_piece((uint64_t)points[(size_t)r * n + p], mcgp::kChampCountBits * (int)n, (int)w) |
                    (countback[r] ? mcgp::champ_piece(1, mcgp::kChampCountBits * (int)(n - 1 - p), (int)w) : 0ull);
    // the bonus goes to the points field only
    std::vector<ChampBonusAdd> bonus_add(n_races, ChampBonusAdd{{0, 0, 0}});
    for (uint32_t r = 0; r < n_races && bonus_points; ++r)
        for (uint32_t w = 0; w < words; ++w)
            bonus_add[r].w[w] = mcgp::champ_piece((uint64_t)bonus_points[r], mcgp::kChampCountBits * (int)n, (int)w);
    const uint32_t gain_cols = (uint32_t)G + 1;
    out->words = words;
    out->team_cbits = team_cbits;
    out->team_words = team_words;
    out->gain_cols = gain_cols;
    out->members = std::move(members);
    out->n_members = std::move(n_members);
    out->init_key = std::move(init_key);
    out->add = std::move(add);
    out->init_pts = std::move(init_pts);
    out->bonus_add = std::move(bonus_add);
    return "";
}

// The points still to be had after race r (include/mcgp.h, "Remaining points"): for a driver M_r = the sum over the
// later races q of the largest entry of points[q]; for a team of m drivers B_r = the sum over q of the m largest
// entries of points[q].  driver_rem: [R]; team_rem: [R][T], n_members [T] as pack_championship gives it.  Both are 0
// in the last row.  bonus_points: [R] or NULL; a later race's bonus adds to M_r and, once (one car takes it), to the B_r of
// every team that has a driver.
inline void champ_remaining(uint32_t n_races, uint32_t n, const int32_t *points, const uint8_t *n_members, uint32_t n_teams,
                            std::vector<uint32_t> *driver_rem, std::vector<uint32_t> *team_rem,
                            const int32_t *bonus_points = nullptr)
{
    driver_rem->assign(n_races, 0);
    team_rem->assign((size_t)n_races * n_teams, 0);
    std::vector<uint32_t> best(n + 1, 0);           // best[k]: the k largest entries of the races after r, summed
    std::vector<int32_t> row(n);
    for (uint32_t r = n_races; r-- > 0;) {
        (*driver_rem)[r] = best[1];
        for (uint32_t t = 0; t < n_teams; ++t) (*team_rem)[(size_t)r * n_teams + t] = best[n_members[t]];
        std::copy(points + (size_t)r * n, points + (size_t)(r + 1) * n, row.begin());
        std::sort(row.begin(), row.end(), [](int32_t a, int32_t b) { return a > b; });
        uint32_t sum = 0;
        for (uint32_t k = 1; k <= n; ++k) {
            sum += (uint32_t)row[k - 1];
            best[k] += sum + (bonus_points ? (uint32_t)bonus_points[r] : 0u);
        }
    }
}

}  // namespace mcgp
