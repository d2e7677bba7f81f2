// emu_champ.cpp -- DEBUGGING build of the standings kernels' source for the host (not product code, not a fallback:
// nothing in monte_carlo_gp_amd/ can reach it).  Compiles csrc/championship.hip.h with g++ through the stand-in
// <hip/hip_runtime.h> of this directory in its EMU_BLOCK_THREADS mode and calls the two real __global__ functions,
// champ_accumulate and champ_rank, on finishing orders the caller hands in.  The key layout and the kernels' tables
// come from csrc/champ_pack.h, the text the C ABI itself uses.  emu_champ_rounds_run does the same for champ_round
// (csrc/champ_rounds.hip.h), the per-round standings kernel of mcgp_run_championship_rounds, and emu_champ_bonus_run for
// champ_bonus (csrc/champ_bonus.hip.h), the fastest-lap bonus of mcgp_run_championship_bonus, and emu_champ_given_run for
// champ_given (csrc/champ_given.hip.h), the title odds by finishing position of mcgp_run_championship_live.
//
// Execution model: REAL BLOCK SEMANTICS.  A block is 256 host threads (both kernels have a fixed block of 256) that
// run at the same time and meet at __syncthreads(), a pthread barrier; atomicAdd is __atomic_fetch_add; a __shared__
// array is one static object and the dynamic LDS one buffer of exactly the bytes the launch asks for (so that the
// address sanitizer sees an LDS offset past the block's allocation).  The blocks of a grid run one after another on the
// same 256 threads: blockIdx.x = 0 .. grid - 1, and a grid smaller than the tile count makes the kernels' grid-stride
// loops run.  The thread count is the block size, whatever the machine's CPU count.  tests/test_champ_host_build.py.
#define EMU_BLOCK_THREADS 1
#include <pthread.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcgp.h"
#include "../../monte_carlo_gp_amd/csrc/champ_pack.h"
#include "../../monte_carlo_gp_amd/csrc/champ_rounds.hip.h"
#include "../../monte_carlo_gp_amd/csrc/champ_given.hip.h"

thread_local emu_dim3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0};
emu_dim3 blockDim{1, 1, 1}, gridDim{1, 1, 1};
void *emu_dynamic_lds = nullptr;

namespace {

constexpr unsigned kBlock = 256;
static_assert(kBlock == (unsigned)mcgp::kChampAccBlock && kBlock == (unsigned)mcgp::kChampRankBlock, "one block size");
static_assert(kBlock == (unsigned)mcgp::kChampRoundBlock, "one block size");
static_assert(kBlock == (unsigned)mcgp::kChampGivenBlock, "one block size");

pthread_barrier_t g_block_barrier;       // __syncthreads(): the 256 threads of the block
pthread_barrier_t g_pool_barrier;        // start and end of a launch: the 256 threads and the caller

struct Launch {
    void (*body)(void *);
    void *arg;
    unsigned grid;
    bool quit;
} g_launch;

void *pool_thread(void *p)
{
    const unsigned tid = (unsigned)(uintptr_t)p;
    for (;;) {
        pthread_barrier_wait(&g_pool_barrier);                   // a launch is posted
        if (g_launch.quit) return nullptr;
        threadIdx = {tid, 0, 0};
        for (unsigned b = 0; b < g_launch.grid; ++b) {
            blockIdx = {b, 0, 0};
            g_launch.body(g_launch.arg);
            pthread_barrier_wait(&g_block_barrier);              // the block is done before its LDS is reused
        }
        pthread_barrier_wait(&g_pool_barrier);                   // the launch is done
    }
}

struct Pool {
    pthread_t th[kBlock];
    bool up = false;
    void start()
    {
        if (up) return;
        pthread_barrier_init(&g_block_barrier, nullptr, kBlock);
        pthread_barrier_init(&g_pool_barrier, nullptr, kBlock + 1);
        pthread_attr_t at;
        pthread_attr_init(&at);
        pthread_attr_setstacksize(&at, 1 << 20);
        for (unsigned t = 0; t < kBlock; ++t) pthread_create(&th[t], &at, pool_thread, (void *)(uintptr_t)t);
        pthread_attr_destroy(&at);
        up = true;
    }
    void stop()
    {
        if (!up) return;
        g_launch.quit = true;
        pthread_barrier_wait(&g_pool_barrier);
        for (unsigned t = 0; t < kBlock; ++t) pthread_join(th[t], nullptr);
        pthread_barrier_destroy(&g_block_barrier);
        pthread_barrier_destroy(&g_pool_barrier);
        g_launch.quit = false;
        up = false;
    }
} g_pool;

// One kernel launch: grid blocks of 256 threads.
template <typename F>
void launch(unsigned grid, F &&f)
{
    g_launch.body = [](void *a) { (*static_cast<F *>(a))(); };
    g_launch.arg = &f;
    g_launch.grid = grid;
    blockDim = {kBlock, 1, 1};
    gridDim = {grid, 1, 1};
    pthread_barrier_wait(&g_pool_barrier);
    pthread_barrier_wait(&g_pool_barrier);
}

std::string g_err;

int fail(int rc, const std::string &msg, const char **err)
{
    g_err = msg;
    *err = g_err.c_str();
    return rc;
}

// The limits of mcgp_run_championship on a season handed in as finishing orders; G, awarded, n_cb: the three sums the
// checks hand to the layout (pack_championship).
int check_season(uint32_t n_races, uint32_t n, uint64_t n_sims, uint64_t cap, const uint8_t *orders, const int32_t *points,
                 const uint8_t *countback, const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                 uint32_t n_teams, uint32_t acc_grid, uint32_t rank_grid, uint64_t *G_out, uint64_t *awarded_out,
                 uint32_t *n_cb_out, const char **err)
{
    if (n_races < 1 || n_races > (uint32_t)mcgp::kChampMaxRaces) return fail(MCGP_E_BAD_ARG, "n_races must be in [1, 64]", err);
    if (n < 1 || n > MCGP_MAX_CARS) return fail(MCGP_E_BAD_ARG, "n must be in [1, 32]", err);
    if (n_teams < 1 || n_teams > n) return fail(MCGP_E_BAD_ARG, "n_teams must be in [1, n]", err);
    if (cap < 1 || acc_grid < 1 || rank_grid < 1) return fail(MCGP_E_BAD_ARG, "cap and the grids must be at least 1", err);
    for (uint32_t d = 0; d < n; ++d)
        if (team[d] < 0 || (uint32_t)team[d] >= n_teams) return fail(MCGP_E_BAD_ARG, "a team index is outside [0, n_teams)", err);
    // the limits of mcgp_run_championship, and the three sums its checks hand to the layout
    constexpr uint64_t kMaxPoints = (1u << mcgp::kChampPointsBits) - 1, kMaxCount = (1u << mcgp::kChampCountBits) - 1;
    uint64_t G = 0, awarded = 0;
    uint32_t n_cb = 0;
    for (uint32_t r = 0; r < n_races; ++r) {
        if (countback[r] > 1) return fail(MCGP_E_BAD_ARG, "countback[r] must be 0 or 1", err);
        n_cb += countback[r];
        int64_t best = 0;
        for (uint32_t p = 0; p < n; ++p) {
            const int32_t v = points[(size_t)r * n + p];
            if (v < 0 || (uint64_t)v > kMaxPoints) return fail(MCGP_E_BAD_ARG, "a points-table entry is outside [0, 65535]", err);
            if (v > best) best = v;
            awarded += (uint64_t)v;
        }
        G += (uint64_t)best;
    }
    for (uint32_t d = 0; d < n; ++d) {
        const int64_t ip = init_points ? init_points[d] : 0;
        if (ip < 0 || (uint64_t)ip + G > kMaxPoints) return fail(MCGP_E_BAD_ARG, "a driver's total points may leave [0, 65535]", err);
        for (uint32_t p = 0; p < n; ++p) {
            const int64_t ic = init_counts ? init_counts[(size_t)d * n + p] : 0;
            if (ic < 0 || (uint64_t)ic + n_cb > kMaxCount) return fail(MCGP_E_BAD_ARG, "a driver's count may leave [0, 31]", err);
        }
    }
    for (uint64_t i = 0; i < (uint64_t)n_races * n_sims * n; ++i)
        if (orders[i] >= n) return fail(MCGP_E_BAD_ARG, "an order names a driver outside [0, n)", err);
    *G_out = G;
    *awarded_out = awarded;
    *n_cb_out = n_cb;
    return MCGP_OK;
}

}  // namespace

void emu_block_barrier() { pthread_barrier_wait(&g_block_barrier); }

extern "C" {

// The standings of n_sims seasons from their finishing orders.  orders: [n_races][n_sims][n] u8 (driver classified
// p-th); points [n_races][n], countback [n_races], init_points [n] or NULL, init_counts [n][n] or NULL, team [n]: as
// mcgp_run_championship takes them, and checked against the same limits.  The simulations go through in chunks of
// `cap` (the library's staging capacity; the key buffer's simulation stride): every chunk starts from the initial keys
// again, in a key buffer that still holds the chunk before it (0xA5 bytes before the first).  gain_in_lds: 0 or 1, or
// -1 for the library's rule under a block budget of lds_per_block bytes.  acc_grid / rank_grid: most blocks of a
// launch (the library's cu_count * 8 and cu_count * blocks per CU).  champ_hist [n][n], team_hist [T][T] and
// gain_hist [n][G + 1] are ACCUMULATED into.  keys_out: NULL or [words][n][cap], the key buffer after the last chunk.
// info_out: NULL or {words, team_cbits, team_words, gain_cols, gain_in_lds, the rank kernel's LDS bytes}.
int emu_champ_run(uint32_t n_races, uint32_t n, uint64_t n_sims, uint64_t cap, const uint8_t *orders, const int32_t *points,
                  const uint8_t *countback, const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                  uint32_t n_teams, int32_t gain_in_lds_arg, uint32_t lds_per_block, uint32_t acc_grid, uint32_t rank_grid,
                  unsigned long long *champ_hist, unsigned long long *team_hist, unsigned long long *gain_hist,
                  uint64_t *keys_out, uint32_t *info_out, const char **err)
{
    static const char *none = "";
    *err = none;
    if (!orders || !points || !countback || !team || !champ_hist || !team_hist || !gain_hist)
        return fail(MCGP_E_BAD_ARG, "a championship array is NULL", err);
    uint64_t G = 0, awarded = 0;
    uint32_t n_cb = 0;
    const int chk = check_season(n_races, n, n_sims, cap, orders, points, countback, init_points, init_counts, team, n_teams,
                                 acc_grid, rank_grid, &G, &awarded, &n_cb, err);
    if (chk != MCGP_OK) return chk;
    mcgp::ChampPack pk;
    const std::string e = mcgp::pack_championship(n_races, n, points, countback, init_points, init_counts, team, n_teams, G,
                                                  awarded, n_cb, &pk);
    if (!e.empty()) return fail(MCGP_E_BAD_ARG, e, err);
    const uint32_t words = pk.words, gain_cols = pk.gain_cols;
    // the rank kernel's LDS, as the library decides it
    const mcgp::ChampRankLds lds_base = mcgp::champ_rank_lds(n, words, n_teams, pk.team_words, gain_cols, false);
    const mcgp::ChampRankLds lds_gain = mcgp::champ_rank_lds(n, words, n_teams, pk.team_words, gain_cols, true);
    const bool gain_in_lds = gain_in_lds_arg < 0 ? lds_gain.bytes <= lds_per_block / 2 : gain_in_lds_arg != 0;
    const uint32_t rank_lds = gain_in_lds ? lds_gain.bytes : lds_base.bytes;
    if (info_out) {
        const uint32_t info[6] = {words, pk.team_cbits, pk.team_words, gain_cols, gain_in_lds ? 1u : 0u, rank_lds};
        std::memcpy(info_out, info, sizeof(info));
    }
    if (n_sims == 0) return MCGP_OK;
    if (cap > n_sims) cap = n_sims;
    std::vector<uint64_t> keys((size_t)words * n * cap);
    std::memset(keys.data(), 0xA5, keys.size() * 8);
    // exactly the launch's bytes (operator new aligns to 16, as HIP's dynamic LDS is)
    std::vector<unsigned char> lds(rank_lds);
    unsigned char *lds_at = lds.data();
    g_pool.start();
    for (uint64_t done = 0; done < n_sims; done += cap) {
        const uint64_t m = (n_sims - done) < cap ? (n_sims - done) : cap;
        for (uint32_t rr = 0; rr < n_races; ++rr) {
            // the chunk's orders in a buffer of their own size, aligned as an allocation is
            std::vector<uint32_t> stage((m * n + 3) / 4 + 1);
            uint8_t *d_orders = reinterpret_cast<uint8_t *>(stage.data());
            std::memcpy(d_orders, orders + ((size_t)rr * n_sims + done) * n, m * n);
            const uint64_t tiles = (m + mcgp::kChampAccBlock - 1) / mcgp::kChampAccBlock;
            const uint64_t *add = pk.add.data() + (size_t)rr * n * words;
            const uint32_t first = rr == 0 ? 1u : 0u;
            launch((unsigned)(tiles < acc_grid ? tiles : acc_grid), [&] {
                mcgp::champ_accumulate(d_orders, m, n, words, cap, keys.data(), add, pk.init_key.data(), first);
            });
        }
        const uint64_t tiles = (m + mcgp::kChampTile - 1) / mcgp::kChampTile;
        emu_dynamic_lds = lds_at;
        launch((unsigned)(tiles < rank_grid ? tiles : rank_grid), [&] {
            mcgp::champ_rank(keys.data(), m, cap, n, words, n_teams, pk.team_words, pk.team_cbits, pk.members.data(),
                             pk.n_members.data(), pk.init_pts.data(), gain_cols, gain_in_lds ? 1u : 0u, champ_hist, team_hist,
                             gain_hist);
        });
        emu_dynamic_lds = nullptr;
    }
    if (keys_out) std::memcpy(keys_out, keys.data(), keys.size() * 8);
    return MCGP_OK;
}

// The standings after every race of n_sims seasons: emu_champ_run's inputs (orders, tables, standings, teams, cap,
// acc_grid), champ_accumulate after every race of a chunk and champ_round right behind it on a grid of at most
// round_grid blocks, as mcgp_run_championship_rounds launches them.  round_hist [R][n][n], contend [R][n], secure [R][n]
// and, when teams != 0, team_round_hist [R][T][T], team_contend [R][T], team_secure [R][T] are ACCUMULATED into
// (teams == 0: the three may be NULL and the kernel runs without teams).  rem_out: NULL or [R + R * T], the
// remaining-points tables (drivers, then teams).  info_out: NULL or {words, team_cbits, team_words, the kernel's LDS
// bytes}.
int emu_champ_rounds_run(uint32_t n_races, uint32_t n, uint64_t n_sims, uint64_t cap, const uint8_t *orders,
                         const int32_t *points, const uint8_t *countback, const int32_t *init_points,
                         const int32_t *init_counts, const int32_t *team, uint32_t n_teams, uint32_t teams, uint32_t acc_grid,
                         uint32_t round_grid, unsigned long long *round_hist, unsigned long long *contend,
                         unsigned long long *secure, unsigned long long *team_round_hist, unsigned long long *team_contend,
                         unsigned long long *team_secure, uint32_t *rem_out, uint32_t *info_out, const char **err)
{
    static const char *none = "";
    *err = none;
    if (!orders || !points || !countback || !team || !round_hist || !contend || !secure)
        return fail(MCGP_E_BAD_ARG, "a championship array is NULL", err);
    if (teams && (!team_round_hist || !team_contend || !team_secure)) return fail(MCGP_E_BAD_ARG, "a team array is NULL", err);
    uint64_t G = 0, awarded = 0;
    uint32_t n_cb = 0;
    const int chk = check_season(n_races, n, n_sims, cap, orders, points, countback, init_points, init_counts, team, n_teams,
                                 acc_grid, round_grid, &G, &awarded, &n_cb, err);
    if (chk != MCGP_OK) return chk;
    mcgp::ChampPack pk;
    const std::string e = mcgp::pack_championship(n_races, n, points, countback, init_points, init_counts, team, n_teams, G,
                                                  awarded, n_cb, &pk);
    if (!e.empty()) return fail(MCGP_E_BAD_ARG, e, err);
    std::vector<uint32_t> driver_rem, team_rem;
    mcgp::champ_remaining(n_races, n, points, pk.n_members.data(), n_teams, &driver_rem, &team_rem);
    if (rem_out) {
        std::memcpy(rem_out, driver_rem.data(), 4 * driver_rem.size());
        std::memcpy(rem_out + n_races, team_rem.data(), 4 * team_rem.size());
    }
    const uint32_t words = pk.words, T = teams ? n_teams : 0;
    const uint32_t round_lds = mcgp::champ_round_lds(n, words, T, pk.team_words).bytes;
    if (info_out) {
        const uint32_t info[4] = {words, pk.team_cbits, pk.team_words, round_lds};
        std::memcpy(info_out, info, sizeof(info));
    }
    if (n_sims == 0) return MCGP_OK;
    if (cap > n_sims) cap = n_sims;
    std::vector<uint64_t> keys((size_t)words * n * cap);
    std::memset(keys.data(), 0xA5, keys.size() * 8);
    std::vector<unsigned char> lds(round_lds);
    unsigned char *lds_at = lds.data();
    g_pool.start();
    for (uint64_t done = 0; done < n_sims; done += cap) {
        const uint64_t m = (n_sims - done) < cap ? (n_sims - done) : cap;
        for (uint32_t rr = 0; rr < n_races; ++rr) {
            std::vector<uint32_t> stage((m * n + 3) / 4 + 1);
            uint8_t *d_orders = reinterpret_cast<uint8_t *>(stage.data());
            std::memcpy(d_orders, orders + ((size_t)rr * n_sims + done) * n, m * n);
            const uint64_t tiles = (m + mcgp::kChampAccBlock - 1) / mcgp::kChampAccBlock;
            const uint64_t *add = pk.add.data() + (size_t)rr * n * words;
            const uint32_t first = rr == 0 ? 1u : 0u;
            launch((unsigned)(tiles < acc_grid ? tiles : acc_grid), [&] {
                mcgp::champ_accumulate(d_orders, m, n, words, cap, keys.data(), add, pk.init_key.data(), first);
            });
            const uint64_t rtiles = (m + mcgp::kChampTile - 1) / mcgp::kChampTile;
            emu_dynamic_lds = lds_at;
            launch((unsigned)(rtiles < round_grid ? rtiles : round_grid), [&] {
                mcgp::champ_round(keys.data(), m, cap, n, words, T, pk.team_words, pk.team_cbits, pk.members.data(),
                                  pk.n_members.data(), driver_rem[rr], team_rem.data() + (size_t)rr * n_teams,
                                  rr + 1 == n_races ? 1u : 0u, round_hist + (size_t)rr * n * n, contend + (size_t)rr * n,
                                  secure + (size_t)rr * n, T ? team_round_hist + (size_t)rr * T * T : nullptr,
                                  T ? team_contend + (size_t)rr * T : nullptr, T ? team_secure + (size_t)rr * T : nullptr);
            });
            emu_dynamic_lds = nullptr;
        }
    }
    return MCGP_OK;
}

// The standing keys of n_sims seasons with fastest-lap bonuses: emu_champ_run's inputs, and per race bonus_points [R],
// bonus_within [R] and the two byte rows race_fastest_kernel leaves, fl_driver and fl_pos [R][n_sims] (rows of races
// without a bonus are not read).  The argument checks are the library's: the bonuses join G and awarded before the
// limits.  Per chunk and race: champ_accumulate, then champ_bonus where the race has a bonus, on a grid of at most
// acc_grid blocks.  keys_out [words][n][cap]: the key buffer after the last chunk, for the caller to decode; bonus_hist
// and fastest_hist [R][n] are ACCUMULATED into.  info_out: NULL or {words, team_cbits, team_words, gain_cols}.
int emu_champ_bonus_run(uint32_t n_races, uint32_t n, uint64_t n_sims, uint64_t cap, const uint8_t *orders,
                        const int32_t *points, const uint8_t *countback, const int32_t *init_points,
                        const int32_t *init_counts, const int32_t *team, uint32_t n_teams, const int32_t *bonus_points,
                        const int32_t *bonus_within, const uint8_t *fl_driver, const uint8_t *fl_pos, uint32_t acc_grid,
                        uint64_t *keys_out, unsigned long long *bonus_hist, unsigned long long *fastest_hist,
                        uint32_t *info_out, const char **err)
{
    static const char *none = "";
    *err = none;
    if (!orders || !points || !countback || !team || !bonus_points || !bonus_within || !fl_driver || !fl_pos || !keys_out ||
        !bonus_hist || !fastest_hist)
        return fail(MCGP_E_BAD_ARG, "a championship array is NULL", err);
    // check_season's limits hold without the bonuses; G and awarded then take them, and the points limit is tested again
    uint64_t G = 0, awarded = 0;
    uint32_t n_cb = 0;
    if (n_races < 1 || n_races > (uint32_t)mcgp::kChampMaxRaces) return fail(MCGP_E_BAD_ARG, "n_races must be in [1, 64]", err);
    if (n < 1 || n > MCGP_MAX_CARS) return fail(MCGP_E_BAD_ARG, "n must be in [1, 32]", err);
    uint64_t bonus_sum = 0;
    for (uint32_t r = 0; r < n_races; ++r) {
        if (bonus_points[r] < 0 || bonus_points[r] > 65535) return fail(MCGP_E_BAD_ARG, "bonus_points is outside [0, 65535]", err);
        if (bonus_points[r] > 0 && (bonus_within[r] < 1 || (uint32_t)bonus_within[r] > n))
            return fail(MCGP_E_BAD_ARG, "bonus_within is outside [1, n]", err);
        bonus_sum += (uint64_t)bonus_points[r];
    }
    const int chk = check_season(n_races, n, n_sims, cap, orders, points, countback, init_points, init_counts, team, n_teams,
                                 acc_grid, 1, &G, &awarded, &n_cb, err);
    if (chk != MCGP_OK) return chk;
    G += bonus_sum;
    awarded += bonus_sum;
    for (uint32_t d = 0; d < n; ++d)
        if ((uint64_t)(init_points ? init_points[d] : 0) + G > 65535)
            return fail(MCGP_E_BAD_ARG, "a driver's total points may leave [0, 65535]", err);
    mcgp::ChampPack pk;
    const std::string e = mcgp::pack_championship(n_races, n, points, countback, init_points, init_counts, team, n_teams, G,
                                                  awarded, n_cb, &pk, bonus_points);
    if (!e.empty()) return fail(MCGP_E_BAD_ARG, e, err);
    const uint32_t words = pk.words;
    if (info_out) {
        const uint32_t info[4] = {words, pk.team_cbits, pk.team_words, pk.gain_cols};
        std::memcpy(info_out, info, sizeof(info));
    }
    if (n_sims == 0) return MCGP_OK;
    if (cap > n_sims) cap = n_sims;
    std::vector<uint64_t> keys((size_t)words * n * cap);
    std::memset(keys.data(), 0xA5, keys.size() * 8);
    g_pool.start();
    for (uint64_t done = 0; done < n_sims; done += cap) {
        const uint64_t m = (n_sims - done) < cap ? (n_sims - done) : cap;
        for (uint32_t rr = 0; rr < n_races; ++rr) {
            std::vector<uint32_t> stage((m * n + 3) / 4 + 1);
            uint8_t *d_orders = reinterpret_cast<uint8_t *>(stage.data());
            std::memcpy(d_orders, orders + ((size_t)rr * n_sims + done) * n, m * n);
            const uint64_t tiles = (m + mcgp::kChampAccBlock - 1) / mcgp::kChampAccBlock;
            const uint64_t *add = pk.add.data() + (size_t)rr * n * words;
            const uint32_t first = rr == 0 ? 1u : 0u;
            launch((unsigned)(tiles < acc_grid ? tiles : acc_grid), [&] {
                mcgp::champ_accumulate(d_orders, m, n, words, cap, keys.data(), add, pk.init_key.data(), first);
            });
            if (bonus_points[rr] == 0) continue;
            // the chunk's two byte rows in buffers of their own size (an index past the chunk is past the allocation)
            std::vector<uint8_t> d_drv(fl_driver + (size_t)rr * n_sims + done, fl_driver + (size_t)rr * n_sims + done + m);
            std::vector<uint8_t> d_pos(fl_pos + (size_t)rr * n_sims + done, fl_pos + (size_t)rr * n_sims + done + m);
            launch((unsigned)(tiles < acc_grid ? tiles : acc_grid), [&] {
                mcgp::champ_bonus(d_drv.data(), d_pos.data(), m, n, words, cap, keys.data(), pk.bonus_add[rr],
                                  (uint32_t)bonus_within[rr], fastest_hist + (size_t)rr * n, bonus_hist + (size_t)rr * n);
            });
        }
    }
    std::memcpy(keys_out, keys.data(), keys.size() * 8);
    return MCGP_OK;
}

// The title odds by finishing position of n_sims seasons: emu_champ_run's inputs (orders, tables, standings, teams, cap,
// acc_grid) and given_race in [0, n_races).  Per chunk: champ_accumulate after every race, the given race's from a kept
// buffer of exactly the chunk's size that lives to the end of the chunk, then champ_given on the chunk's keys and the kept
// orders on a grid of at most given_grid blocks, as mcgp_run_championship_live launches them.  table_in_lds: 1 for the
// kernel's per-block LDS table, 0 for global atomics; the dynamic LDS is a buffer of exactly champ_given_lds' bytes.
// given_out [n][n][n] ([driver][position][champion]) is ACCUMULATED into.  info_out: NULL or {words, the kernel's LDS
// bytes}.
int emu_champ_given_run(uint32_t n_races, uint32_t n, uint64_t n_sims, uint64_t cap, const uint8_t *orders,
                        const int32_t *points, const uint8_t *countback, const int32_t *init_points,
                        const int32_t *init_counts, const int32_t *team, uint32_t n_teams, uint32_t given_race,
                        uint32_t table_in_lds, uint32_t acc_grid, uint32_t given_grid, unsigned long long *given_out,
                        uint32_t *info_out, const char **err)
{
    static const char *none = "";
    *err = none;
    if (!orders || !points || !countback || !team || !given_out) return fail(MCGP_E_BAD_ARG, "a championship array is NULL", err);
    uint64_t G = 0, awarded = 0;
    uint32_t n_cb = 0;
    const int chk = check_season(n_races, n, n_sims, cap, orders, points, countback, init_points, init_counts, team, n_teams,
                                 acc_grid, given_grid, &G, &awarded, &n_cb, err);
    if (chk != MCGP_OK) return chk;
    if (given_race >= n_races) return fail(MCGP_E_BAD_ARG, "given_race is outside [0, n_races)", err);
    mcgp::ChampPack pk;
    const std::string e = mcgp::pack_championship(n_races, n, points, countback, init_points, init_counts, team, n_teams, G,
                                                  awarded, n_cb, &pk);
    if (!e.empty()) return fail(MCGP_E_BAD_ARG, e, err);
    const uint32_t words = pk.words;
    const uint32_t given_lds = mcgp::champ_given_lds(n, table_in_lds != 0).bytes;
    if (info_out) {
        const uint32_t info[2] = {words, given_lds};
        std::memcpy(info_out, info, sizeof(info));
    }
    if (n_sims == 0) return MCGP_OK;
    // (cap is not cut down to n_sims here: a key stride above the simulation count is part of what is tested)
    std::vector<uint64_t> keys((size_t)words * n * cap);
    std::memset(keys.data(), 0xA5, keys.size() * 8);
    std::vector<unsigned char> lds(given_lds);
    unsigned char *lds_at = lds.data();
    g_pool.start();
    for (uint64_t done = 0; done < n_sims; done += cap) {
        const uint64_t m = (n_sims - done) < cap ? (n_sims - done) : cap;
        // the given race's orders of the chunk, in a buffer of their own size, aligned as an allocation is
        std::vector<uint32_t> keep((m * n + 3) / 4);
        uint8_t *d_keep = reinterpret_cast<uint8_t *>(keep.data());
        for (uint32_t rr = 0; rr < n_races; ++rr) {
            std::vector<uint32_t> stage((m * n + 3) / 4);
            uint8_t *d_orders = rr == given_race ? d_keep : reinterpret_cast<uint8_t *>(stage.data());
            std::memcpy(d_orders, orders + ((size_t)rr * n_sims + done) * n, m * n);
            const uint64_t tiles = (m + mcgp::kChampAccBlock - 1) / mcgp::kChampAccBlock;
            const uint64_t *add = pk.add.data() + (size_t)rr * n * words;
            const uint32_t first = rr == 0 ? 1u : 0u;
            launch((unsigned)(tiles < acc_grid ? tiles : acc_grid), [&] {
                mcgp::champ_accumulate(d_orders, m, n, words, cap, keys.data(), add, pk.init_key.data(), first);
            });
        }
        const uint64_t gtiles = (m + mcgp::kChampGivenBlock - 1) / mcgp::kChampGivenBlock;
        emu_dynamic_lds = lds_at;
        launch((unsigned)(gtiles < given_grid ? gtiles : given_grid), [&] {
            mcgp::champ_given(keys.data(), d_keep, m, cap, n, words, table_in_lds, given_out);
        });
        emu_dynamic_lds = nullptr;
    }
    return MCGP_OK;
}

// Ends the block's threads (they are started by the first run and kept between runs).
void emu_champ_shutdown() { g_pool.stop(); }

}  // extern "C"
