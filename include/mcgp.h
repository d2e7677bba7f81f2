/* mcgp.h -- C ABI of the MI355X (gfx950) Monte Carlo race-simulation engine.
 *
 * libmcgp_hip.so is the drop-in for the reference's hot path
 *     RaceSimulator(config).run_monte_carlo(...)      reference src/simulation.py:56-100
 * (sole call site: reference src/predictor.py:264,283-291).  The reference has no
 * FFI of its own (it is pure Python); these entry points are what a ctypes
 * binding of that method binds -- see INTEGRATION.md for the stub.
 *
 * Conventions
 *   - plain pointers and sizes, no C++ / torch types; caller owns every buffer and
 *     the library keeps no pointer past return;
 *   - every function returns 0 on success or a negative MCGP_E_* code and never
 *     throws or aborts; mcgp_last_error() gives the thread-local message;
 *   - blocking calls, re-entrant for distinct devices (one cached context per
 *     device, guarded by a mutex);
 *   - there is NO CPU fallback: without a usable HIP device every compute entry
 *     point fails with MCGP_E_NO_DEVICE;
 *   - no RNG state: every random draw is a pure function of
 *     (seed, sim_offset + i, lap, purpose, index) (Philox4x32-10), so any split
 *     of [0, N) over calls / devices / ranks sums to the same histogram.
 */
#ifndef MCGP_H
#define MCGP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: mcgp_build_hash, mcgp_run_batch; the retirement draw of laps >= 2 moved to one word per driver and race, which
 * changes the results for a given seed (the oracle's Philox back-end moved with it) */
/* 3: mcgp_run_championship */
/* 4: mcgp_run_matchups */
/* 5: mcgp_race_state, mcgp_run_from_state */
/* 6: mcgp_run_trace; later, mcgp_pit_plan and mcgp_run_strategies (added entry points only: no existing struct or
 * function changed, so the version stays; a caller tests for the symbol); later still, mcgp_run_gaps, in the same way;
 * mcgp_run_championship_rounds likewise; mcgp_run_conditions, mcgp_run_stints and mcgp_run_moves too; and
 * mcgp_run_championship_bonus; mcgp_time_penalty and mcgp_run_penalties; mcgp_lap_event and mcgp_run_events;
 * mcgp_run_championship_live; mcgp_pace_offset and mcgp_run_paces; mcgp_grid_edit and mcgp_run_grids;
 * mcgp_run_pit_windows; mcgp_pace_prior and mcgp_run_priors */
#define MCGP_ABI_VERSION 6
#define MCGP_MAX_CARS 32
#define MCGP_MAX_LAPS 1000

enum {
    MCGP_OK = 0,
    MCGP_E_BAD_ARG = -1,    /* NULL pointer, n out of [1, 32], laps out of [1, 1000], bad enum */
    MCGP_E_NO_DEVICE = -2,  /* no HIP device / device index out of range */
    MCGP_E_HIP = -3,        /* a HIP runtime call failed (message has the HIP error string) */
    MCGP_E_NOMEM = -4       /* device or host allocation failed */
};

/* tyre compounds (reference src/config.py:45-51) and track condition
 * (run_monte_carlo argument `track_condition`, reference src/simulation.py:68) */
enum { MCGP_SOFT = 0, MCGP_MEDIUM = 1, MCGP_HARD = 2, MCGP_INTERMEDIATE = 3, MCGP_WET = 4 };
enum { MCGP_DRY = 0, MCGP_DAMP = 1, MCGP_WET_TRACK = 2 };
enum { MCGP_DEVIATES_32 = 0, MCGP_DEVIATES_53 = 1 };

/* RaceConfig -- replaces the dataclass at reference src/simulation.py:37-52, with
 * the dict-valued fields resolved to dense tables by the caller (the host shim):
 *   tire_compounds[c].get('pace_delta', 0) / .get('deg_rate', 0.05) / .get('optimal_laps', 30)
 *   (reference :317-325, :454-455).
 * pop_*: outcome of `available.pop()` on the two-element set at reference :486,488,
 * which depends on PYTHONHASHSEED in the reference; explicit here. */
typedef struct mcgp_config {
    int32_t total_laps;
    int32_t track_condition;
    double pit_loss;
    double overtake_delta;
    double sc_probability;
    double vsc_probability;
    double red_flag_probability;
    double drs_delta;
    double dirty_air_threshold;
    double dirty_air_penalty;
    double comp_pace_delta[5];
    double comp_deg_rate[5];
    int32_t comp_optimal_laps[5];
    int32_t pop_soft_hard;      /* compound id taken from {SOFT, HARD}   */
    int32_t pop_medium_hard;    /* compound id taken from {MEDIUM, HARD} */
    /* Width of the random deviates.  0 (default): 32-bit uniforms w / 2^32 and normals from a binary32 cubic table --
     * the product's fast path.  MCGP_DEVIATES_53: the reference's width -- 53-bit uniforms (random.random(),
     * np.random.choice: genrand_res53) and binary64 normals (reference src/simulation.py:137,194,302,330,524) --, every
     * draw keeping the 32-bit mode's word as its leading bits and taking 21 more from a companion Philox block; a
     * priced option (half as many Philox blocks again, a binary64 inverse normal from a table in LDS), built for every
     * field size; MCGP_E_BAD_ARG for a problem only the generic kernel takes. */
    int32_t deviates;
} mcgp_config;

/* Per-driver inputs as structure-of-arrays of length n; index = position of the driver
 * in grid_probs' key order.  Replaces the five dict arguments of run_monte_carlo
 * (reference :62-66) with their .get() defaults resolved:
 *   base_pace     base_pace.get(d, 90.0)                           :202,294,514
 *   tire_deg      tire_deg.get(d, 0.05)                            :203,295,514
 *   tire_deg_pit  tire_deg.get(d, 0.0)                             :458
 *   variance      driver_variance.get(d, 0.15)                     :204,296
 *   team_dnf      config.dnf_rates.get(driver_teams.get(d,'Unknown'), 0.002)   :286
 *   lap_dnf       driver_dnf_rates.get(d, team_dnf[d])             :190-193 */
typedef struct mcgp_drivers {
    const double *base_pace;
    const double *tire_deg;
    const double *tire_deg_pit;
    const double *variance;
    const double *team_dnf;
    const double *lap_dnf;
} mcgp_drivers;

int32_t mcgp_abi_version(void);
/* Identity of the binary: the hash of the sources it was compiled from (csrc/source_hash.py: sha256 over the .hip and .h
 * files of csrc/, the Makefile and this header, 16 hex digits; "unknown" for a build outside the Makefile).  The host
 * binding computes the same hash from the tree and refuses a library that carries another one; bench.py quotes
 * profiled counters only when they were taken from a binary with this hash.  The file also holds the text
 * "MCGP_BUILD_HASH=<hash>", readable without loading the library. */
const char *mcgp_build_hash(void);
int32_t mcgp_device_count(void);          /* number of HIP devices, 0 if none */
const char *mcgp_last_error(void);        /* thread-local, never NULL */

/* run_monte_carlo (reference :59-100) on `device`.
 *   grid_probs  n x n row-major [driver][grid slot]     (grid_probs dict, reference :62)
 *   hist_out    n x n row-major [driver][position-1] counts; ACCUMULATED into
 *               (caller zeroes); divide by the total simulation count for the
 *               probabilities of reference :97-100
 *   orders_out  optional, [n_sims][n]: driver index classified p-th in simulation
 *               sim_offset+i; NULL to skip (histogram-only mode writes no per-sim bytes)
 * Host buffers in, host buffers out. */
int32_t mcgp_run(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                 uint32_t n, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                 int32_t device, uint64_t *hist_out, uint8_t *orders_out);

/* Same computation with DEVICE-resident outputs, asynchronous on `stream`
 * (a hipStream_t, NULL = the device's default stream): d_hist (n*n uint64, device,
 * accumulated) and optional d_orders (n_sims*n uint8, device).  Used by the
 * multi-GPU path (RCCL all-reduce of d_hist) and by bench.py.  The small
 * parameter block is uploaded on the same stream before the launch; a block cached
 * from an earlier call on ANOTHER stream is re-used only behind an event wait on
 * that upload, and is overwritten (4 blocks are cached) only after the launches of
 * EVERY stream that used it have completed.  Runs of 2^32 simulations or more are split into several launches
 * on the stream (the per-block histogram counts in 32 bits).  Every launch is preceded, on the same stream, by a
 * 4-byte memset of the stream's work counter (the kernel's waves claim their simulations from it; the library
 * keeps a counter per stream, 8 per device, and recycles the least recently used one behind its last launch).
 * The call itself is NOT capturable into a hipGraph: on a stream's first use it creates events and allocates the
 * counter and the kernel's per-lane scratch, a recycled counter or an evicted parameter block is waited for on the
 * host, and a captured graph would keep a counter the library may later hand to another stream.  A step is one
 * memset + one kernel of ~75 ms at bench size, so there is no launch overhead for a graph to remove.  Results do
 * not depend on which wave ran which simulation. */
int32_t mcgp_run_device(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                        uint32_t n, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                        int32_t device, void *stream, uint64_t *d_hist, uint8_t *d_orders);

/* Several problems in ONE launch: the reference predicts a race from 10 000 simulations (reference
 * src/predictor.py:284) and a backtest runs the races of a season one after the other (src/validation.py:179-185); at
 * that size a launch lasts as long as one race of one lane and most of the device idles.  n_problems races of the same
 * field size n, n_sims simulations each: cfgs[p], drvs[p], grid_probs[p] (n x n) as for mcgp_run, simulation ids
 * sim_offsets[p] .. sim_offsets[p] + n_sims - 1 (NULL: 0) under seeds[p]; hist_out = [n_problems][n][n], ACCUMULATED
 * into only after every launch has succeeded: on an error it is left untouched.  Every problem gets exactly what
 * mcgp_run would give it, error or histogram (a sweep of the reference is a loop over independent predictions): the
 * problems the shared launch takes go into it; a problem at deviates = MCGP_DEVIATES_53, or one only the second kernel
 * serves (lap times near zero, a negative overtake_delta), or every problem under MCGP_FORCE_GENERIC=1, runs by itself
 * inside the same call.  Host buffers in and out, blocking.  mcgp_last_kernel_ms afterwards = the device time of
 * everything the call ran. */
int32_t mcgp_run_batch(uint32_t n_problems, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                       const double *const *grid_probs, uint32_t n, uint64_t n_sims, const uint64_t *sim_offsets,
                       const uint64_t *seeds, int32_t device, uint64_t *hist_out);

/* Championship simulation: drivers' and constructors' title odds over a calendar of n_races races (at most 64) of the same
 * n drivers in the same index order.  Simulation s of the season (ids sim_offset .. sim_offset + n_sims - 1) is the tuple
 * of the finishing orders mcgp_run gives each race r alone for id s: cfgs[r], drvs[r], grid_probs[r] (n x n) under
 * seeds[r], at that race's deviate width.
 *   points       [n_races][n] int32: points of classified position p + 1 (0 past the table; >= 0).  Points go by the
 *                classification the race model makes -- retired cars are classified behind the finishers, as in the
 *                reference -- so a retired car scores when fewer cars finish than the table pays.  Half points: scale
 *                the table by 2.
 *   countback    [n_races] u8: 1 for a Grand Prix, 0 for a sprint (scores, does not count for tie-breaks)
 *   init_points  [n] int32 or NULL (0): points before these races
 *   init_counts  [n][n] int32 or NULL (0): earlier countback finishes of driver d in position p + 1
 *   team         [n] int32: team index of each driver in [0, n_teams), 1 <= n_teams <= n; a team's points and counts
 *                are the sums of its drivers' (its initial standing too)
 * Ranking: more points, then more 1st places, then more 2nd places, ... down to n-th; a full tie goes to the lower
 * driver (team) index.  The regulations decide such a tie by further criteria this model does not have.
 * Outputs, ACCUMULATED into (caller zeroes):
 *   champ_hist   [n][n]    counts of [driver][championship position - 1]
 *   team_hist    [n_teams][n_teams] the same for the teams
 *   gain_hist    [n][G + 1] counts of [driver][points gained in these races], G = sum over r of max_p points[r][p]
 *   race_hist    [n_races][n][n] or NULL: each race's position histogram, equal to mcgp_run's for that race
 * Limits (MCGP_E_BAD_ARG, message names the limit, checked before any device lookup): n in [1, 32], n_races in
 * [1, 64], init_points[d] + G <= 65535, init_counts[d][p] + (number of countback races) <= 31.
 * The device work goes chunk by chunk (2^22 simulations) and race by race through mcgp_run's launch path; device memory
 * does not grow with n_sims.  Host buffers in and out, blocking; any split of [0, N) over calls, sim_offsets or devices
 * sums to the same counts.  mcgp_last_kernel_ms afterwards = the device time of everything the call ran. */
int32_t mcgp_run_championship(uint32_t n_races, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                              const double *const *grid_probs, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                              const uint64_t *seeds, const int32_t *points, const uint8_t *countback,
                              const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                              uint32_t n_teams, int32_t device, uint64_t *champ_hist, uint64_t *team_hist,
                              uint64_t *gain_hist, uint64_t *race_hist);

/* Championship by round: mcgp_run_championship, and the standings after EVERY race of the call.  Every argument through
 * race_hist is mcgp_run_championship's, same order and meaning, and champ_hist, team_hist, gain_hist and race_hist equal
 * what that call gives for the same arguments.
 *
 * Definitions.  R races, n drivers, T teams, points[r][p] as above.  "After race r" (r = 0..R-1) means the initial
 * standings plus races 0..r of the call.  Ranking is the existing one, for drivers and for teams: points, then
 * countback, then the lower index.
 *   - Standings position after race r: the rank of the entrant by that rule among the keys after race r.
 *   - Leader: the entrant in position 0.  It has the most points; `lead` is its points.
 *   - Remaining points.  For a driver: M_r = sum over q > r of max_p points[q][p].  For team e with m_e drivers:
 *     B_r(e) = sum over q > r of (the sum of the m_e largest entries of points[q][0..n)).  Both are 0 for r = R-1.  The
 *     host computes them.
 *   - In contention after race r.  The leader is always in contention.  For r < R-1, any other driver d with
 *     lead - pts_d <= M_r is in contention.  For teams the test is lead - pts_e <= B_r(e).  The bound is inclusive.  A
 *     driver who can draw level on points is still in, because the countback of races not yet run could go their way.
 *     After the last race only the leader is in contention.
 *   - Secure after race r: the entrant is the only one in contention.  The bound is the conventional sufficient one.
 *     It ignores that two entrants cannot both take a race's maximum.  Whoever is secure at r is the final champion,
 *     because points are >= 0.  Once secure, an entrant stays secure.  That follows from the two properties:
 *     secure[r][d] is non-decreasing in r, and secure[R-1][d] = champ_hist[d][0].  The clinch-round distribution is
 *     therefore the difference of consecutive rows.  No per-simulation state has to survive between races.  A title
 *     that is already secure before race 0 shows in row 0.
 *
 * Outputs, ACCUMULATED into (caller zeroes), and only after every launch has succeeded: a call that fails leaves all of
 * them untouched.
 *   round_hist        [R][n][n]  [race][driver][standings position]; required
 *   contend_out       [R][n]     simulations with the driver in contention after race r; required
 *   secure_out        [R][n]     simulations with the driver's title secure after race r; required
 *   team_round_hist   [R][T][T]  \
 *   team_contend_out  [R][T]      > the same for the teams: all three given or all three NULL
 *   team_secure_out   [R][T]     /
 * The limits and argument checks are mcgp_run_championship's, made before any device lookup; a NULL round_hist,
 * contend_out or secure_out, or a partly given team trio, is MCGP_E_BAD_ARG and the message names the argument.  A
 * per-round standings kernel runs after every race of a chunk on the keys as they then stand (csrc/champ_rounds.hip.h);
 * device memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets or devices sums to the same
 * counts.  mcgp_last_kernel_ms afterwards = the device time of the whole call. */
int32_t mcgp_run_championship_rounds(uint32_t n_races, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                                     const double *const *grid_probs, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                                     const uint64_t *seeds, const int32_t *points, const uint8_t *countback,
                                     const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                                     uint32_t n_teams, int32_t device, uint64_t *champ_hist, uint64_t *team_hist,
                                     uint64_t *gain_hist, uint64_t *race_hist, uint64_t *round_hist, uint64_t *contend_out,
                                     uint64_t *secure_out, uint64_t *team_round_hist, uint64_t *team_contend_out,
                                     uint64_t *team_secure_out);

/* Championship with a fastest-lap bonus: mcgp_run_championship_rounds, and per race a bonus for the driver who sets the
 * fastest lap (the 2019-2024 rule: 1 point, if classified in the top ten).  Every argument through team_secure_out is
 * mcgp_run_championship_rounds', same order and meaning, except that round_hist, contend_out and secure_out may be all
 * three NULL (no per-round work; the team trio must then be NULL too).  With every bonus_points[r] == 0 the call
 * returns what mcgp_run_championship_rounds (mcgp_run_championship, without the round trio) returns, cell for cell.
 *
 * Definitions.
 *   - Fastest lap of a race simulation: mcgp_run_trace's.  The smallest last lap time of a car running after lap k,
 *     over laps 2..L; a tie goes to the earlier lap, then to the better running position (strict <, laps in order, cars
 *     in running order).  A race in which no car completes a lap >= 2 has none; every race of one lap is such a race.
 *   - Bonus of race r: bonus_points[r] >= 0 points to the fastest-lap driver, if that driver's classified position
 *     (1-based, the race model's classification) is <= bonus_within[r].  A car that set the fastest lap and retired later
 *     still takes the bonus if it is classified inside the limit, as a retired car scores when fewer cars finish than
 *     the table pays.  The bonus adds to the points only, never to a countback count; team points are the sums of the
 *     drivers' points, bonus included.
 *   - Limits and bounds.  G = sum over r of (max_p points[r][p] + bonus_points[r]): gain_hist has G + 1 columns and the
 *     65535 limit applies to init_points[d] + this G.  By round, the remaining points include the bonuses still to
 *     come: M_r and B_r(e) each add the sum over q > r of bonus_points[q] (at most one car of a team takes a bonus).
 *     Secure stays monotone and secure[R-1] = champ_hist[.][0], because points are >= 0.
 *   bonus_points  [R] int32 in [0, 65535]
 *   bonus_within  [R] int32 in [1, n] where bonus_points[r] > 0, ignored otherwise
 *   bonus_hist    [R][n] or NULL: simulations in which the driver took race r's bonus; ACCUMULATED into
 *   fastest_hist  [R][n] or NULL: simulations in which the driver set race r's fastest lap (equal to mcgp_run_trace's
 *                 fastest_out for that race); ACCUMULATED into; rows of races without a bonus stay untouched
 * Every argument is checked before any device lookup and the message names the field and the race; a race with a bonus
 * at MCGP_DEVIATES_53 is MCGP_E_BAD_ARG (the generic kernel has no 53-bit path).  Outputs are added into only after every
 * launch has succeeded; n_sims == 0 succeeds without a device.
 * Price: a race without a bonus goes through mcgp_run's launch path as before; a race with one runs on the generic
 * kernel's code (race_fastest_kernel, csrc/fastest.hip.h), which tracks lap times: about 52 ms per 10^6 simulations of a
 * 20-car, 60-lap race on an MI355X against 6.7 ms on the register kernel.  champ_bonus (csrc/champ_bonus.hip.h) then adds
 * the bonus to the standing keys behind the race's champ_accumulate.  Added entry point only: MCGP_ABI_VERSION stays 6
 * and a caller tests for the symbol. */
int32_t mcgp_run_championship_bonus(uint32_t n_races, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                                    const double *const *grid_probs, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                                    const uint64_t *seeds, const int32_t *points, const uint8_t *countback,
                                    const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                                    uint32_t n_teams, int32_t device, uint64_t *champ_hist, uint64_t *team_hist,
                                    uint64_t *gain_hist, uint64_t *race_hist, uint64_t *round_hist, uint64_t *contend_out,
                                    uint64_t *secure_out, uint64_t *team_round_hist, uint64_t *team_contend_out,
                                    uint64_t *team_secure_out, const int32_t *bonus_points, const int32_t *bonus_within,
                                    uint64_t *bonus_hist, uint64_t *fastest_hist);

/* Head-to-head and podium-combination counts of one race: mcgp_run's inputs and simulations (ids sim_offset ..
 * sim_offset + n_sims - 1), counted on the device so that no finishing order leaves it.  "Classified" is the race model's
 * order, which puts retired cars behind the finishers, as the reference does.
 *   hist_out    [n][n]    [driver][position - 1] counts, equal to mcgp_run's
 *   ahead_out   [n][n]    [i][j] = simulations in which driver i is classified ahead of driver j: the diagonal is 0 and
 *                         ahead[i][j] + ahead[j][i] = n_sims for i != j
 *   podium_out  [n][n][n] [a][b][c] = simulations whose first three classified cars are a, b, c in that order; NULL to
 *                         skip (n >= 3 required otherwise); the sum over b and c is hist[a][0]
 * All three are ACCUMULATED into (caller zeroes), and only after every launch has succeeded: on an error they are left
 * as they were.  Arguments are checked as mcgp_run checks them, before any device lookup (MCGP_E_BAD_ARG).  The device
 * work goes chunk by chunk (2^22 simulations) through mcgp_run's launch path into a staging buffer that a counting kernel
 * reads; device memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets or devices sums to the
 * same counts.  mcgp_last_kernel_ms afterwards = the device time of everything the call ran. */
int32_t mcgp_run_matchups(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                          uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                          uint64_t *ahead_out, uint64_t *podium_out);

/* A race after lap `lap` (laps completed), as the race model leaves it at the end of that lap; per-car arrays in
 * driver-index order (the mcgp_drivers order). */
typedef struct mcgp_race_state {
    int32_t lap;                      /* laps completed, 1 .. total_laps */
    int32_t drs_disabled_until;       /* 0 .. total_laps + 2: lap + 2 after a red flag or safety car, lap + 1 after a
                                       * VSC (reference simulate_race's variable; 0 if no event has happened) */
    const double *cumulative_time;    /* [n], finite */
    const double *last_lap_time;      /* [n], finite */
    const uint8_t *grid_slot;         /* [n], permutation of 0..n-1 */
    const uint8_t *compound;          /* [n], MCGP_SOFT .. MCGP_WET */
    const uint8_t *used_compounds;    /* [n], bit c = compound c used; must contain `compound` */
    const int16_t *tire_age;          /* [n], 0 .. 1023 - (total_laps - lap) (the age field's width) */
    const int16_t *retired_lap;       /* [n], 0 = running, else 1 .. lap */
} mcgp_race_state;

/* In-race odds: the rest of a race from n_states mid-race states of the same n drivers.  Simulation i of state s (ids
 * sim_offsets[s] .. sim_offsets[s] + n_sims - 1; sim_offsets NULL: 0 for every state) runs laps lap + 1 .. total_laps
 * with the draws mcgp_run's simulation i makes on those laps:
 *   - the field order is rebuilt from the state: all cars, retired ones included, by (cumulative time, grid slot); DRS
 *     and dirty air as the end of lap `lap` sets them (DRS only if lap > 2 and lap > drs_disabled_until); fuel from
 *     the lap number;
 *   - a running car retires on the lap its once-per-race draw gives, if that lap is after `lap` (or never); a draw of
 *     an earlier lap contradicts the state and is redrawn from a second word with the per-lap chain shifted to start at
 *     lap + 1, so that P(retire on lap + j | running) is the per-lap probability chain again;
 *   - classification as mcgp_run's.
 * So a state the race model itself produced for simulation i continues bit for bit into mcgp_run's finishing order of
 * simulation i; giving every state the same ids gives common random numbers (a "pit now / stay out" comparison sees
 * the same futures).
 *   hist_out    [n_states][n][n] [state][driver][position - 1] counts, ACCUMULATED into only after every launch has
 *               succeeded
 *   orders_out  [n_states][n_sims][n] driver index classified p-th, or NULL
 * Every argument is checked before any device lookup: a field outside the limits above, n_states outside [1, 4096],
 * deviates other than MCGP_DEVIATES_32 (the resumed runs have no 53-bit path), a NULL pointer or a non-finite time is
 * MCGP_E_BAD_ARG with a message that names the field and the state.  n_sims == 0 succeeds without a device.  Runs on
 * the generic LDS kernel (mcgp::race_resume_kernel); orders are staged in chunks (at most 2^22 n bytes on the device),
 * a state's runs are split at 2^32 simulations per launch.  Host buffers in and out, blocking.  mcgp_last_kernel_ms
 * afterwards = the device time of everything the call ran. */
int32_t mcgp_run_from_state(const mcgp_config *cfg, const mcgp_drivers *drv, uint32_t n, uint32_t n_states,
                            const mcgp_race_state *states, uint64_t n_sims, const uint64_t *sim_offsets, uint64_t seed,
                            int32_t device, uint64_t *hist_out, uint8_t *orders_out);

/* Live title odds: a championship whose FIRST race resumes from a mid-race state, and the title odds by finishing position
 * in one race of the call.  Every argument through fastest_hist is mcgp_run_championship_bonus', same order and meaning,
 * except that bonus_points and bonus_within may BOTH be NULL (no bonus anywhere; bonus_hist and fastest_hist are then
 * not read) and that the round trio may be NULL as there.
 *   state0           NULL: race 0 from the grid, as before.  Else race 0 is mcgp_run_from_state's race of one state:
 *                    cfgs[0], drvs[0], the state, seed seeds[0], sim_offsets[0] = sim_offset.  Simulation i of the season
 *                    uses for race 0 the finishing order mcgp_run_from_state gives for id sim_offset + i; with race_hist,
 *                    race_hist[0] equals that call's hist_out.  Races 1..R-1 are unchanged.  init_points / init_counts
 *                    are the standings before race 0, as before: nothing is inferred from the state.
 *   given_race       -1: no conditional table; else 0 .. n_races - 1
 *   title_given_out  [n][n][n], NULL exactly when given_race == -1.  Cell [d][p][e] counts the simulations in which driver
 *                    d is classified p + 1-th in race given_race AND driver e is champion.  Champion: position 0 by the
 *                    ranking above (the largest key; a full tie goes to the lower driver index), judged on the final
 *                    standings, bonuses included.  ACCUMULATED into.  Invariants: for every (d, p) the sum over e equals
 *                    race_hist[given_race][d][p]; for every p and e the sum over d equals champ_hist[e][0].
 * Without state0 and with given_race == -1 every output equals mcgp_run_championship_bonus', cell for cell (with the bonus
 * arrays NULL: mcgp_run_championship_rounds' or mcgp_run_championship's), from the same launches.
 * Checks, all before any device lookup, each MCGP_E_BAD_ARG with a message that names the argument: given_race outside
 * [-1, n_races - 1]; title_given_out given with given_race == -1, or NULL otherwise; with state0: grid_probs[0] given,
 * cfgs[0].deviates != MCGP_DEVIATES_32 (the resumed race has no 53-bit path), bonus_points[0] > 0 (the laps before the
 * state are unknown, so the race's fastest lap is not defined), and any field mcgp_run_from_state rejects, with its
 * message.  Without state0, grid_probs[0] is required as before; every championship check is unchanged.
 * n_sims == 0 succeeds without a device.  Outputs are added into only after every launch has succeeded.  Any split of
 * [0, N) over calls, sim_offsets or devices sums to the same counts; device memory does not grow with n_sims (the given
 * race's orders of one chunk stay in a second staging buffer of 2^22 n bytes until the chunk's standings are ranked).
 * Race 0 with a state runs mcgp::race_resume_kernel inside the chunk loop; the table is counted by champ_given
 * (csrc/champ_given.hip.h) behind the chunk's champ_rank: its table is a per-block LDS table when that fits the device's
 * LDS per block next to a tile of orders, else it is counted by global atomics (with a given race,
 * mcgp_last_launch_info / mcgp_last_kernel_name describe the last champ_given launch; its LDS bytes tell the two apart:
 * 256 n rounded up to 16, plus 4 n^3 with the table).  mcgp_last_kernel_ms afterwards = the device time of the whole
 * call.
 * Device times on one MI355X, three S60 races x 10^6 simulations, medians of 5 calls (max - min of the five in brackets;
 * tools/championship_live_time.py): (a) mcgp_run_championship at the parent commit 21.512 ms (1.325; 0.091 without the
 * first call); (b) the same call at this commit 21.515 ms (1.430); (c) this entry with state0 = NULL and given_race = -1
 * 21.550 ms (1.121) -- b and c issue a's launches and lie within a's spread; (d) given_race = 0: 21.694 ms (1.358), champ_given
 * about 0.18 ms; (e) a lap-30 state as race 0: 37.718 ms (0.843), the 30 remaining laps on the generic kernel's code
 * against 60 laps on the register kernel.
 * Added entry point only: MCGP_ABI_VERSION stays 6 and a caller tests for the symbol. */
int32_t mcgp_run_championship_live(uint32_t n_races, const mcgp_config *cfgs, const mcgp_drivers *drvs,
                                   const double *const *grid_probs, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                                   const uint64_t *seeds, const int32_t *points, const uint8_t *countback,
                                   const int32_t *init_points, const int32_t *init_counts, const int32_t *team,
                                   uint32_t n_teams, int32_t device, uint64_t *champ_hist, uint64_t *team_hist,
                                   uint64_t *gain_hist, uint64_t *race_hist, uint64_t *round_hist, uint64_t *contend_out,
                                   uint64_t *secure_out, uint64_t *team_round_hist, uint64_t *team_contend_out,
                                   uint64_t *team_secure_out, const int32_t *bonus_points, const int32_t *bonus_within,
                                   uint64_t *bonus_hist, uint64_t *fastest_hist, const mcgp_race_state *state0,
                                   int32_t given_race, uint64_t *title_given_out);

/* Race trace: what happened lap by lap in mcgp_run's simulations (ids sim_offset .. sim_offset + n_sims - 1, the same
 * draws, so hist_out equals mcgp_run's), counted on the device; no per-lap data leaves it.  Everything is read from the
 * race model's state after the end of lap k (its update_positions), lap 1 included:
 *   - running position after lap k: a car's rank among the cars not retired, by (cumulative time, grid slot); a retired
 *     car has none and counts in column n.  After lap L the running positions are the classified positions of the
 *     running cars;
 *   - laps led: the laps k in 1..L after which the driver is in running position 0;
 *   - pit stops: the laps k in 2..L on which the car pitted, i.e. after which it is running on tyres of age 0;
 *   - fastest lap: the driver with the smallest lap time of a car running after lap k, over laps 2..L (lap 1 records no
 *     lap time); a tie goes to the earlier lap, then to the better running position on that lap; a simulation in which
 *     no car completes a lap >= 2 counts nowhere;
 *   - race events: per simulation, the number of laps 2..L whose event draw gave a red flag, a safety car or a VSC
 *     (the short-circuit chain, counted whether or not any car still runs).
 *   hist_out      [n][n]        [driver][position - 1], equal to mcgp_run's
 *   lap_pos_out   [L][n][n + 1] [lap - 1][driver][running position, or n = retired]; every row sums to n_sims
 *   laps_led_out  [n][L + 1]    [driver][laps led], or NULL
 *   stops_out     [n][L + 1]    [driver][pit stops], or NULL
 *   fastest_out   [n]           simulations in which the driver sets the fastest lap, or NULL
 *   events_out    [3][L + 1]    [red flag, safety car, VSC][number in the race], or NULL
 * L = cfg->total_laps.  All are ACCUMULATED into (caller zeroes), and only after every launch has succeeded: on an error
 * they are left as they were.  Arguments are checked as mcgp_run checks them, before any device lookup (MCGP_E_BAD_ARG);
 * deviates must be MCGP_DEVIATES_32 (the generic kernel runs the trace and has no 53-bit path).  n_sims == 0 succeeds
 * without a device.  The device work goes chunk by chunk through a staging buffer of 512 MiB / (L n) simulations (one
 * byte per lap, driver and simulation; rounded down to a multiple of 256, then to whole rounds of the device's resident
 * blocks, grid_blocks x block_threads of mcgp_last_launch_info, which after this call describes its first chunk's race
 * launch) that counting kernels read; device memory does not grow with n_sims.  Any split
 * of [0, N) over calls, sim_offsets or devices sums to the same counts.  mcgp_last_kernel_ms afterwards = the device time
 * of everything the call ran. */
int32_t mcgp_run_trace(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                       uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                       uint64_t *lap_pos_out, uint64_t *laps_led_out, uint64_t *stops_out, uint64_t *fastest_out,
                       uint64_t *events_out);

/* A pit plan: one driver's strategy in a scenario of mcgp_run_strategies. */
#define MCGP_MAX_PLAN_STOPS 8
#define MCGP_MAX_SCENARIOS 64
typedef struct mcgp_pit_plan {
    int32_t driver;                   /* driver index, 0 .. n - 1, at most one plan per driver and scenario */
    int32_t start_compound;           /* -1: the model's start; else MCGP_SOFT .. MCGP_WET (grid runs only) */
    int32_t start_age;                /* 0 .. 1023 - total_laps with start_compound >= 0; 0 otherwise */
    uint32_t n_stops;                 /* 0 .. MCGP_MAX_PLAN_STOPS */
    int16_t stop_lap[MCGP_MAX_PLAN_STOPS];        /* strictly increasing; [2, L] from the grid, [lap + 1, L] from a state */
    uint8_t stop_compound[MCGP_MAX_PLAN_STOPS];   /* MCGP_SOFT .. MCGP_WET */
} mcgp_pit_plan;

/* Pit-strategy comparison: one race under n_scenarios sets of planned pit stops, with common random numbers.
 * Scenario s holds plan_count[s] plans (concatenated in `plans`), at most one per driver; drivers without a plan keep
 * the race model's rule.  For a planned driver:
 *   - the rule is off: the rule-based stop never fires for this car;
 *   - on each stop lap p it stops where the rule's stop would happen: after its own lap time of lap p is added and
 *     before the overtakes, only if it is still running after that lap.  The stop adds pit_loss, sets the compound,
 *     sets the tyre age to 0 and adds the compound to the used set.  The rule's "more than 5 laps remain" guard does
 *     not apply;
 *   - race events are unchanged: a red flag's free tyre change and the safety car / VSC age decrement apply to it as
 *     to every car, and its later planned stops still happen;
 *   - from the grid (state NULL, grid_probs given), start_compound -1 is the model's start (SOFT at age 4 on slots
 *     1-10, MEDIUM at age 0 behind, INTERMEDIATE / WET on a damp / wet track); otherwise the car starts on that
 *     compound at start_age and its used set is that compound.  Lap 1 has no pit step, so stops lie in [2, L];
 *   - from a state (grid_probs NULL), the state fixes the tyres: start_compound must be -1 and start_age 0; stops lie
 *     in [state->lap + 1, L].
 * The two-compound rule of a dry race is NOT enforced here: a plan may run one dry compound (the Python layer checks).
 * Random numbers: simulation i of every scenario has id sim_offset + i and draws what mcgp_run's (from the grid) or
 * mcgp_run_from_state's (from a state, sim_offsets[0] = sim_offset) simulation i draws.  An empty scenario is therefore
 * bit-identical to those calls, and the grid, the retirement laps and the event draws are shared by every scenario.
 * The lap noise is drawn per place in the running order, so a changed strategy reassigns it: the pairing between
 * scenarios is partial.
 *   hist_out    [S][n][n]      [scenario][driver][position - 1]
 *   delta_out   [S][n][2n - 1] [scenario][driver][(pos_s - pos_0) + n - 1]: the paired change of each driver's position
 *                              against scenario 0 in the same simulation (scenario 0 is all in the centre bin); or NULL
 *   orders_out  [S][n_sims][n] driver index classified p-th, or NULL
 * hist_out and delta_out are ACCUMULATED into, orders_out is written, and all only after every launch has succeeded:
 * on an error they are left as they were.  Every argument is checked before any device lookup: n_scenarios outside
 * [1, 64], a plan outside the limits above (driver, a duplicate driver, start fields, n_stops, a stop lap or
 * compound), an invalid state (as mcgp_run_from_state checks it), grid_probs NULL from the grid or given with a state,
 * deviates other than MCGP_DEVIATES_32 (the generic kernel runs the scenarios and has no 53-bit path), or a NULL
 * pointer is MCGP_E_BAD_ARG with a message that names the scenario, the plan and the field.  n_sims == 0 succeeds
 * without a device.  The device work goes chunk by chunk through a staging buffer of 256 MiB / (S n) simulations (one
 * byte per scenario, simulation and driver) that a counting kernel reads; device memory does not grow with n_sims.  Any
 * split of [0, N) over calls, sim_offsets or devices sums to the same counts.  mcgp_last_kernel_ms afterwards = the
 * device time of everything the call ran; mcgp_last_launch_info describes its first chunk's race launch. */
int32_t mcgp_run_strategies(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                            const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                            const mcgp_pit_plan *plans, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                            int32_t device, uint64_t *hist_out, uint64_t *delta_out, uint8_t *orders_out);

/* A time penalty: seconds added to one driver's race in a scenario of mcgp_run_penalties. */
#define MCGP_MAX_SCENARIO_PENALTIES 256
enum { MCGP_PEN_SERVE_AT_STOP = 0, MCGP_PEN_AT_FLAG = 1, MCGP_PEN_ON_LAP = 2 };
typedef struct mcgp_time_penalty {
    int32_t driver;                   /* driver index, 0 .. n - 1 */
    int32_t kind;                     /* MCGP_PEN_* */
    int32_t lap;                      /* SERVE_AT_STOP: pending from this lap; ON_LAP: the lap; AT_FLAG: 0 */
    double seconds;                   /* finite, in (0, 1e6] */
} mcgp_time_penalty;

/* Time penalties: one race under n_scenarios sets of planned pit stops AND time penalties, with common random numbers.
 * Scenario s holds plan_count[s] plans (concatenated in `plans`; exactly mcgp_run_strategies' plans, with its checks;
 * `plans` may be NULL when every count is 0) and penalty_count[s] penalties (concatenated in `penalties`, which may be
 * NULL when every count is 0).  L = cfg->total_laps; `first` = 2 from the grid and state->lap + 1 from a state, the first
 * lap that has a pit step.
 *   - MCGP_PEN_SERVE_AT_STOP (a 5 s or 10 s penalty): pending from lap `lap` in [first, L]; served at the car's first pit
 *     stop on a lap >= `lap`, the model's rule stop or a planned one.  Served means, where the pit step is:
 *     t = cum + lap_time; t = t + pit_loss; t = t + seconds, in this order.  A red flag's free tyre change is not a stop
 *     and serves nothing.  A car still running at the flag with the penalty unserved adds it at the flag; a car that
 *     retires first never serves it;
 *   - MCGP_PEN_AT_FLAG (a post-race penalty): `lap` must be 0; added at the flag if the car is running;
 *   - MCGP_PEN_ON_LAP (a drive-through, a stop-go, any time lost on a known lap; the caller gives the loss): `lap` in
 *     [first, L]; on that lap t = t + seconds after the car's lap time and after any pit stop of that lap (a served
 *     penalty included), before the overtakes, only if the car is still running after that lap (a car whose retirement
 *     lap is that lap gets nothing).  No tyre change; last_lap_time is untouched, as pit_loss leaves it untouched;
 *   - at the flag, after the last lap and before the classification: every running car adds its unserved SERVE_AT_STOP
 *     seconds, then its AT_FLAG seconds (at most two binary64 additions to its cumulative time, in that order); then the
 *     field is sorted by (time, grid slot) again.  Retired cars are untouched and classify as they always do.
 * Per scenario and driver at most one SERVE_AT_STOP, one AT_FLAG and one ON_LAP per lap (the caller sums penalties of
 * one kind), and at most MCGP_MAX_SCENARIO_PENALTIES penalties per scenario.
 * Random numbers: simulation i of every scenario has id sim_offset + i and draws what mcgp_run's (from the grid) or
 * mcgp_run_from_state's (from a state) simulation i draws; nothing new is drawn, and a pending penalty changes nobody's
 * behaviour (the model has no driver reaction to it).  A scenario without penalties is bit-identical to the same
 * scenario of mcgp_run_strategies.
 *   hist_out    [S][n][n]      [scenario][driver][position - 1]
 *   delta_out   [S][n][2n - 1] as mcgp_run_strategies': paired position changes against scenario 0; or NULL
 *   fate_out    [S][n][4]      [scenario][driver][fate of the driver's SERVE_AT_STOP penalty]: 0 = the driver has none in
 *                              the scenario, 1 = served at a stop, 2 = added at the flag, 3 = retired unserved; every row
 *                              sums to n_sims; or NULL
 *   orders_out  [S][n_sims][n] driver index classified p-th, or NULL
 * hist_out, delta_out and fate_out are ACCUMULATED into, orders_out is written, and all only after every launch has
 * succeeded: on an error they are left as they were.  Every argument is checked before any device lookup: what
 * mcgp_run_strategies checks (n_scenarios, plans, the state, grid_probs, deviates other than MCGP_DEVIATES_32, NULLs),
 * penalty_count NULL or above 256, `penalties` NULL with a non-zero count, and a penalty outside the limits above (kind,
 * driver, lap for its kind and for a grid or state run, seconds, a duplicate) are MCGP_E_BAD_ARG with a message that
 * names the scenario, the penalty and the field.  n_sims == 0 succeeds without a device.  The device work goes chunk by
 * chunk through mcgp_run_strategies' staging budget (one byte per scenario, simulation and driver: position | fate << 5)
 * that one counting kernel reads; device memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets
 * or devices sums to the same counts.  mcgp_last_kernel_name afterwards is "mcgp::race_penalties_kernel".
 * Measured on one MI355X (S60, two scenarios x 10^6 simulations, device ms per 10^6): 98.76 without penalties against
 * 97.76 for mcgp_run_strategies (1 % more, outside its 0.38 ms of noise), 98.6 to 99.0 with one penalised scenario. */
int32_t mcgp_run_penalties(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                           const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                           const mcgp_pit_plan *plans, const uint32_t *penalty_count, const mcgp_time_penalty *penalties,
                           uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                           uint64_t *delta_out, uint64_t *fate_out, uint8_t *orders_out);

/* An event override: on laps first_lap..last_lap (inclusive) of a scenario of mcgp_run_events the race-interrupting event
 * is `kind` instead of what the lap's draw gives. */
#define MCGP_MAX_SCENARIO_EVENTS 64
enum { MCGP_EVT_NONE = 0, MCGP_EVT_RED_FLAG = 1, MCGP_EVT_SAFETY_CAR = 2, MCGP_EVT_VSC = 3 };
typedef struct mcgp_lap_event {
    int32_t first_lap, last_lap;      /* both in [first, L], first_lap <= last_lap */
    int32_t kind;                     /* MCGP_EVT_* */
} mcgp_lap_event;

/* Event scenarios: one race under n_scenarios sets of planned pit stops AND race events set on chosen laps (a safety
 * car on lap 31; no event for the rest of the race; a red flag in the last ten laps), with common random numbers.
 * Scenario s holds plan_count[s] plans (concatenated in `plans`; exactly mcgp_run_strategies' plans, with its checks;
 * `plans` may be NULL when every count is 0) and event_count[s] overrides (concatenated in `events`, which may be NULL
 * when every count is 0).  L = cfg->total_laps; `first` = 2 from the grid and state->lap + 1 from a state, the first lap
 * that has an event step.
 *   - an override covers laps first_lap..last_lap, both in [first, L]; two overrides of one scenario share no lap, and a
 *     scenario has at most MCGP_MAX_SCENARIO_EVENTS of them;
 *   - on a covered lap the outcome of the model's short-circuit chain (red flag, else safety car, else VSC, else
 *     nothing) is REPLACED by `kind`, whatever the lap's event words say: MCGP_EVT_NONE = no event on that lap; any other
 *     kind = that event's handler runs exactly as if it had been drawn.  Laps without an override are drawn as always;
 *   - nothing new is drawn and no other draw moves: a forced VSC still decides its tyre-age decrement from word 3 of the
 *     lap's event block (e3 < t_vsc_tire), a forced event sets drs_disabled_until as a drawn one does, and an event on a
 *     lap with no running car does what a drawn one does.  So a scenario without overrides is cell for cell the same
 *     scenario of mcgp_run_strategies, and a scenario whose overrides equal what a simulation drew changes nothing for
 *     that simulation;
 *   - an event in this model is ONE lap's instantaneous bunching of the field (the gaps close on that lap, DRS is off
 *     for the next one or two laps); it has no duration.  A safety-car period of several laps is a range of laps;
 *   - no driver reacts to a forced event beyond what the model does on a drawn one: pitting under the safety car is
 *     what the caller's plans express (a planned stop on the forced lap).
 * Random numbers: simulation i of every scenario has id sim_offset + i and draws what mcgp_run's (from the grid) or
 * mcgp_run_from_state's (from a state) simulation i draws.
 *   hist_out    [S][n][n]      [scenario][driver][position - 1]
 *   delta_out   [S][n][2n - 1] as mcgp_run_strategies': paired position changes against scenario 0; or NULL
 *   events_out  [S][3][L + 1]  [scenario][red flag, safety car, VSC][number of such laps], over the recorded laps (2..L
 *                              from the grid, state->lap + 1..L from a state), counted as mcgp_run_trace counts (whether
 *                              or not a car still runs), forced and drawn alike; every row sums to n_sims; or NULL
 *   orders_out  [S][n_sims][n] driver index classified p-th, or NULL
 * hist_out, delta_out and events_out are ACCUMULATED into, orders_out is written, and all only after every launch has
 * succeeded: on an error they are left as they were.  Every argument is checked before any device lookup: what
 * mcgp_run_strategies checks (n_scenarios, plans, the state, grid_probs, deviates other than MCGP_DEVIATES_32, NULLs),
 * event_count NULL or above 64, `events` NULL with a non-zero count, a kind outside the enum, first_lap > last_lap, a lap
 * outside [first, L] ("(lap 1 has no event)" from the grid, "(after the state's lap)" from a state) and two overrides of
 * one scenario that share a lap are MCGP_E_BAD_ARG with a message that names the scenario, the override and the field.
 * n_sims == 0 succeeds without a device.  The device work goes chunk by chunk through mcgp_run_strategies' staging budget
 * (one byte per scenario, simulation and driver, and one u32 per scenario and simulation) that one counting kernel reads;
 * device memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets or devices sums to the same
 * counts.  mcgp_last_kernel_name afterwards is "mcgp::race_events_kernel". */
int32_t mcgp_run_events(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                        const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                        const mcgp_pit_plan *plans, const uint32_t *event_count, const mcgp_lap_event *events,
                        uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                        uint64_t *delta_out, uint64_t *events_out, uint8_t *orders_out);

/* A lap-time offset: in a scenario of mcgp_run_paces, `seconds` are added to `driver`'s base pace on laps
 * first_lap..last_lap (MCGP_PACE_LAPS) or from first_lap until the car's next pit stop (MCGP_PACE_UNTIL_STOP). */
#define MCGP_MAX_SCENARIO_PACES 64
enum { MCGP_PACE_LAPS = 0, MCGP_PACE_UNTIL_STOP = 1 };
typedef struct mcgp_pace_offset {
    int32_t driver;               /* 0 .. n - 1 */
    int32_t kind;                 /* MCGP_PACE_* */
    int32_t first_lap, last_lap;  /* LAPS: both in [first, L], first_lap <= last_lap; UNTIL_STOP: first_lap in [first, L], last_lap 0 */
    double seconds;               /* finite, |seconds| <= 60; negative = faster; 0 is legal */
} mcgp_pace_offset;

/* Pace scenarios: one race under n_scenarios sets of planned pit stops AND lap-time offsets (front-wing damage that
 * costs 0.6 s a lap until the nose is changed; an engine mode worth 0.15 s a lap for ten laps; an upgrade worth 0.2 s
 * from lap 1), with common random numbers.  Scenario s holds plan_count[s] plans (concatenated in `plans`; exactly
 * mcgp_run_strategies' plans, with its checks; `plans` may be NULL when every count is 0) and pace_count[s] offsets
 * (concatenated in `paces`, which may be NULL when every count is 0).  L = cfg->total_laps; `first`, the first lap an
 * offset may name, is 1 from the grid (lap 1 reads the base pace too) and state->lap + 1 from a state.
 *   - effective base pace of car d on lap k, built in this order: b = base_pace[d]; if a LAPS offset of d covers lap k,
 *     b = b + seconds; if d's UNTIL_STOP offset is active, b = b + seconds: at most two binary64 additions.  b replaces
 *     base_pace[d] in exactly these places and nowhere else: lap 1's base_lap; the lap time of laps >= 2
 *     ((b + tire) - fuel_effect + ...); the pace of the overtake model on lap k, in the candidate scan and in the
 *     attempt probability, on all three passes.  So, unlike an MCGP_PEN_ON_LAP penalty, a slowed car is easier to pass
 *     and the car behind inherits its lap time through dirty air.  The pit rule, the retirement draw, the event step,
 *     DRS and dirty air, and every random word do not move; nothing new is drawn;
 *   - an UNTIL_STOP offset is active from lap first_lap on.  The pit step of the car's first stop on a lap
 *     q >= first_lap (the rule's or a planned one) clears it: the lap time of lap q carries the offset, because it is
 *     computed before the pit step; the overtakes of lap q and everything later do not.  A red flag's free tyre change
 *     is not a stop and clears nothing (as for mcgp_run_penalties' SERVE_AT_STOP); lap 1 has no pit step;
 *   - per scenario and driver: the LAPS offsets of one driver share no lap; a driver has at most one UNTIL_STOP offset
 *     (a LAPS and an UNTIL_STOP offset may cover the same laps); a scenario has at most MCGP_MAX_SCENARIO_PACES offsets.
 * Identities: a scenario without offsets is cell for cell the same scenario of mcgp_run_strategies; so is a scenario
 * whose offsets are all 0.0 (x + 0.0 == x); a LAPS offset [first, L] on every driver is the race under
 * base_pace[d] + seconds[d], bit for bit.
 * Random numbers: simulation i of every scenario has id sim_offset + i and draws what mcgp_run's (from the grid) or
 * mcgp_run_from_state's (from a state) simulation i draws.
 *   hist_out    [S][n][n]      [scenario][driver][position - 1]
 *   delta_out   [S][n][2n - 1] as mcgp_run_strategies': paired position changes against scenario 0; or NULL
 *   carried_out [S][n][L + 1]  [scenario][driver][c], c = the number of laps whose lap time carried the driver's
 *                              UNTIL_STOP offset, p its first_lap: the car stops on lap q >= p: q - p + 1; it retires
 *                              on lap r > p: r - p; it retires on lap r <= p, or was retired in the state: 0; it runs to
 *                              the flag unstopped: L - p + 1; a driver without an UNTIL_STOP offset in the scenario:
 *                              column 0.  Every row sums to n_sims; or NULL
 *   orders_out  [S][n_sims][n] driver index classified p-th, or NULL
 * hist_out, delta_out and carried_out are ACCUMULATED into, orders_out is written, and all only after every launch has
 * succeeded: on an error they are left as they were.  Every argument is checked before any device lookup: what
 * mcgp_run_strategies checks (n_scenarios, plans, the state, grid_probs, deviates other than MCGP_DEVIATES_32, NULLs),
 * pace_count NULL or above 64, `paces` NULL with a non-zero count, a kind outside the enum, a driver outside [0, n), a lap
 * outside [first, L] ("(after the state's lap)" from a state), first_lap > last_lap, last_lap != 0 with UNTIL_STOP,
 * seconds not finite or |seconds| > 60, two LAPS offsets of one driver that share a lap and a second UNTIL_STOP offset
 * of one driver are MCGP_E_BAD_ARG with a message that names the scenario, the offset and the field.  n_sims == 0
 * succeeds without a device.  The device work goes chunk by chunk through mcgp_run_strategies' staging budget (one byte
 * per scenario, simulation and driver, and a u16 more when carried_out is wanted) that one counting kernel reads; device
 * memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets or devices sums to the same counts.
 * mcgp_last_kernel_name afterwards is "mcgp::race_paces_kernel".
 * Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five with max - min;
 * profiles/paces_time.txt): mcgp_run_strategies built from the parent commit, two empty scenarios, 97.72 (0.34);
 * mcgp_run_paces, two empty scenarios, 99.61 (0.48), 1.9 % more; an empty scenario and one LAPS range of ten laps on one
 * driver 101.24 (0.50); an empty scenario and one UNTIL_STOP offset from lap 5, 105.76 (0.43), 8.2 % more: a lap on which
 * the scenario has an offset pays a bit test wherever a base pace is read, every other lap one wave-uniform test. */
int32_t mcgp_run_paces(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                       const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                       const mcgp_pit_plan *plans, const uint32_t *pace_count, const mcgp_pace_offset *paces,
                       uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                       uint64_t *delta_out, uint64_t *carried_out, uint8_t *orders_out);

/* Combined what-if scenarios: one race under n_scenarios sets of planned pit stops, time penalties, event overrides AND
 * lap-time offsets, with common random numbers ("a safety car on lap 31; NOR has 5 s to serve and stops under it; VER
 * carries 0.4 s of damage until his next stop").  Scenario s holds plan_count[s] plans, penalty_count[s] penalties,
 * event_count[s] overrides and pace_count[s] offsets, each concatenated in its array: the structs, limits and checks of
 * mcgp_run_strategies, mcgp_run_penalties, mcgp_run_events and mcgp_run_paces.  Unlike in those calls, penalty_count,
 * event_count and pace_count may each be NULL: none in any scenario, and the item pointer is then not read.  A non-NULL
 * count array with a non-zero total and a NULL item array is MCGP_E_BAD_ARG.  L = cfg->total_laps.  The first lap an item
 * may name stays per kind: penalties and events 2 from the grid, state->lap + 1 from a state; offsets 1 from the grid,
 * state->lap + 1 from a state.
 * Each rule is the one its own call states above; nothing new is drawn and no draw moves.  On lap k they meet so:
 *   1. event step.  A lap with an override takes the override's kind instead of the chain's outcome, with the drawn
 *      event's handler (bunching, tyre step, drs_disabled_until, re-sort after a tie).  A forced red flag's free tyre
 *      change is not a stop: it serves no SERVE_AT_STOP penalty and clears no UNTIL_STOP offset;
 *   2. car step, for every running car in field order.  b = base_pace[d], + the covering LAPS offset, + the active
 *      UNTIL_STOP offset, stands wherever mcgp_run_paces puts it.  t = cum + lap_time.  If the car stops (rule or plan),
 *      t = t + pit_loss; then, if a SERVE_AT_STOP penalty is pending and k >= its lap, t = t + seconds and it is served;
 *      then, if an UNTIL_STOP offset is active and k >= its first_lap, it is cleared, which does not touch t (the lap
 *      time of lap k carried the offset, the overtakes of lap k do not).  Stopped or not, an ON_LAP addition on lap k:
 *      t = t + seconds.  At most four binary64 additions to t, in that order.  A car that retires on lap k reaches none
 *      of this;
 *   3. overtake passes.  They read the offset pace, as in mcgp_run_paces; penalties make nobody easier to pass;
 *   4. at the flag, after lap L and before classification: every running car adds its unserved SERVE_AT_STOP seconds,
 *      then its AT_FLAG seconds, and the field is sorted by (time, grid slot) again.  A scenario with no SERVE_AT_STOP
 *      and no AT_FLAG penalty skips the step;
 *   5. fate and laps carried as in mcgp_run_penalties and mcgp_run_paces: one stop on a lap k that is >= both laps
 *      gives fate 1 (served at a stop) and closes the carried count at k - first_lap + 1.
 * Identities: a call with every count zero is mcgp_run_strategies on the same plans, cell for cell; a call whose only
 * non-empty table is the penalties is mcgp_run_penalties on the same arguments (hist, delta, fate, every order), and
 * its carried is all in column 0 and its events are mcgp_run_events' counts of a scenario without overrides; the same
 * for events only against mcgp_run_events (fate and carried all in column 0) and for offsets only against
 * mcgp_run_paces; a scenario whose overrides equal what a simulation drew changes nothing for that simulation.
 *   hist_out    [S][n][n]      [scenario][driver][position - 1]
 *   delta_out   [S][n][2n - 1] as mcgp_run_strategies'; or NULL
 *   fate_out    [S][n][4]      as mcgp_run_penalties'; or NULL
 *   events_out  [S][3][L + 1]  as mcgp_run_events'; or NULL
 *   carried_out [S][n][L + 1]  as mcgp_run_paces'; or NULL
 *   orders_out  [S][n_sims][n] driver index classified p-th, or NULL
 * The count outputs are ACCUMULATED into, orders_out is written, and all only after every launch has succeeded: on an
 * error they are left as they were.  delta's centre bin, fate column 0 and carried column 0 are derived on the host
 * from n_sims.  Every argument is checked before any device lookup, the tables in the order penalties, events, offsets,
 * with the single-kind calls' messages: they name the scenario, the item by its table ("penalty 2", "event 0",
 * "offset 1") and the field, so a "lap" or "first_lap" is never ambiguous.  deviates other than MCGP_DEVIATES_32 is
 * refused.  n_sims == 0 succeeds without a device.  The device work goes chunk by chunk through mcgp_run_strategies'
 * staging budget: per scenario and simulation a byte per driver (position | fate << 5), a u32 when events_out is wanted
 * and a u16 per driver when carried_out is wanted, each in its own call's layout and counted by that call's counting
 * kernel; device memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets or devices sums to the
 * same counts.  mcgp_last_kernel_name afterwards is "mcgp::race_combined_kernel"; mcgp_last_launch_info describes the
 * first chunk's race launch.  Added entry point only: MCGP_ABI_VERSION stays 6 and a caller tests for the symbol.
 * Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five with max - min;
 * profiles/combined_time.txt): at the parent commit mcgp_run_strategies 98.22 (0.39), mcgp_run_penalties with
 * a penalty to serve 99.83 (0.34), mcgp_run_events with a safety car 98.97 (0.23), mcgp_run_paces with an UNTIL_STOP
 * offset 106.69 (0.39), the dearest; mcgp_run_combined with two empty scenarios 102.84 (0.41), 3.6 % below that; with the
 * penalty 103.08 (0.35), the safety car 102.50 (0.45), the offset 108.13 (0.49), +1.4 %; with all three and a planned
 * stop 109.59 (0.42), +2.7 %: each kind costs what it costs alone, their meeting nothing. */
int32_t mcgp_run_combined(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                          const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios,
                          const uint32_t *plan_count, const mcgp_pit_plan *plans,
                          const uint32_t *penalty_count, const mcgp_time_penalty *penalties,
                          const uint32_t *event_count, const mcgp_lap_event *events,
                          const uint32_t *pace_count, const mcgp_pace_offset *paces,
                          uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device,
                          uint64_t *hist_out, uint64_t *delta_out, uint64_t *fate_out,
                          uint64_t *events_out, uint64_t *carried_out, uint8_t *orders_out);

/* A track-condition change: in a scenario of mcgp_run_weather, laps first_lap..last_lap have `condition` instead of
 * cfg->track_condition.  A wrong-tyre model: the seconds a car on `compound` loses per lap under `condition`. */
#define MCGP_MAX_SCENARIO_TRACK_CHANGES 64
typedef struct mcgp_track_change {
    int32_t first_lap, last_lap;  /* both in [first, L], first_lap <= last_lap */
    int32_t condition;            /* MCGP_DRY .. MCGP_WET_TRACK */
} mcgp_track_change;
typedef struct mcgp_weather_model {
    double wrong_tyre_sec[3][5];  /* [condition][compound], seconds, finite, in [0, 60] */
} mcgp_weather_model;

/* Weather scenarios: one race under n_scenarios sets of planned pit stops AND track conditions by lap ("it starts to
 * rain on lap 30: who gains if NOR boxes for intermediates at once and VER stays out two laps?"), with common random
 * numbers.  Scenario s holds plan_count[s] plans (concatenated in `plans`; exactly mcgp_run_strategies' plans, with its
 * checks; `plans` may be NULL when every count is 0) and change_count[s] changes (concatenated in `changes`, which may be
 * NULL when every count is 0).  `model` is one table for the whole call.  L = cfg->total_laps; `first`, the first lap a
 * change may name, is 2 from the grid and state->lap + 1 from a state.
 *   - condition of a lap: c_k is the `condition` of the scenario's change that covers lap k, else cfg->track_condition.
 *     Lap 1 from the grid always has cfg->track_condition.  The changes of one scenario share no lap, and a scenario has
 *     at most MCGP_MAX_SCENARIO_TRACK_CHANGES of them; a change to cfg->track_condition is legal and changes nothing;
 *   - classes: SOFT, MEDIUM and HARD are dry tyres, INTERMEDIATE and WET wet tyres; DRY is a dry condition, DAMP and
 *     WET_TRACK wet ones.  A car is on the wrong tyres on lap k iff the class of its compound is not the class of c_k;
 *   - c_k stands wherever lap k's code reads the track condition, and nowhere else: the red flag's free tyre change
 *     (stint_compound(c_k, remaining)), the rule stop's stint_compound, and the rule stop's two-compound waiver (the
 *     waiver tests c_k == MCGP_DRY; the compounds used are still the dry ones the car has run);
 *   - crossover stop: a car under the model's rule (no plan in the scenario) stops when
 *     (age > optimal stint || on the wrong tyres on lap k) && remaining_laps > 5; what follows the test is the rule's
 *     own pit step, with c_k.  Every rule car therefore reacts on the same lap.  A planned driver has the rule off, as
 *     everywhere: "stays out" is a plan without a stop on that lap;
 *   - wrong-tyre pace: b = base_pace[d] + model->wrong_tyre_sec[c_k][compound] replaces base_pace[d] in exactly the places
 *     where mcgp_run_paces puts its b: lap 1's base_lap (cfg->track_condition, the start compound); the lap time of laps
 *     >= 2, with the compound the car is on when the lap time is computed, before the pit step; the pace of the overtake
 *     model in the candidate scan and the attempt on all three passes, with the compound after the pit step.  The table
 *     is read whether or not the class is wrong: intermediates on a fully wet track can cost something too.
 * Identities: a scenario whose changes, if any, all name cfg->track_condition, in which no car is ever on the wrong tyres
 * (true from the grid with plans of the right class) and whose table entries are 0 where it reads them, is cell for cell
 * the same scenario of mcgp_run_strategies, and its wrong_laps is all in column 0.
 * Random numbers: simulation i of every scenario has id sim_offset + i and draws what mcgp_run's (from the grid) or
 * mcgp_run_from_state's (from a state) simulation i draws; nothing new is drawn and no draw moves.
 *   hist_out       [S][n][n]      [scenario][driver][position - 1]
 *   delta_out      [S][n][2n - 1] as mcgp_run_strategies': paired position changes against scenario 0; or NULL
 *   wrong_laps_out [S][n][L + 1]  [scenario][driver][w], w = the number of recorded laps (1 .. L from the grid,
 *                                 state->lap + 1 .. L from a state) whose lap time was computed with the car on the wrong
 *                                 tyres; a car that retires on lap k has no lap time on k.  Every row sums to n_sims; or
 *                                 NULL
 *   orders_out     [S][n_sims][n] driver index classified p-th, or NULL
 * hist_out, delta_out and wrong_laps_out are ACCUMULATED into, orders_out is written, and all only after every launch has
 * succeeded: on an error they are left as they were.  Every argument is checked before any device lookup: what
 * mcgp_run_strategies checks (n_scenarios, plans, the state, grid_probs, deviates other than MCGP_DEVIATES_32, NULLs),
 * change_count NULL or above 64, `changes` NULL with a non-zero count, `model` NULL, a table entry that is not finite or
 * outside [0, 60], a condition outside the enum, a lap outside [first, L] ("(lap 1 has the configuration's condition)"
 * from the grid, "(after the state's lap)" from a state), first_lap > last_lap and two changes of one scenario that share
 * a lap are MCGP_E_BAD_ARG with a message that names the scenario, the change and the field.  n_sims == 0 succeeds
 * without a device.  The device work goes chunk by chunk through mcgp_run_strategies' staging budget (one byte per
 * scenario, simulation and driver, and a u16 more when wrong_laps_out is wanted); device memory does not grow with
 * n_sims.  Any split of [0, N) over calls, sim_offsets or devices sums to the same counts.  mcgp_last_kernel_name
 * afterwards is "mcgp::race_weather_kernel".  Added entry point only: MCGP_ABI_VERSION stays 6 and a caller tests for
 * the symbol.
 * Not in this call: weather inside mcgp_run_combined; a condition that is drawn rather than given; rule cars that react
 * on different laps; MCGP_DEVIATES_53; the register kernels.
 * Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five with max - min;
 * profiles/weather_time.txt): mcgp_run_strategies built from the parent commit, two empty scenarios, 97.39 (0.11);
 * mcgp_run_weather, two empty scenarios and a zero table, 101.64 (0.21), 4.4 % more; an empty scenario and one that is damp
 * from lap L / 2 to the flag, a zero table, 101.44 (0.43), 4.2 % more; the same change under the default table, 107.27 (0.15),
 * 10.1 % more: a lap whose condition has a non-zero row pays a bit test wherever a base pace is read, and the read of the
 * table where the car's entry is non-zero; every other lap one wave-uniform test.  The five other scenario calls compile to the parent's code and keep its times. */
int32_t mcgp_run_weather(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                         const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                         const mcgp_pit_plan *plans, const uint32_t *change_count, const mcgp_track_change *changes,
                         const mcgp_weather_model *model, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                         int32_t device, uint64_t *hist_out, uint64_t *delta_out, uint64_t *wrong_laps_out,
                         uint8_t *orders_out);

/* A grid edit: in a scenario of mcgp_run_grids, `driver` (row index of grid_probs) is moved on the grid that the
 * simulation draws. */
enum { MCGP_GRID_DROP = 0, MCGP_GRID_PIN = 1, MCGP_GRID_PIT_LANE = 2 };
typedef struct mcgp_grid_edit {
    int32_t driver;   /* [0, n) */
    int32_t kind;     /* MCGP_GRID_DROP .. MCGP_GRID_PIT_LANE */
    int32_t value;    /* DROP: places, in [1, 255]; PIN: the slot, in [1, n]; PIT_LANE: 0 */
    double seconds;   /* PIT_LANE: seconds added to lap 1, finite, in [0, 1e6]; DROP and PIN: 0 */
} mcgp_grid_edit;

/* Grid scenarios: one race under n_scenarios sets of planned pit stops AND grid edits ("what does a new power unit
 * cost VER?  A pit-lane start?  NOR and VER have the front row, the rest is a forecast"), with common random numbers.
 * Scenario s holds plan_count[s] plans (concatenated in `plans`; exactly mcgp_run_strategies' plans from the grid, with
 * its checks; `plans` may be NULL when every count is 0) and edit_count[s] edits (concatenated in `edits`, which may be
 * NULL when every count is 0), at most one per driver.  There is no state argument: a mid-race state has no grid.
 * Per simulation, with s_d the slot (0-based) that mcgp_run's simulation of the same id draws for driver d, the slots
 * are assigned in this order:
 *   1. the PIT_LANE drivers take the last slots, ordered among themselves by s_d;
 *   2. the PIN drivers take their slots.  Two pins of one scenario may not name one slot, and a pin must lie in front of
 *      the pit-lane slots;
 *   3. every other driver is sorted by (s_d + drop_d, s_d), drop_d = 0 without an edit, and they fill the free slots front
 *      to back.  With drops alone this is the reference's apply_grid_penalties (src/predictor.py:69-97) per simulation:
 *      a dropped driver whose key ties with a driver drawn on that slot stays in front of it, so a one-place drop moves
 *      nobody; a drop of n - 1 places or more is the back of the grid (for the driver drawn on pole with exactly n - 1,
 *      in front of the car drawn last).
 * The cars are then set up by the new slot: the start compound and age follow it (SOFT at age 4 on slots 1-10 of a dry
 * race, and so on), a plan's start tyres are applied after that, the new slot is the car's grid slot in every tie of
 * times, and lap 1's position factor and top-three clip use it.  A pit-lane car that does not retire on lap 1 gets one
 * more binary64 addition, cum = (0.0 + lap_time) + seconds, before lap 1's sort.
 * Random numbers: nothing new is drawn and no draw moves.  The grid words are drawn exactly as mcgp_run draws them; lap
 * 1's words are keyed by driver and follow the driver.
 * Identities: a scenario without edits is mcgp_run_strategies' scenario cell for cell, an empty scenario mcgp_run's race;
 * a scenario that pins all n drivers gives, for simulation i, what mcgp_simulate_race gives with that grid and
 * sim_id = sim_offset + i.
 *   hist_out   [S][n][n]      [scenario][driver][position - 1]
 *   delta_out  [S][n][2n - 1] as mcgp_run_strategies': paired position changes against scenario 0; or NULL
 *   start_out  [S][n][n]      [scenario][driver][start slot after the edits]; every row and every column sums to n_sims;
 *                             or NULL
 *   gain_out   [S][n][2n - 1] [scenario][driver][(start slot - classified position) + n - 1]: above the centre, places
 *                             gained from the edited grid; every row sums to n_sims; or NULL
 *   orders_out [S][n_sims][n] driver index classified p-th, or NULL
 * hist_out, delta_out, start_out and gain_out are ACCUMULATED into, orders_out is written, and all only after every launch
 * has succeeded: on an error they are left as they were.  Every argument is checked before any device lookup: what
 * mcgp_run_strategies checks from the grid (n_scenarios, plans, grid_probs, deviates other than MCGP_DEVIATES_32, NULLs),
 * edit_count NULL or above n, `edits` NULL with a non-zero count, a driver outside [0, n), a kind outside the enum, a
 * value outside its range, seconds that are not finite or outside [0, 1e6], non-zero seconds on DROP or PIN, two edits of
 * one driver, two pins on one slot and a pin inside the pit-lane slots are MCGP_E_BAD_ARG with a message that names the
 * scenario, the edit and the field.  n_sims == 0 succeeds without a device.  The device work goes chunk by chunk through
 * mcgp_run_strategies' staging budget (one byte per scenario, simulation and driver, and a u16 more when start_out or
 * gain_out is wanted); device memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets or devices
 * sums to the same counts.  mcgp_last_kernel_name afterwards is "mcgp::race_grids_kernel".  Added entry point only:
 * MCGP_ABI_VERSION stays 6 and a caller tests for the symbol.
 * Not in this call: grid edits from a mid-race state or inside mcgp_run_combined; MCGP_DEVIATES_53; the register
 * kernels; a pit-lane start with a free first-lap tyre rule beyond what a plan gives.
 * Price (one MI355X, S60, two scenarios x 10^6 simulations, device ms per 10^6, medians of five with max - min;
 * profiles/grid_time.txt): mcgp_run_strategies built from the parent commit, two empty scenarios, 97.65 (0.20);
 * mcgp_run_grids, two empty scenarios, 98.20 (0.15), 0.6 % more: the edit step is skipped by one wave-uniform test, but the
 * instantiation is another kernel (its table, lap 1's pit-lane test, its own register allocation), and 0.55 ms is outside the
 * parent's spread; an empty scenario and a ten-place drop of one driver, 98.27 (0.51); an empty scenario and a pit-lane
 * start with start_out and gain_out wanted, 99.31 (0.49), 1.7 % more: the u16 staging and grid_count.  The six other
 * scenario calls compile to the parent's code. */
int32_t mcgp_run_grids(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs, uint32_t n,
                       uint32_t n_scenarios, const uint32_t *plan_count, const mcgp_pit_plan *plans,
                       const uint32_t *edit_count, const mcgp_grid_edit *edits, uint64_t n_sims, uint64_t sim_offset,
                       uint64_t seed, int32_t device, uint64_t *hist_out, uint64_t *delta_out, uint64_t *start_out,
                       uint64_t *gain_out, uint8_t *orders_out);

/* A pace prior: in a scenario of mcgp_run_priors, every simulation draws an error of `driver`'s base pace
 * (MCGP_PRIOR_DRIVER) or one error shared by the drivers in `members` (MCGP_PRIOR_GROUP: a team), normal with standard
 * deviation `sigma` seconds a lap. */
#define MCGP_MAX_SCENARIO_PRIORS 64
#define MCGP_MAX_PRIOR_EDGES 15
enum { MCGP_PRIOR_DRIVER = 0, MCGP_PRIOR_GROUP = 1 };
typedef struct mcgp_pace_prior {
    int32_t kind;       /* MCGP_PRIOR_* */
    int32_t driver;     /* DRIVER: 0 .. n - 1; GROUP: 0 */
    uint32_t members;   /* GROUP: bit d = driver d; at least one bit, none at or above n; DRIVER: 0 */
    uint32_t pad;
    double sigma;       /* seconds a lap, finite, 0 <= sigma <= 10 */
} mcgp_pace_prior;

/* Pace uncertainty: one race under n_scenarios sets of planned pit stops AND pace priors ("the pace figures are FP1
 * estimates, good to 0.15 s a driver and 0.2 s a team: how sure are these odds, and what is a tenth worth to VER?"),
 * with common random numbers.  Scenario s holds plan_count[s] plans (concatenated in `plans`; exactly
 * mcgp_run_strategies' plans, with its checks; `plans` may be NULL when every count is 0) and prior_count[s] items
 * (concatenated in `priors`, which may be NULL when every count is 0).  Per scenario a driver has at most one DRIVER item
 * and belongs to at most one GROUP item; a scenario has at most MCGP_MAX_SCENARIO_PRIORS items.
 *   - draws: simulation i has id sim_offset + i = c1 << 32 | c0, and block j is philox4x32_10(c0, c1, 0, 5 << 16 | j)
 *     under the seed, a purpose no other draw has.  Driver d's own deviate is word d & 3 of block d >> 2; the deviate of a
 *     group whose lowest member is g is word g & 3 of block 8 + (g >> 2); z is the word through the model's binary32
 *     inverse-normal table.  A deviate depends on (seed, id, driver index) alone: it is the same in every scenario, from
 *     the grid and from a state, so two scenarios that differ only in their sigmas are compared under common random
 *     numbers.  Only blocks that hold a wanted deviate are drawn.  Every other random word stays where it is;
 *   - offset x_d, binary32 seconds a lap, in this arithmetic: t = sigma_own * (double)z_d for a driver with a DRIVER item,
 *     else t = +0.0; for a member of a group t = t + sigma_group * (double)z_g; x_d = (float)t.  A driver with neither
 *     kind of item has x_d = +0.0f;
 *   - b = base_pace[d] + (double)x_d, one binary64 addition, replaces base_pace[d] where mcgp_run_paces puts its b and
 *     nowhere else: lap 1's base_lap; the lap time of laps >= 2; the pace of the overtake model, in the candidate scan and
 *     in the attempt probability, on all three passes.  From a state it applies to laps state->lap + 1 .. L;
 *   - bins: `edges` holds n_edges (0 .. MCGP_MAX_PRIOR_EDGES) finite, strictly increasing seconds, the same for every
 *     scenario; the bin of x_d is the number of edges e with e <= (double)x_d (an IEEE compare: -0.0 counts as 0.0), which
 *     is searchsorted(edges, x, side='right'); B = n_edges + 1 bins.
 * Identities: a scenario without items, or whose sigmas are all 0, is cell for cell the same scenario of
 * mcgp_run_strategies; simulation i of a scenario is the race under base_pace[d] + (double)x_d(i), which mcgp_run_paces
 * gives with a LAPS offset [first, L] of x_d(i) seconds on every driver.
 *   hist_out    [S][n][n]       [scenario][driver][position - 1]
 *   delta_out   [S][n][2n - 1]  as mcgp_run_strategies': paired position changes against scenario 0; or NULL
 *   draws_out   [S][n][B][n]    [scenario][driver][bin of x_d][position - 1]: the driver's finishing distribution by its
 *                               own drawn error, a pace-sensitivity curve; every [s][d] block sums to n_sims; or NULL
 *   offsets_out [S][n_sims][n]  x_d of each simulation; or NULL
 *   orders_out  [S][n_sims][n]  driver index classified p-th, or NULL
 * hist_out, delta_out and draws_out are ACCUMULATED into, offsets_out and orders_out are written, and all only after every
 * launch has succeeded: on an error they are left as they were.  Every argument is checked before any device lookup: what
 * mcgp_run_strategies checks (n_scenarios, plans, the state, grid_probs, deviates other than MCGP_DEVIATES_32, NULLs),
 * prior_count NULL or above 64, `priors` NULL with a non-zero count, n_edges above 15, `edges` NULL with n_edges > 0, an
 * edge that is not finite or not above the one before, a kind outside the enum, a driver outside [0, n), non-zero
 * members on a DRIVER item or a non-zero driver on a GROUP item, empty members or a bit at or above n, a sigma that is
 * not finite, negative or above 10, a second DRIVER item of one driver and a driver in two groups are MCGP_E_BAD_ARG with
 * a message that names the scenario, the item and the field.  n_sims == 0 succeeds without a device.  The device work goes
 * chunk by chunk through mcgp_run_strategies' staging budget (two bytes per scenario, simulation and driver, and four
 * more when offsets_out is wanted) that one counting kernel reads; device memory does not grow with n_sims.  Any split of
 * [0, N) over calls, sim_offsets or devices sums to the same counts.  mcgp_last_kernel_name afterwards is
 * "mcgp::race_priors_kernel".  Added entry point only: MCGP_ABI_VERSION stays 6 and a caller tests for the symbol.
 * Not in this call: uncertainty in tyre degradation, variance or retirement rates; MCGP_DEVIATES_53; the register kernels;
 * the other what-if rule sets.
 * Launch shape: a lane keeps its n binary32 offsets in LDS behind its rows (4n bytes: 27n against 23n a lane), so a block
 * may hold one wave fewer than mcgp_run_strategies' (DESIGN 3.24 has the shape and the price). */
int32_t mcgp_run_priors(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                        const mcgp_race_state *state, uint32_t n, uint32_t n_scenarios, const uint32_t *plan_count,
                        const mcgp_pit_plan *plans, const uint32_t *prior_count, const mcgp_pace_prior *priors,
                        uint32_t n_edges, const double *edges, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                        int32_t device, uint64_t *hist_out, uint64_t *delta_out, uint64_t *draws_out, float *offsets_out,
                        uint8_t *orders_out);

/* Race time gaps: the model's binary64 cumulative times, counted on the device as histograms over caller-given edges
 * (seconds): every car's gap to the leader by lap, the lead (winning margin on the last lap) and the gap between named
 * pairs of drivers, from the grid or from a mid-race state.  Everything is read from the race model's state after the
 * end of lap k (its update_positions; where mcgp_run_trace reads), L = cfg->total_laps, B = n_edges + 1 bins.
 *   - simulations: from the grid (state NULL, grid_probs given) ids sim_offset .. sim_offset + n_sims - 1 with the draws
 *     of mcgp_run's simulation i; laps 1 .. L are recorded.  From a state (grid_probs NULL, one mcgp_race_state) the
 *     draws and rules of mcgp_run_from_state with sim_offsets[0] = sim_offset; laps state->lap + 1 .. L are recorded
 *     and the rows of earlier laps are left as the caller passed them.  hist_out equals mcgp_run's /
 *     mcgp_run_from_state's for the same ids;
 *   - bins: edges finite, edges[0] > 0, strictly increasing; bin(x) = the number of edges <= x (edges[b - 1] <= x <
 *     edges[b]: a value equal to an edge goes up).  Every binned value is one binary64 subtraction of the cumulative
 *     times of two running cars, the later minus the earlier in the running order, so it is >= 0; no other arithmetic
 *     is applied, so the counts are a pure function of the model's times;
 *   - running order: the cars not retired by (cumulative time, grid slot), as mcgp_run_trace defines it.
 *   hist_out     [n][n]                [driver][position - 1]
 *   lap_gap_out  [L][n][B + 1]         [lap - 1][driver][bin(cum_driver - cum_leader)], column B = retired (no gap).
 *                                      The leader counts in bin 0; each recorded row sums to n_sims; row L - 1 is the
 *                                      finishing-gap distribution of the classified runners
 *   lead_out     [L][B + 1]            [lap - 1][bin(cum_second - cum_leader)], column B = fewer than two cars running;
 *                                      row L - 1 is the winning margin; or NULL
 *   pair_out     [L][n_pairs][2B + 1]  for pair p = (a, b) = pairs[2p], pairs[2p + 1]: column bin(cum_b - cum_a) if both
 *                                      run and a is ahead of b in the running order, B + bin(cum_a - cum_b) if b is
 *                                      ahead, 2B if either has retired; NULL exactly when n_pairs == 0
 * All are ACCUMULATED into (caller zeroes), and only after every launch has succeeded: on an error they are left as they
 * were.  Every argument is checked before any device lookup (MCGP_E_BAD_ARG, the message names the field): what mcgp_run
 * / mcgp_run_from_state check, grid_probs and state both or neither given, n_edges outside [1, 63], an edge that is
 * non-finite, <= 0 or not above its predecessor, n_pairs > 64, a pair index >= n, a pair of one driver, pairs / pair_out
 * NULL with n_pairs > 0 or pair_out given with n_pairs == 0, deviates other than MCGP_DEVIATES_32 (the generic kernel
 * runs the call and has no 53-bit path).  n_sims == 0 succeeds without a device.  The device work goes chunk by chunk
 * through a staging buffer of 512 MiB / (recorded laps x (n + 1 + n_pairs)) simulations (one byte per recorded lap, row
 * and simulation; rounded down to a multiple of 256, then to whole rounds of the device's resident blocks, grid_blocks x
 * block_threads of mcgp_last_launch_info, which after this call describes its first chunk's race launch) that a
 * counting kernel reads; device memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets or
 * devices sums to the same counts.  mcgp_last_kernel_ms afterwards = the device time of everything the call ran;
 * mcgp_last_kernel_name = "mcgp::race_gaps_kernel". */
#define MCGP_MAX_GAP_EDGES 63
#define MCGP_MAX_GAP_PAIRS 64
int32_t mcgp_run_gaps(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                      const mcgp_race_state *state, uint32_t n, uint32_t n_edges, const double *edges, uint32_t n_pairs,
                      const uint8_t *pairs, uint64_t n_sims, uint64_t sim_offset, uint64_t seed, int32_t device,
                      uint64_t *hist_out, uint64_t *lap_gap_out, uint64_t *lead_out, uint64_t *pair_out);

/* Pit window: if driver a stopped at the end of this lap and lost `loss` seconds, where would it rejoin, behind whom, how
 * far behind, and is the stop free?  Counted on the device by lap for up to 64 windows (driver, loss), from the grid or
 * from a mid-race state.  NOTHING IS RE-SIMULATED: the simulations are mcgp_run's / mcgp_run_from_state's, unmodified --
 * same ids, same draws, hist_out equal to theirs -- and a window only asks a question of the times they have after the
 * end of each recorded lap (the race model's update_positions; where mcgp_run_gaps reads).  The race after such a stop
 * (fresh tyres, the traffic's reaction) is mcgp_run_strategies' question.  L = cfg->total_laps, B = n_edges + 1 bins, W =
 * n_windows; several windows may name the same driver with different losses.  For window w = (a, loss) =
 * (window_drivers[w], window_losses[w]) after a lap on which a is running:
 *   - hypothetical rejoin time t* = cum_a + loss: one binary64 addition, the model's own stop arithmetic;
 *   - a running car d != a is ahead at rejoin if (cum_d, grid slot of d) < (t*, grid slot of a) -- the running order's own
 *     key, as mcgp_run_trace defines it --, else behind at rejoin;
 *   - rejoin position = the number of running cars ahead at rejoin, 0-based; places lost = rejoin position - a's own
 *     0-based running position, in [0, n - 1]; a free stop is places lost = 0;
 *   - car ahead = the last car in running order among those ahead at rejoin, car behind = the first among those behind;
 *     gap ahead = t* - cum_ahead and gap behind = cum_behind - t*, one subtraction each, >= 0;
 *   - bins as mcgp_run_gaps has them: edges finite, edges[0] > 0, strictly increasing; bin(x) = the number of edges <= x
 *     (a gap of zero is in bin 0).
 * Laps 1 .. L are recorded from the grid, laps state->lap + 1 .. L from a state; the rows of earlier laps are left as the
 * caller passed them.
 *   hist_out        [n][n]          [driver][position - 1]
 *   rejoin_out      [L][W][n + 1]   [lap - 1][w][rejoin position], column n = a has retired
 *   lost_out        [L][W][n + 1]   [lap - 1][w][places lost], column n = retired
 *   ahead_out       [L][W][n + 2]   [lap - 1][w][driver index of the car ahead], column n = rejoins in the lead, n + 1 =
 *                                   retired
 *   gap_ahead_out   [L][W][B + 1]   [lap - 1][w][bin(gap ahead)], column B = no car ahead, or retired
 *   gap_behind_out  [L][W][B + 1]   [lap - 1][w][bin(gap behind)], column B = no car behind, or retired
 * Every recorded row sums to n_sims.  All are ACCUMULATED into (caller zeroes), and only after every launch has
 * succeeded: on an error they are left as they were.  All six outputs are required.  Every argument is checked before
 * any device lookup (MCGP_E_BAD_ARG, the message names the field): what mcgp_run / mcgp_run_from_state check, grid_probs
 * and state both or neither given, the edge rules of mcgp_run_gaps, n_windows outside [1, 64], a NULL pointer, a driver
 * index >= n, a loss that is not finite or is negative, deviates other than MCGP_DEVIATES_32.  n_sims == 0 succeeds
 * without a device.  The device work goes chunk by chunk through a staging buffer of 1 GiB / (recorded laps x 5 W)
 * simulations (five bytes per recorded lap, window and simulation; rounded as mcgp_run_gaps rounds its chunk) that a
 * counting kernel reads; device memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets or
 * devices sums to the same counts.  mcgp_last_kernel_ms afterwards = the device time of everything the call ran;
 * mcgp_last_kernel_name = "mcgp::race_window_kernel". */
#define MCGP_MAX_PIT_WINDOWS 64
int32_t mcgp_run_pit_windows(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                             const mcgp_race_state *state, uint32_t n, uint32_t n_edges, const double *edges,
                             uint32_t n_windows, const uint8_t *window_drivers, const double *window_losses, uint64_t n_sims,
                             uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out, uint64_t *rejoin_out,
                             uint64_t *lost_out, uint64_t *ahead_out, uint64_t *gap_ahead_out, uint64_t *gap_behind_out);

/* Combination and conditional odds: up to 64 conditions evaluated inside every simulation on its own finished race, from
 * the grid or from a mid-race state; per condition the number of simulations that met it and the position histogram
 * among those.  An atom holds in a simulation iff (lo <= value <= hi) != (negate != 0); a condition holds iff all of its
 * atoms hold; a condition with zero atoms always holds.  Values are integers, read once per simulation after
 * classification:
 *   MCGP_FACT_POSITION(a)     classified position of driver a, 1 .. n (the race model's classification: retired cars
 *                             behind the finishers, as everywhere else in this ABI)
 *   MCGP_FACT_GRID(a)         grid slot of a, 1 .. n: the sampled slot from the grid, grid_slot[a] + 1 from a state
 *   MCGP_FACT_RETIRED_LAP(a)  0 if a is running at the flag, else the lap on which it retired (lap 1 included; from a
 *                             state also the state's own retired_lap of a car that is already out)
 *   MCGP_FACT_AHEAD_BY(a, b)  POSITION(b) - POSITION(a), a != b: > 0 means a is classified ahead of b
 *   MCGP_FACT_GAINED(a)       GRID(a) - POSITION(a)
 *   MCGP_FACT_FINISHERS       the number of cars with RETIRED_LAP = 0
 *   MCGP_FACT_RED_FLAGS / MCGP_FACT_SAFETY_CARS / MCGP_FACT_VSCS
 *                             the number of laps whose event draw gave that event (the short-circuit chain, counted as
 *                             mcgp_run_trace counts it): laps 2 .. L from the grid, laps state->lap + 1 .. L from a state
 *                             (earlier events are not part of a state)
 * a (and b) are ignored for the race-wide facts.  Bounds beyond a fact's range are legal: such an atom is always true or
 * always false.
 *   - simulations: from the grid (state NULL, grid_probs given) ids sim_offset .. sim_offset + n_sims - 1 with the draws
 *     of mcgp_run's simulation i; from a state (grid_probs NULL, one mcgp_race_state) the draws and rules of
 *     mcgp_run_from_state with sim_offsets[0] = sim_offset.
 *   hist_out       [n][n]      [driver][position - 1]: equal to mcgp_run's / mcgp_run_from_state's for the same ids
 *   count_out      [C]         the number of simulations in which condition c holds
 *   cond_hist_out  [C][n][n]   [c][driver][position - 1] over those simulations, or NULL; every row of condition c sums
 *                              to count_out[c]
 * All are ACCUMULATED into (caller zeroes), and only after every launch has succeeded: on an error they are left as they
 * were.  Every argument is checked before any device lookup (MCGP_E_BAD_ARG, the message names the condition, the atom
 * and the field): what mcgp_run / mcgp_run_from_state check, grid_probs and state both or neither given, n_conditions
 * outside [1, 64], conditions / hist_out / count_out NULL, n_atoms > 8, an unknown fact, a (or b, for AHEAD_BY) outside
 * [0, n), a == b for AHEAD_BY, lo > hi, deviates other than MCGP_DEVIATES_32 (the generic kernel runs the call and has no
 * 53-bit path).  n_sims == 0 succeeds without a device.  The device work goes chunk by chunk through a staging buffer of
 * 256 MiB / (n + 8) simulations (per simulation the finishing order, n bytes, and one 64-bit mask of the conditions met;
 * rounded down to a multiple of 256, then to whole rounds of the device's resident blocks, grid_blocks x block_threads of
 * mcgp_last_launch_info, which after this call describes its first chunk's race launch) that a counting kernel reads;
 * device memory does not grow with n_sims.  Any split of [0, N) over calls, sim_offsets or devices sums to the same
 * counts.  mcgp_last_kernel_ms afterwards = the device time of everything the call ran; mcgp_last_kernel_name =
 * "mcgp::race_conditions_kernel". */
#define MCGP_MAX_CONDITIONS 64
#define MCGP_MAX_CONDITION_ATOMS 8
enum { MCGP_FACT_POSITION = 0, MCGP_FACT_GRID = 1, MCGP_FACT_RETIRED_LAP = 2, MCGP_FACT_AHEAD_BY = 3,
       MCGP_FACT_GAINED = 4, MCGP_FACT_FINISHERS = 5, MCGP_FACT_RED_FLAGS = 6, MCGP_FACT_SAFETY_CARS = 7,
       MCGP_FACT_VSCS = 8 };
typedef struct mcgp_condition_atom { int32_t fact, a, b, lo, hi, negate; } mcgp_condition_atom;
typedef struct mcgp_condition { uint32_t n_atoms; mcgp_condition_atom atom[MCGP_MAX_CONDITION_ATOMS]; } mcgp_condition;
int32_t mcgp_run_conditions(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                            const mcgp_race_state *state, uint32_t n, uint32_t n_conditions,
                            const mcgp_condition *conditions, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                            int32_t device, uint64_t *hist_out, uint64_t *count_out, uint64_t *cond_hist_out);

/* Tyre stints: when the race model pits each driver, which compound sequence it runs and how a driver's finishing
 * positions split by stop count, counted on the device, from the grid or from a mid-race state.  Everything is read from
 * the race model's state after the end of lap k (its update_positions; where mcgp_run_trace reads), L = cfg->total_laps.
 *   - recorded laps: from the grid laps 2 .. L (lap 1 has no pit step and no race event); from a state laps state->lap +
 *     1 .. L (stops before the state's lap are unknown and not counted);
 *   - pit stop on lap k: the car is running after lap k with tyre age 0 (mcgp_run_trace's definition); red-flag change
 *     on lap k: lap k's event is a red flag and the car is running after lap k;
 *   - stints: a car begins a new stint on a recorded lap with a pit stop or a red-flag change (both on one lap: one
 *     stint), on the compound it has after that lap.  Stint 0 is on the compound the race starts on (from a state:
 *     state->compound[d], for retired cars too), so every car has at least one; a car's stops and stints count up to
 *     its retirement;
 *   - simulations: from the grid (state NULL, grid_probs given) ids sim_offset .. sim_offset + n_sims - 1 with the draws
 *     of mcgp_run's simulation i; from a state (grid_probs NULL, one mcgp_race_state) the draws and rules of
 *     mcgp_run_from_state with sim_offsets[0] = sim_offset.
 *   hist_out       [n][n]          [driver][position - 1]: equal to mcgp_run's / mcgp_run_from_state's for the same ids
 *   stop_lap_out   [n][4][L + 1]   [driver][k][lap of the driver's (k + 1)-th stop among the recorded laps], column 0 =
 *                                  no such stop; every [driver][k] row sums to n_sims, column 1 stays 0, a fifth or
 *                                  later stop is recorded nowhere here
 *   stops_pos_out  [n][5][n]       [driver][min(stops, 4)][position - 1], or NULL; summed over the stops axis it equals
 *                                  hist_out
 *   seq_out        [n][1296]       [driver][code], or NULL: code = sum over j < m of (c_j + 1) 6^j for a car with m <= 4
 *                                  stints on compounds c_0 .. c_{m-1} (MCGP_SOFT .. MCGP_WET), column 0 = more than 4
 *                                  stints; every row sums to n_sims
 * All are ACCUMULATED into (caller zeroes), and only after every launch has succeeded: on an error they are left as they
 * were.  Every argument is checked before any device lookup (MCGP_E_BAD_ARG, the message names the field): what mcgp_run
 * / mcgp_run_from_state check, grid_probs and state both or neither given, hist_out / stop_lap_out NULL, deviates other
 * than MCGP_DEVIATES_32 (the generic kernel runs the call and has no 53-bit path).  n_sims == 0 succeeds without a
 * device.  The device work goes chunk by chunk through a staging buffer of 256 MiB / (9 n) simulations (per driver and
 * simulation one 64-bit record and one position byte; rounded down to a multiple of 256, then to whole rounds of the
 * device's resident blocks, grid_blocks x block_threads of mcgp_last_launch_info, which after this call describes its
 * first chunk's race launch) that a counting kernel reads; device memory does not grow with n_sims.  Any split of [0, N)
 * over calls, sim_offsets or devices sums to the same counts.  mcgp_last_kernel_ms afterwards = the device time of
 * everything the call ran; mcgp_last_kernel_name = "mcgp::race_stints_kernel". */
#define MCGP_STINT_STOPS 4        /* stops whose lap is recorded; stop counts are capped here */
#define MCGP_STINT_SEQ 4          /* stints a sequence code holds */
#define MCGP_STINT_SEQ_CODES 1296 /* 6^4 */
int32_t mcgp_run_stints(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                        const mcgp_race_state *state, uint32_t n, uint64_t n_sims, uint64_t sim_offset,
                        uint64_t seed, int32_t device, uint64_t *hist_out, uint64_t *stop_lap_out,
                        uint64_t *stops_pos_out, uint64_t *seq_out);

/* Race movement: how a car got where it finished -- the joint grid x finish table, the places won or lost at the start
 * and the passes by driver, lap and pair -- counted on the device, from the grid or from a mid-race state.  Everything is
 * read where mcgp_run_trace reads: after update_positions of lap k, L = cfg->total_laps.  Let run_k(d) mean "d is not
 * retired after lap k".  Let pos_k(d) be its running position among the running cars, in `ord` order (cumulative time,
 * then grid slot).  Let pit_k(d) mean "running after lap k with tyre age 0", for k >= 2.  This is the trace's definition.
 *   - Baseline.  From the grid, pos_0(d) is d's sampled grid slot and every car runs.  From a state after lap k0, the
 *     baseline is pos_k0.  This is the order start_from_state leaves after its own update_positions.
 *   - Start gain (from the grid only).  This is slot(d) - pos_1(d).  A car that retires on lap 1 has none.
 *   - Pass on lap k.  From the grid, k runs over 2..L.  From a state, k runs over k0 + 1..L.  Take an ordered pair (a, b)
 *     with run_{k-1} and run_k true for both.  If pos_{k-1}(a) > pos_{k-1}(b) and pos_k(a) < pos_k(b), then a took a
 *     place from b on lap k.  The pass is through the pits if pit_k(a) or pit_k(b).  Otherwise it is on track.  A place
 *     gained because a car retired is not a pass.  This is the model's order change, not a claim about a wheel-to-wheel
 *     move: two lap ends are compared, and a place swapped twice within a lap is not seen.
 *   - Classified position.  This is classify_and_count's position.  Retired cars rank behind the runners, as in hist.
 *   - simulations: from the grid (state NULL, grid_probs given) ids sim_offset .. sim_offset + n_sims - 1 with the draws
 *     of mcgp_run's simulation i; from a state (grid_probs NULL, one mcgp_race_state) the draws and rules of
 *     mcgp_run_from_state with sim_offsets[0] = sim_offset.
 *   hist_out         [n][n]        [driver][position - 1]: equal to mcgp_run's / mcgp_run_from_state's for the same ids
 *   grid_fin_out     [n][n][n]     [driver][grid slot][classified position - 1]; from a state the slot is
 *                                  state->grid_slot.  Summed over slots it equals hist_out
 *   start_gain_out   [n][2n]       [driver][slot - pos_1 + n - 1]; column 2n - 1 = retired on lap 1; every row sums to
 *                                  n_sims.  May be NULL; with a state it MUST be NULL
 *   passes_out       [n][4][128]   [driver][kind][min(count, MCGP_MOVE_DRIVER_CAP)]; kinds: 0 made on track, 1 lost on
 *                                  track, 2 gained through the pits, 3 lost through the pits; every [driver][kind] row
 *                                  sums to n_sims.  May be NULL
 *   race_passes_out  [1024]        [min(on-track passes of the race, MCGP_MOVE_RACE_CAP)]; sums to n_sims.  May be NULL
 *   lap_passes_out   [L + 1][2]    [lap][on track, through the pits]: the passes on that lap summed over the simulations;
 *                                  rows 0 and 1 stay 0.  May be NULL
 *   pair_passes_out  [n][n]        [a][b]: times a took a place from b on track, summed over laps and simulations.  May
 *                                  be NULL
 * All are ACCUMULATED into (caller zeroes), and only after every launch has succeeded: on an error they are left as they
 * were.  An output that is NULL is not counted.  Every argument is checked before any device lookup (MCGP_E_BAD_ARG, the
 * message names the field): what mcgp_run / mcgp_run_from_state check, grid_probs and state both or neither given,
 * hist_out / grid_fin_out NULL, start_gain_out with a state, deviates other than MCGP_DEVIATES_32 (the generic kernel
 * runs the call and has no 53-bit path).  n_sims == 0 succeeds without a device.  The device work goes chunk by chunk
 * through a staging buffer of 512 MiB / ((L + 2) n) simulations (one byte per lap and driver as mcgp_run_trace stages
 * them, then every driver's grid slot and classified position; at most the launch cap, rounded down to a multiple of 256,
 * then to whole rounds of the device's resident blocks, grid_blocks x block_threads of mcgp_last_launch_info, which after
 * this call describes its first chunk's race launch) that two counting kernels read; with passes_out the first hands the
 * second 4 n more bytes per simulation of the chunk.  Device memory does not grow with n_sims.  Any split of [0, N) over
 * calls, sim_offsets or devices sums to the same counts.  mcgp_last_kernel_ms afterwards = the device time of everything
 * the call ran; mcgp_last_kernel_name = "mcgp::race_moves_kernel". */
#define MCGP_MOVE_DRIVER_CAP 127   /* a driver's passes of one kind in one race, saturating */
#define MCGP_MOVE_RACE_CAP  1023   /* on-track passes in one race, saturating */
int32_t mcgp_run_moves(const mcgp_config *cfg, const mcgp_drivers *drv, const double *grid_probs,
                       const mcgp_race_state *state, uint32_t n, uint64_t n_sims, uint64_t sim_offset, uint64_t seed,
                       int32_t device, uint64_t *hist_out, uint64_t *grid_fin_out, uint64_t *start_gain_out,
                       uint64_t *passes_out, uint64_t *race_passes_out, uint64_t *lap_passes_out,
                       uint64_t *pair_passes_out);

/* simulate_race (reference :147-242): one race from a FIXED starting grid
 * (grid[p] = driver index on slot p), simulation id sim_id.  order_out[p] = driver
 * index classified p-th.  Bit-identical to what mcgp_run computes for a simulation
 * whose sampled grid equals `grid`. */
int32_t mcgp_simulate_race(const mcgp_config *cfg, const mcgp_drivers *drv, const uint8_t *grid,
                           uint32_t n, uint64_t sim_id, uint64_t seed, int32_t device,
                           uint8_t *order_out);

/* Grid-probability front end on the device ("next" row f3): the n x n matrix [driver][grid slot] that
 * F1Predictor._predict_quali + _adjust_for_penalties build from the Elo quali ratings
 * (reference src/elo.py:124-141 softmax; src/predictor.py:321-375 teammate / form / circuit adjustments and the
 * Gaussian bump around (1 - p) n; :377-407 penalty shift).  Inputs are arrays of length n in driver order with the
 * reference's .get() defaults resolved by the caller (rating: ratings.get(d).get('quali', 1500); features: 0;
 * penalty: grid positions, strings already mapped through PENALTY_TYPES).  exp() is the front end's own
 * (csrc/frontend_exp.h): results agree with the reference's numpy matrices to ~1e-15 relative and are
 * bit-identical to the CPU oracle's restatement of the same text.
 *   mcgp_grid_probs        host arrays in, host matrix out (n x n doubles)
 *   mcgp_run_from_ratings  run_monte_carlo with the matrix produced ON THE DEVICE, written by the front-end
 *                          kernel straight into the race kernel's parameter block (no host round trip);
 *                          hist_out as in mcgp_run, grid_probs_out optional (NULL to skip). */
int32_t mcgp_grid_probs(const double *quali_rating, const double *teammate_delta, const double *form_score,
                        const double *circuit_affinity, const int32_t *penalty, uint32_t n, int32_t device,
                        double *grid_probs_out);
int32_t mcgp_run_from_ratings(const mcgp_config *cfg, const mcgp_drivers *drv, const double *quali_rating,
                              const double *teammate_delta, const double *form_score,
                              const double *circuit_affinity, const int32_t *penalty, uint32_t n, uint64_t n_sims,
                              uint64_t sim_offset, uint64_t seed, int32_t device, uint64_t *hist_out,
                              double *grid_probs_out);

/* Elo updates of a whole season on the device ("next" row f4): the events of F1EloSystem.update_quali_ratings
 * (reference src/elo.py:45-83) and update_race_ratings (:85-122), applied in order in ONE kernel launch with the
 * ratings resident in LDS between events.  Per event e: kind[e] = 0 updates the qualifying ratings, 1 the race
 * ratings; k[e] = the K factor set_recency_weight (:13-38) leaves for it; count[e] = m entries of the result list,
 * who[e * n_drivers + j] = driver index of entry j, value[e * n_drivers + j] = its best lap time (qualifying) or
 * finishing position (race): lower wins, equal values tie.  Every entry's delta is the sum over the other entries,
 * in list order, of k (actual - expected) / (m - 1) with the ratings BEFORE the event; all deltas are applied
 * afterwards; m < 2 changes nothing (:54-56, :93-94).  ratings = [2][n_drivers] (qualifying row, race row), in and
 * out, with drivers not seen yet at the caller's initial rating (the reference creates them at that value on first
 * appearance, :59-61).  after_out (optional, NULL to skip) = [n_events][2][n_drivers], the ratings after each
 * event.  `10 ** exponent` is the library's own (csrc/elo_update.h): bit-identical to the CPU oracle's restatement
 * of the same text and within a few ulp of the reference's ratings.  MCGP_E_BAD_ARG: n_drivers out of [1, 32], an
 * entry count above n_drivers, a driver index >= n_drivers or listed twice in one event, a kind other than 0 / 1,
 * a non-finite k, value or rating. */
int32_t mcgp_elo_season(uint32_t n_drivers, uint32_t n_events, const int32_t *kind, const double *k,
                        const uint32_t *count, const uint8_t *who, const double *value, double *ratings,
                        double *after_out, int32_t device);

/* Measurement hooks (bench.py): duration in ms of the race kernel(s) of a call, from
 * hipEvents the library records on the call's launch stream around its launches
 * (the query synchronises on the stop event).  Every stream keeps its own pair of
 * events, so calls on different streams of one device do not disturb each other:
 *   mcgp_stream_kernel_ms  the most recent call launched on `stream` (NULL = the
 *                          default stream, which is where mcgp_run and
 *                          mcgp_simulate_race launch); the library remembers the 8
 *                          most recently used streams per device;
 *   mcgp_last_kernel_ms    the most recent call on `device` by any thread --
 *                          meaningful when one thread drives the device.
 * mcgp_last_launch_info / mcgp_last_kernel_name describe that same most recent call -- including the block SHAPE the
 * launch ended up with: the register kernel's default block fills a CU's LDS almost completely (163 264 of 163 840 B at
 * 20 cars); on a device or under a runtime that offers less per block the launch falls back, by itself, to the same
 * kernel in blocks of 4 waves (block_threads = 256, name "mcgp::race_kernel_reg<n, 4>"), same results, about 15 % slower.
 * If not even that block fits, the call fails with MCGP_E_HIP and a message that names both sizes. */
int32_t mcgp_last_kernel_ms(int32_t device, float *ms_out);
int32_t mcgp_stream_kernel_ms(int32_t device, void *stream, float *ms_out);
int32_t mcgp_last_launch_info(int32_t device, uint32_t *grid_blocks, uint32_t *block_threads,
                              uint32_t *lds_bytes);
const char *mcgp_last_kernel_name(int32_t device);   /* "" before the first launch */

#ifdef __cplusplus
}
#endif
#endif
