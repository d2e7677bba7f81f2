// race_kernel.hip.h -- the whole-race Monte Carlo kernel for CDNA4 (gfx950).
//
// One LANE runs one simulation (one full race: grid sampling, lap 1, laps 2..L,
// classification); a 64-lane wavefront therefore advances 64 independent races in
// lock step and every per-car quantity is a structure-of-arrays row in LDS:
//
//     cum [car][lane]  f64   cumulative race time        reference CarState.cumulative_time :20
//     last[car][lane]  f64   last lap time               reference CarState.last_lap_time   :29
//     pk  [car][lane]  u32   tyre age | compound | used compounds | grid slot | dnf | drs | dirty-air flag
//     ord [rank][lane] u8    driver index at time-rank r (ALL cars, stable by grid slot)
//
// "car" is the DRIVER index (row order of grid_probs), not the grid slot: with a
// counter-based RNG the per-car loops of the reference (src/simulation.py:186,284,450)
// carry no order dependence, so they run in time-rank order, which lets the
// dirty-air "car ahead" value (reference :179-183) ride along in a register.
// Row stride = blockDim.x, so lane l touches bank (2l mod 64) whatever car it
// indexes: every LDS access of the kernel, including the per-lane gathers by
// driver index, is bank-conflict free.
//
// Everything that orders cars follows Python's stable sort: key
// (cumulative_time, grid slot) -- reference :179,231,353,384,410,506,549 sort lists
// that are in grid order (Q1), so equal times keep grid order.
//
// The block protocol (run_block, over load_block), the start of a race (start_from_grid), the laps after lap 1
// (run_laps) and the classification (classify_and_count) are functions shared with the other race kernels of this
// family: race_resume_kernel (resume.hip.h) runs a race on from a mid-race state, race_trace_kernel (trace.hip.h) and
// race_gaps_kernel (gaps.hip.h) observe every lap, race_scenario_kernel (scenario.hip.h) plans the pit stops.  A kernel
// is its arguments and the lane body it hands run_block: sim id, start, run_laps, classify_and_count, its own output.
//
// Floating point: IEEE binary64 in the reference's evaluation order; this file
// is compiled with -ffp-contract=off.  The only fused operations are the three
// explicit binary32 fmaf of the inverse-normal cubic.
#pragma once
#include "race_common.hip.h"

namespace mcgp {

// pk word of THIS kernel (the register kernel has its own layout: k3* in race_kernel_reg.hip.h)
constexpr uint32_t kAgeMask = 0x3FFu;          // tyre age; lap of retirement once dnf is set
constexpr int kCompShift = 10;                 // 3 bits
constexpr int kUsedShift = 13;                 // 5 bits, one per compound
constexpr int kGposShift = 18;                 // 5 bits, grid slot
constexpr uint32_t kDnf = 1u << 23;
constexpr uint32_t kDrs = 1u << 24;
constexpr uint32_t kDirty = 1u << 25;          // 0 < time_behind_leader < dirty_air_threshold


// Per-lane view of the LDS rows.
struct Rows {
    double *cum;
    double *last;
    uint32_t *pk;
    uint8_t *ord;
    uint16_t *out;   // lap of the driver's retirement (laps >= 2), 0 = not in this race: drawn once per race
    int B;      // row stride (threads per block)
    int tid;
    __device__ __forceinline__ double &Cum(uint32_t d) const { return cum[d * B + tid]; }
    __device__ __forceinline__ double &Last(uint32_t d) const { return last[d * B + tid]; }
    __device__ __forceinline__ uint32_t &Pk(uint32_t d) const { return pk[d * B + tid]; }
    __device__ __forceinline__ uint8_t &Ord(int i) const { return ord[i * B + tid]; }
    __device__ __forceinline__ uint16_t &Out(uint32_t d) const { return out[d * B + tid]; }
};

__device__ __forceinline__ uint32_t gpos_of(uint32_t pk) { return (pk >> kGposShift) & 31u; }

// Stable sort of `ord` over ALL cars by (cumulative_time, grid slot): Python's
// sorted(cars, key=cumulative_time) on the grid-ordered list (reference :506).
// Restricted to running cars it is also the order of reference :179,231,353,384,410,549.
// Insertion sort: the field is nearly sorted from the previous lap.
__device__ __forceinline__ void sort_by_time(const Rows &s, int n)
{
    uint32_t dtop = s.Ord(0);
    double ktop = s.Cum(dtop);
    uint32_t gtop = gpos_of(s.Pk(dtop));
    for (int i = 1; i < n; ++i) {
        const uint32_t x = s.Ord(i);
        const double kx = s.Cum(x);
        const uint32_t gx = gpos_of(s.Pk(x));
        if (ktop > kx || (ktop == kx && gtop > gx)) {
            int j = i;
            s.Ord(j) = (uint8_t)dtop;
            --j;
            while (j > 0) {
                const uint32_t y = s.Ord(j - 1);
                const double ky = s.Cum(y);
                if (!(ky > kx || (ky == kx && gpos_of(s.Pk(y)) > gx))) break;
                s.Ord(j) = (uint8_t)y;
                --j;
            }
            s.Ord(j) = (uint8_t)x;
        } else {
            dtop = x; ktop = kx; gtop = gx;
        }
    }
}

// _update_positions, reference :538-560: gap to the leader (kept as the dirty-air
// predicate of reference :209-212) and the DRS flag.
__device__ __forceinline__ void update_positions(const Rows &s, int n, bool drs_allowed, double dirty_thr)
{
    bool first = true;
    double leader = 0.0, prev = 0.0;
    for (int i = 0; i < n; ++i) {
        const uint32_t d = s.Ord(i);
        uint32_t pk = s.Pk(d);
        if (pk & kDnf) continue;
        const double t = s.Cum(d);
        if (first) { leader = t; }
        const double tbl = t - leader;
        pk &= ~(kDrs | kDirty);
        if (tbl > 0 && tbl < dirty_thr) pk |= kDirty;
        if (!first && drs_allowed && (t - prev) < 1.0) pk |= kDrs;
        s.Pk(d) = pk;
        prev = t;
        first = false;
    }
}

// What the lap code reads besides the lane's rows: the block's LDS copies of the parameter block's tables, and its scalars.
struct LapEnv {
    const KParams *P;
    int n, L, track;
    const float4 *norm;
    const double *base, *factor, *deg, *var;
    const unsigned long long *dnf, *dnf1;
    const double *cdeg, *cdelta;
    const uint16_t *opt;
    double pit_loss, overtake_delta, drs_delta, dirty_thr, dirty_pen;
};

// The block's dynamic LDS: tables, histogram (kMaxCars^2 u32), then the per-lane rows (offsets are multiples of 16).
// Copies the tables in and zeroes the histogram -- the caller syncs before reading either --, sets the histogram and
// the lane's rows, and returns the lap code's view.
__device__ __forceinline__ LapEnv load_block(unsigned char *smem, const KParams *__restrict__ P, uint32_t *&s_hist, Rows &s)
{
    const int tid = threadIdx.x;
    const int B = blockDim.x;
    const int n = P->n;
    float4 *t_norm = reinterpret_cast<float4 *>(smem);
    double *t_base = reinterpret_cast<double *>(smem + kNormalRows * 16);
    double *t_factor = t_base + kMaxCars;
    double *t_deg = t_factor + kMaxCars;
    double *t_var = t_deg + kMaxCars;
    unsigned long long *t_dnf = reinterpret_cast<unsigned long long *>(t_var + kMaxCars);
    unsigned long long *t_dnf1 = t_dnf + kMaxCars;
    double *t_cdeg = reinterpret_cast<double *>(t_dnf1 + kMaxCars);
    double *t_cdelta = t_cdeg + kCompStride;
    uint16_t *t_opt = reinterpret_cast<uint16_t *>(t_cdelta + kCompStride);
    s_hist = reinterpret_cast<uint32_t *>(t_opt + kMaxCars * kCompStride);
    s.cum = reinterpret_cast<double *>(s_hist + kMaxCars * kMaxCars);
    s.last = s.cum + (size_t)n * B;
    s.pk = reinterpret_cast<uint32_t *>(s.last + (size_t)n * B);
    s.ord = reinterpret_cast<uint8_t *>(s.pk + (size_t)n * B);
    s.out = reinterpret_cast<uint16_t *>(s.ord + (size_t)n * B);
    s.B = B;
    s.tid = tid;

    for (int i = tid; i < kNormalRows * 4; i += B)
        reinterpret_cast<uint32_t *>(t_norm)[i] = P->normal_bits[i];
    for (int i = tid; i < kMaxCars; i += B) {
        t_base[i] = P->base_pace[i];
        t_factor[i] = P->factor[i];
        t_deg[i] = P->tire_deg[i];
        t_var[i] = P->variance[i];
        t_dnf[i] = P->t_dnf[i];
        t_dnf1[i] = P->t_dnf1[i];
    }
    for (int i = tid; i < kCompStride; i += B) {
        t_cdeg[i] = P->comp_deg[i];
        t_cdelta[i] = P->comp_delta[i];
    }
    for (int i = tid; i < kMaxCars * kCompStride; i += B) t_opt[i] = P->opt_laps[i];
    for (int i = tid; i < n * n; i += B) s_hist[i] = 0u;

    LapEnv e;
    e.P = P;
    e.n = n;
    e.L = P->total_laps;
    e.track = P->track;
    e.norm = t_norm;
    e.base = t_base;
    e.factor = t_factor;
    e.deg = t_deg;
    e.var = t_var;
    e.dnf = t_dnf;
    e.dnf1 = t_dnf1;
    e.cdeg = t_cdeg;
    e.cdelta = t_cdelta;
    e.opt = t_opt;
    e.pit_loss = P->pit_loss;
    e.overtake_delta = P->overtake_delta;
    e.drs_delta = P->drs_delta;
    e.dirty_thr = P->dirty_thr;
    e.dirty_pen = P->dirty_pen;
    return e;
}

// What a start hands run_laps: the first lap to run and the reference's drs_disabled_until before it.
struct RaceStart {
    int first_lap, drs_disabled_until;
};

// start_from_grid's hook for a car's starting tyres: the model's own (the call vanishes at compile time).
struct ModelTyres {
    __device__ __forceinline__ void operator()(uint32_t /*driver*/, uint32_t & /*comp*/, uint32_t & /*age*/) const {}
};

// The pace policy of every kernel but race_scenario_kernel with paces or weather: a car's base pace is the model's.  start_from_grid and run_laps
// ask a policy once per lap, begin_lap(lap) (wave-uniform), and wherever the model reads base_pace[d] -- lap 1's base_lap,
// the lap time of laps >= 2, the pace of the overtake passes (candidate scan and attempt probability) -- base(d, b) with
// b = base_pace[d], and use what it returns.  ModelPace returns b itself, so that the call vanishes; OffsetPace
// (paces.hip.h) adds the caller's lap-time offsets there, WeatherPace (weather.hip.h) the seconds of the car's compound
// under the lap's track condition.
struct ModelPace {
    __device__ __forceinline__ void begin_lap(int /*lap*/) {}
    __device__ __forceinline__ double base(uint32_t /*d*/, double b) const { return b; }
};

// _initialize_cars' tyres of the car on grid slot `pos` (0-based) under track condition `track`, reference :244-273.
__device__ __forceinline__ void start_tyres(int track, int pos, uint32_t &comp, uint32_t &age)
{
    if (track == 2) { comp = 4u; age = 0u; }
    else if (track == 1) { comp = 3u; age = 0u; }
    else { comp = pos < 10 ? 0u : 1u; age = pos < 10 ? 4u : 0u; }
}

// The grid policy of every kernel but race_scenario_kernel with grid edits: the cars start from the slots they drew.
// Where kEdits is set start_from_grid calls, after the sampling loop (pk holds every driver's drawn slot and its cars, ord
// the drawn order, cum 0), edit(s, n, track, hook), which may move the drivers to other slots and sets their cars up by
// the new slot, and, for every car that sets a lap time on lap 1, lap1(d, t) with t = 0.0 + lap_time, and stores what it
// returns.  ModelGrid has neither: both calls vanish at compile time.  GridEdits (grids.hip.h) is the caller's drops, pins
// and pit-lane starts.
struct ModelGrid {
    static constexpr bool kEdits = false;
    template <class StartHook>
    __device__ __forceinline__ void edit(const Rows &, int /*n*/, int /*track*/, StartHook) const {}
    __device__ __forceinline__ double lap1(uint32_t /*d*/, double t) const { return t; }
};

// The start of one lane's race: grid (`fixed_grid`, or NULL: sampled from grid_probs), cars, lap 1 and the once-per-race
// retirement draws.  Leaves the rows after update_positions of lap 1 and every driver's retirement lap (laps >= 2) in
// `out`.  hook(driver, comp, age) may replace a car's starting tyres after the model has picked them
// (race_scenario_kernel: PlannedTyres, strategy.hip.h).  `pace` gives lap 1's base pace (ModelPace: the model's), `grid`
// may move the drivers on the drawn grid (ModelGrid: never).
template <class StartHook = ModelTyres, class PacePolicy = ModelPace, class GridPolicy = ModelGrid>
__device__ __forceinline__ RaceStart start_from_grid(const Rows &s, const LapEnv &e, uint32_t c0, uint32_t c1,
                                                     uint32_t seed_lo, uint32_t seed_hi,
                                                     const uint8_t *__restrict__ fixed_grid, StartHook hook = StartHook(),
                                                     PacePolicy pace = PacePolicy(), GridPolicy grid = GridPolicy())
{
    const KParams *__restrict__ P = e.P;
    const int n = e.n, L = e.L, track = e.track;

    // ================= _sample_grid, reference :102-145 =================
    // probs / cdf scratch lives in the `last` rows (not needed until lap 2).
    {
        uint32_t remaining = (n >= 32) ? 0xffffffffu : ((1u << n) - 1u);
        int n_remaining = n;
        uint32_t g0 = 0, g1 = 0, g2 = 0, g3 = 0;
        for (int pos = 0; pos < n; ++pos) {
            uint32_t sel;
            if (fixed_grid) {
                sel = fixed_grid[pos];
            } else {
                if ((pos & 3) == 0)
                    philox4x32_10(c0, c1, 0u, kPurposeGrid | (uint32_t)(pos >> 2), seed_lo, seed_hi, g0, g1, g2, g3);
                const uint32_t gw = (pos & 3) == 0 ? g0 : (pos & 3) == 1 ? g1 : (pos & 3) == 2 ? g2 : g3;
                const double u = u32_to_unit(gw);
                double total = 0.0;                                   // :119-123
                for (int d = 0; d < n; ++d) {
                    const double p = ((remaining >> d) & 1u) ? P->grid_probs[d * n + pos] : 0.0;
                    total = total + p;
                }
                double prob_sum = 0.0;                                // :125-133
                for (int d = 0; d < n; ++d) {
                    const bool rem = (remaining >> d) & 1u;
                    double p;
                    if (total > 0) p = (rem ? P->grid_probs[d * n + pos] : 0.0) / total;
                    else p = rem ? 1.0 / (double)n_remaining : 0.0;
                    s.Last(d) = p;
                    prob_sum = prob_sum + p;
                }
                const bool renorm = prob_sum > 0 && fabs(prob_sum - 1.0) > 1e-9;   // :134-135
                // np.random.choice: cdf = cumsum(p); cdf /= cdf[-1]; searchsorted(u, 'right')
                double acc = 0.0;
                for (int d = 0; d < n; ++d) {
                    double p = s.Last(d);
                    if (renorm) p = p / prob_sum;
                    acc = (d == 0) ? p : acc + p;
                    s.Last(d) = acc;
                }
                const double cdf_last = acc;
                sel = 0;
                for (int d = 0; d < n; ++d)
                    if (s.Last(d) / cdf_last <= u) sel = (uint32_t)d + 1u;
                if (sel >= (uint32_t)n) sel = (uint32_t)n - 1u;       // unreachable: cdf[-1] == 1 > u
            }
            if ((remaining >> sel) & 1u) { remaining &= ~(1u << sel); --n_remaining; }
            // _initialize_cars, reference :244-273
            uint32_t comp, age;
            start_tyres(track, pos, comp, age);
            hook(sel, comp, age);
            s.Pk(sel) = age | (comp << kCompShift) | ((1u << comp) << kUsedShift) | ((uint32_t)pos << kGposShift);
            s.Cum(sel) = 0.0;
            s.Ord(pos) = (uint8_t)sel;
        }
        for (int d = 0; d < n; ++d) s.Last(d) = 0.0;
    }
    if constexpr (GridPolicy::kEdits) grid.edit(s, n, track, hook);

    // ================= _simulate_lap_1, reference :275-311 =================
    pace.begin_lap(1);
    for (int pos = 0; pos < n; ++pos) {
        const uint32_t d = s.Ord(pos);
        uint32_t pk = s.Pk(d);
        uint32_t w0, w1, w2, w3;
        philox4x32_10(c0, c1, 1u, kPurposeCar | d, seed_lo, seed_hi, w0, w1, w2, w3);
        if ((uint64_t)w0 < e.dnf1[d]) {
            s.Pk(d) = (pk & ~kAgeMask) | kDnf | 1u;
            continue;
        }
        const uint32_t comp = (pk >> kCompShift) & 7u;
        const uint32_t age = pk & kAgeMask;
        const double eff = e.cdeg[comp] * e.factor[d];
        const double tire = (double)age * eff;
        const double fuel_effect = (110.0 - 110.0) * 0.03;
        const double noise = 0.0 + e.var[d] * (double)normal_from_u32(w1, e.norm);
        const double base_lap = pace.base(d, e.base[d]) + tire - fuel_effect + e.cdelta[comp] - 0.0 + noise;
        double pf = 0.5 + (double)(pos + 1) * 0.1;
        if (!(pf < 1.5)) pf = 1.5;
        double sd = 0.0 + pf * (double)normal_from_u32(w2, e.norm);
        if (pos + 1 <= 3 && 1.0 < sd) sd = 1.0;
        const double lap_time = base_lap - sd * 0.5;
        s.Cum(d) = grid.lap1(d, 0.0 + lap_time);
        s.Pk(d) = (pk & ~kAgeMask) | (age + 1u);
    }
    sort_by_time(s, n);
    update_positions(s, n, false, e.dirty_thr);

    // ================= retirements of laps 2..L (:190-197), drawn once per race: race_common.hip.h =================
    {
        uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
        for (int d = 0; d < n; ++d) {
            if ((d & 3) == 0)
                philox4x32_10(c0, c1, 0u, kPurposeRetire | (uint32_t)(d >> 2), seed_lo, seed_hi, r0, r1, r2, r3);
            const uint32_t rw = (d & 3) == 0 ? r0 : (d & 3) == 1 ? r1 : (d & 3) == 2 ? r2 : r3;
            s.Out(d) = (uint16_t)draw_retirement_lap(rw, e.dnf[d], L);
        }
    }
    return {2, 0};
}

// Race events of a lap, as run_laps hands them to its observer: the outcome of the short-circuit chain of :168-176.
constexpr int kEventNone = 0, kEventRed = 1, kEventSc = 2, kEventVsc = 3;

// The per-lap observer of race_kernel and race_resume_kernel: nothing (the call vanishes at compile time).
struct NoLapObserver {
    __device__ __forceinline__ void operator()(const Rows &, int /*lap*/, int /*event*/) {}
};

// The pit policy of race_kernel, race_resume_kernel and race_trace_kernel: the race model's own rule for every car.
// run_laps asks a policy once per lap, begin_lap(lap) (wave-uniform), and once per running car and lap, after the
// car's lap time, decide(d, newc): -1 = the rule decides (_handle_pit_stops, reference :454-492); 0 = no stop and the
// rule is off; 1 = a stop onto compound `newc`, rule off.  RulePit's constant -1 folds the branch away.  After the pit
// step of every running car, after_pit(d, stopped, t) sees the car's new cumulative time and returns what is stored:
// `t` itself here and in PlanPit, so that the call vanishes; ScenarioPit (scenario.hip.h) adds time penalties there.
struct RulePit {
    __device__ __forceinline__ void begin_lap(int /*lap*/) {}
    __device__ __forceinline__ int decide(uint32_t /*d*/, uint32_t & /*newc*/) const { return -1; }
    __device__ __forceinline__ double after_pit(uint32_t /*d*/, bool /*stopped*/, double t) const { return t; }
};

// The event policy of every kernel but race_scenario_kernel with events: each lap's event is drawn.  run_laps asks a policy once per
// lap, at a wave-uniform point before the event step, at(lap): -1 = the short-circuit chain decides, as drawn; a kEvent*
// = that outcome replaces the chain's, whatever the lap's event words say (ForcedEvents, events.hip.h).  DrawnEvents'
// constant -1 folds the test away.
struct DrawnEvents {
    __device__ __forceinline__ int at(int /*lap*/) const { return -1; }
};

// The track policy of every kernel but race_scenario_kernel with weather: the track condition is the race's own on every
// lap.  run_laps asks a policy once per lap, begin_lap(lap, track) (wave-uniform) with the parameter block's condition,
// and uses what it returns wherever that lap's code reads the condition: the red flag's and the rule stop's
// stint_compound and the rule stop's two-compound waiver.  Once per running car and lap, where the lap time is computed,
// lap_time_on(d, comp) sees the compound it is computed on and says whether a car under the model's rule has to stop
// for the other class of tyres.  ModelTrack returns `track` itself and a constant false, so that both calls vanish;
// WeatherTrack (weather.hip.h) reads the caller's condition of the lap.
struct ModelTrack {
    __device__ __forceinline__ int begin_lap(int /*lap*/, int track) { return track; }
    __device__ __forceinline__ bool lap_time_on(uint32_t /*d*/, uint32_t /*comp*/) const { return false; }
};

// Laps first_lap .. L of one lane's race, reference :166-228, from the state the rows hold after lap first_lap - 1: `ord`
// sorted by (cumulative time, grid slot), the DRS / dirty-air flags of update_positions, the retirement laps in `out`,
// and the reference's drs_disabled_until.  race_kernel runs it from lap 2, race_resume_kernel (resume.hip.h) from k + 1.
// After update_positions of every lap, obs(s, lap, event) sees the rows and the lap's kEvent* (race_trace_kernel,
// trace.hip.h, records them; the other kernels pass a NoLapObserver).  `pit` decides the stops (RulePit: the model's
// rule; race_scenario_kernel, scenario.hip.h, passes a ScenarioPit: planned stops and, by rule set, time penalties).
// `evp` may replace a lap's event (DrawnEvents: never; with events the scenario kernel passes ForcedEvents, the
// caller's overrides).  `pace` gives a car's base pace on a lap (ModelPace: the model's; with paces it passes OffsetPace,
// the caller's lap-time offsets; with weather WeatherPace).  `trk` gives a lap's track condition (ModelTrack: the
// race's; with weather it passes WeatherTrack, the caller's condition by lap).
template <class LapObserver, class PitPolicy = RulePit, class EventPolicy = DrawnEvents, class PacePolicy = ModelPace,
          class TrackPolicy = ModelTrack>
__device__ __forceinline__ void run_laps(const Rows &s, const LapEnv &e, uint32_t c0, uint32_t c1, uint32_t seed_lo,
                                         uint32_t seed_hi, int first_lap, int drs_disabled_until, LapObserver &obs,
                                         PitPolicy pit = PitPolicy(), EventPolicy evp = EventPolicy(),
                                         PacePolicy pace = PacePolicy(), TrackPolicy trk = TrackPolicy())
{
    const KParams *__restrict__ P = e.P;
    const int n = e.n, L = e.L, race_track = e.track;
    const float4 *t_norm = e.norm;
    const double *t_base = e.base, *t_factor = e.factor, *t_deg = e.deg, *t_var = e.var;
    const double *t_cdeg = e.cdeg, *t_cdelta = e.cdelta;
    const uint16_t *t_opt = e.opt;
    const double pit_loss = e.pit_loss, overtake_delta = e.overtake_delta, drs_delta = e.drs_delta;
    const double dirty_thr = e.dirty_thr, dirty_pen = e.dirty_pen;
    for (int lap = first_lap; lap <= L; ++lap) {
        const int remaining_laps = L - lap;
        int event = kEventNone;
        const int track = trk.begin_lap(lap, race_track);
        pace.begin_lap(lap);
        // ---- race-interrupting events, :168-176 (short-circuit chain, Q8) ----
        {
            uint32_t e0, e1, e2, e3;
            philox4x32_10(c0, c1, (uint32_t)lap, kPurposeEvent, seed_lo, seed_hi, e0, e1, e2, e3);
            const int forced = evp.at(lap);
            const bool red = forced < 0 ? (uint64_t)e0 < P->t_red : forced == kEventRed;
            const bool sc = forced < 0 ? !red && (uint64_t)e1 < P->t_sc : forced == kEventSc;
            const bool vsc = forced < 0 ? !red && !sc && (uint64_t)e2 < P->t_vsc : forced == kEventVsc;
            event = red ? kEventRed : sc ? kEventSc : vsc ? kEventVsc : kEventNone;
            if (red || sc || vsc) {
                // _handle_red_flag :397-431 / _handle_safety_car :334-376 / _handle_vsc :378-395
                const bool dec_age = sc || (vsc && (uint64_t)e3 < P->t_vsc_tire);
                const uint32_t newc = stint_compound(track, remaining_laps);
                int k = 0;
                double leader = 0.0, prev_nt = -1.0;
                bool tie = false;
                for (int i = 0; i < n; ++i) {
                    const uint32_t d = s.Ord(i);
                    uint32_t pk = s.Pk(d);
                    if (pk & kDnf) continue;
                    const double t = s.Cum(d);
                    if (k == 0) leader = t;
                    double nt;
                    if (red) nt = leader + (double)k * 0.1;
                    else if (sc) nt = leader + (double)k * 0.5;
                    else { const double gap = t - leader; nt = leader + gap * 0.8; }
                    tie |= nt == prev_nt;
                    prev_nt = nt;
                    const double tbl = nt - leader;
                    pk &= ~kDirty;
                    if (tbl > 0 && tbl < dirty_thr) pk |= kDirty;
                    uint32_t age = pk & kAgeMask;
                    if (red) {
                        age = 0u;
                        pk = (pk & ~(7u << kCompShift)) | (newc << kCompShift) | ((1u << newc) << kUsedShift);
                    } else if (dec_age) {
                        age = age > 0u ? age - 1u : 0u;
                    }
                    pk = (pk & ~kAgeMask) | age;
                    s.Cum(d) = nt;
                    s.Pk(d) = pk;
                    ++k;
                }
                drs_disabled_until = lap + (vsc ? 1 : 2);
                // x0.8 is monotone but may round two gaps together: equal times fall back to grid order.  Otherwise
                // the field order (`ord`, which also addresses this lap's draws) stays what the last lap left.
                if (tie) sort_by_time(s, n);
            }
        }

        // ---- every running car's lap, :179-223, with the pit stop of :433-494 folded in ----
        {
            pit.begin_lap(lap);
            double fuel = 110.0 - 1.5 * (double)(lap - 1);     // fuel_load before this lap (Q7)
            if (!(fuel > 0)) fuel = 0.0;
            const double fuel_effect = (110.0 - fuel) * 0.03;
            double carry = 0.0;                                 // car_ahead_times.get(driver, 0)
            for (int i = 0; i < n; ++i) {
                const uint32_t d = s.Ord(i);
                uint32_t pk = s.Pk(d);
                if (pk & kDnf) continue;
                const double ahead_last = carry;
                carry = s.Last(d);
                if ((int)s.Out(d) == lap) {                     // :194-197, drawn before the race
                    s.Pk(d) = (pk & ~kAgeMask) | kDnf | (uint32_t)lap;
                    continue;
                }
                uint32_t w0, w1, w2, w3;
                // the lap noise is addressed by the car's place i in the field order: one block serves places 4j .. 4j+3
                philox4x32_10(c0, c1, (uint32_t)lap, kPurposeCar | ((uint32_t)i >> 2), seed_lo, seed_hi, w0, w1, w2, w3);
                const uint32_t w1x = (i & 3) == 0 ? w0 : (i & 3) == 1 ? w1 : (i & 3) == 2 ? w2 : w3;
                w1 = w1x;
                uint32_t comp = (pk >> kCompShift) & 7u;
                uint32_t age = pk & kAgeMask;
                // _calculate_lap_time :313-332
                const double eff = t_cdeg[comp] * t_factor[d];
                const double tire = (double)age * eff;
                const double drs_gain = (pk & kDrs) ? drs_delta : 0.0;
                const double noise = 0.0 + t_var[d] * (double)normal_from_u32(w1, t_norm);
                const double clean = pace.base(d, t_base[d]) + tire - fuel_effect + t_cdelta[comp] - drs_gain + noise;
                double lap_time = clean;
                if ((pk & kDirty) && ahead_last > 0) {          // :209-216
                    const double dirty_time = clean + dirty_pen;
                    lap_time = ahead_last > dirty_time ? ahead_last : dirty_time;
                }
                double t = s.Cum(d) + lap_time;
                age += 1u;
                const bool wrong = trk.lap_time_on(d, comp);
                // _handle_pit_stops :454-492 (no randomness, no cross-car dependence), or the policy's planned stop
                uint32_t plan_c = 0u;
                const int plan = pit.decide(d, plan_c);
                bool stopped = false;
                if (plan < 0 ? (((int)age > (int)t_opt[d * kCompStride + comp] || wrong) && remaining_laps > 5) : plan > 0) {
                    stopped = true;
                    t = t + pit_loss;
                    uint32_t newc;
                    if (plan > 0) {
                        newc = plan_c;
                    } else {
                        newc = stint_compound(track, remaining_laps);
                        const uint32_t used_dry = (pk >> kUsedShift) & 7u;
                        if (track == 0 && __popc(used_dry) == 1 && ((used_dry >> newc) & 1u)) {
                            const uint32_t avail = 7u & ~used_dry;
                            const uint32_t popped = avail == 5u ? (uint32_t)P->pop_sh : avail == 6u ? (uint32_t)P->pop_mh : 0u;
                            if (remaining_laps > 20) newc = (avail & 2u) ? 1u : popped;
                            else newc = (avail & 1u) ? 0u : popped;
                        }
                    }
                    comp = newc;
                    pk = (pk & ~(7u << kCompShift)) | (comp << kCompShift) | ((1u << comp) << kUsedShift);
                    age = 0u;
                }
                t = pit.after_pit(d, stopped, t);
                s.Cum(d) = t;
                s.Last(d) = lap_time;
                s.Pk(d) = (pk & ~kAgeMask) | age;
            }
        }

        // ---- _simulate_overtakes, :496-536 ----
        bool need_sort = true;
        for (int pass = 0; pass < 3; ++pass) {
            sort_by_time(s, n);
            need_sort = false;
            // adjacent pairs that attempt a pass: neither retired, pace delta over the threshold.
            uint32_t cand = 0u;
            {
                uint32_t dp = s.Ord(0);
                uint32_t pkp = s.Pk(dp);
                double pace_p = pace.base(dp, t_base[dp]) + (double)(pkp & kAgeMask) * t_deg[dp];
                for (int i = 1; i < n; ++i) {
                    const uint32_t d = s.Ord(i);
                    const uint32_t pk = s.Pk(d);
                    const double pace_d = pace.base(d, t_base[d]) + (double)(pk & kAgeMask) * t_deg[d];
                    double delta = pace_p - pace_d;
                    if (pk & kDrs) delta += drs_delta;
                    if (!((pk | pkp) & kDnf) && delta > overtake_delta) cand |= 1u << i;
                    pkp = pk;
                    pace_p = pace_d;
                }
            }
            if (cand == 0u) break;
            bool success = false;
            uint32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0;
            for (uint32_t k = 0; cand != 0u; ++k) {
                if ((k & 3u) == 0u)
                    philox4x32_10(c0, c1, (uint32_t)lap, kPurposeOvt | ((uint32_t)(8 * pass) + (k >> 2)),
                                  seed_lo, seed_hi, o0, o1, o2, o3);
                const uint32_t ow = (k & 3u) == 0u ? o0 : (k & 3u) == 1u ? o1 : (k & 3u) == 2u ? o2 : o3;
                const int i = __ffs((int)cand) - 1;
                cand &= cand - 1u;
                const uint32_t db = s.Ord(i), da = s.Ord(i - 1);
                const uint32_t pkb = s.Pk(db), pka = s.Pk(da);
                const double pace_b = pace.base(db, t_base[db]) + (double)(pkb & kAgeMask) * t_deg[db];
                const double pace_a = pace.base(da, t_base[da]) + (double)(pka & kAgeMask) * t_deg[da];
                double delta = pace_a - pace_b;
                if (pkb & kDrs) delta += drs_delta;
                double prob = delta / 2.0;
                if (!(prob < 0.5)) prob = 0.5;
                if (u32_to_unit(ow) < prob) {
                    double nb = s.Cum(da) - 0.1;
                    if (!(nb > 0.1)) nb = 0.1;
                    s.Cum(db) = nb;
                    s.Cum(da) = nb + 0.3;
                    success = true;
                }
            }
            if (!success) break;
            need_sort = true;
        }
        if (need_sort) sort_by_time(s, n);
        update_positions(s, n, lap > 2 && lap > drs_disabled_until, dirty_thr);   // :227-228
        obs(s, lap, event);
    }
}

// Classification, reference :230-242, of one lane's race, and its count: running cars by time, then retired cars by
// (lap, time) descending, stable -- `ord` insertion-sorted in place with that comparator --; then one count per
// (driver, position) into the block's LDS histogram and, unless `order` is NULL, the order into order[0 .. n).
__device__ __forceinline__ void classify_and_count(const Rows &s, int n, uint32_t *s_hist, uint8_t *__restrict__ order)
{
    for (int i = 1; i < n; ++i) {
        const uint32_t x = s.Ord(i);
        const uint32_t pkx = s.Pk(x);
        const double kx = s.Cum(x);
        int j = i;
        while (j > 0) {
            const uint32_t y = s.Ord(j - 1);
            const uint32_t pky = s.Pk(y);
            bool y_after_x;   // does y classify behind x?
            if (!(pky & kDnf)) {
                // y running: it is ahead of every retired car; among runners `ord` is already sorted
                y_after_x = false;
            } else if (!(pkx & kDnf)) {
                y_after_x = true;          // retired behind running
            } else {
                const uint32_t ly = pky & kAgeMask, lx = pkx & kAgeMask;
                const double ky = s.Cum(y);
                // descending (lap, time); ties keep grid order
                y_after_x = ly < lx || (ly == lx && (ky < kx || (ky == kx && gpos_of(pky) > gpos_of(pkx))));
            }
            if (!y_after_x) break;
            s.Ord(j) = (uint8_t)y;
            --j;
        }
        s.Ord(j) = (uint8_t)x;
    }
    for (int p = 0; p < n; ++p) {
        const uint32_t d = s.Ord(p);
        atomicAdd(&s_hist[d * n + p], 1u);                       // reference :93-94
        if (order) order[p] = (uint8_t)d;
    }
}

// The block protocol of every race kernel of this family: the dynamic LDS is loaded (load_block), the block's batches
// of blockDim.x simulations are dealt out by block index, grid-stride, lane(s, e, s_hist, local) runs simulation `local`
// of the launch's n_sims in this lane's rows, and the block's u32 LDS histogram goes to hist [n][n] with u64 atomics.
template <class Lane>
__device__ __forceinline__ void run_block(const KParams *__restrict__ P, uint64_t n_sims, uint32_t n_batches,
                                          unsigned long long *__restrict__ hist, Lane lane)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x;
    const int B = blockDim.x;
    uint32_t *s_hist;
    Rows s;
    const LapEnv e = load_block(smem, P, s_hist, s);
    __syncthreads();

    for (uint32_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
        const uint64_t local = (uint64_t)batch * (uint64_t)B + (uint64_t)tid;
        if (local >= n_sims) continue;      // tail lanes idle; no barrier inside the loop
        lane(s, e, s_hist, local);
    }

    __syncthreads();
    for (int i = tid; i < e.n * e.n; i += B) {
        const uint32_t c = s_hist[i];
        if (c) atomicAdd(&hist[i], (unsigned long long)c);
    }
}

__global__ void __launch_bounds__(512)
race_kernel(const KParams *__restrict__ P, uint64_t n_sims, uint64_t sim_offset,
            uint32_t seed_lo, uint32_t seed_hi, unsigned long long *__restrict__ hist,
            uint8_t *__restrict__ orders, const uint8_t *__restrict__ fixed_grid, uint32_t n_batches,
            uint32_t * /*ticket: the register kernel's work counter; batches are dealt out by block index here*/,
            uint32_t * /*retire_ws: the register kernel's retirement lists; an LDS row per driver here*/)
{
    run_block(P, n_sims, n_batches, hist, [=](const Rows &s, const LapEnv &e, uint32_t *s_hist, uint64_t local) {
        const uint64_t sim = sim_offset + local;
        const uint32_t c0 = (uint32_t)sim, c1 = (uint32_t)(sim >> 32);
        const RaceStart at = start_from_grid(s, e, c0, c1, seed_lo, seed_hi, fixed_grid);
        NoLapObserver none;
        run_laps(s, e, c0, c1, seed_lo, seed_hi, at.first_lap, at.drs_disabled_until, none);        // reference :166-228
        classify_and_count(s, e.n, s_hist, orders ? orders + local * (uint64_t)e.n : nullptr);      // reference :230-242
    });
}

}  // namespace mcgp
