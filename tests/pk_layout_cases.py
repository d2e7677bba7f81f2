"""Inputs of the pk-layout tests (tests/test_pk_layout_host_build.py, tests/test_gpu_pk_layout.py): n-car fields in which
every row of the register kernel's block-shared tables decides something, and the proof of that from the oracle's own trace.
Not a test module.

The tables the layout moves are gathered by fields of the pk word: the per-(compound, driver) entry {degradation, pit
threshold}, the per-compound pace delta beside the DRS gain, the live and the retired copy of the overtake pace, the pit
rule by regime and used-set.  A run exercises them when cars are on every compound (three runs per field size: a dry, a
damp and a wet track; the wet ones with the WET golden case's parameters), stop in every regime of the pit rule, retire
on lap 1 and later, run with DRS and without, run in dirty air, and meet an event lap."""
import functools

import numpy as np

import oracle_py as O

# field sizes of the tests: re-laid map and pair rows (4 .. 30, the largest with padding for them), re-laid map with the
# separate delta table (31, 32), the earlier map (2, 3: nothing packs; 9, 21: reg_pk_earlier_layout's list)
SIZES = (2, 3, 4, 9, 19, 20, 21, 22, 26, 30, 31, 32)
TRACKS = ('dry', 'damp', 'wet')
LAPS = 50


def field(n, track):
    """n cars, 50 laps, on a dry, damp or wet track: the WET golden case's configuration with retirements from lap 1 on,
    events every few races, and per-driver pace, spread, degradation (hence pit thresholds: stops on laps all over the
    race) and retirement rate."""
    base = O.load_case('WET')
    drivers = [f'D{i:02d}' for i in range(n)]
    teams = list(base['config']['dnf_rates'])
    case = dict(base, track_condition=track)
    # (shorter stints than the golden case's, so that also a two-car field stops in every regime of the pit rule)
    compounds = {c: dict(v, optimal_laps=opt) for (c, v), opt in zip(base['config']['tire_compounds'].items(), (9, 13, 17, 14, 16))}
    case['config'] = dict(base['config'], total_laps=LAPS, tire_compounds=compounds, driver_teams={d: teams[i % 10] for i, d in enumerate(drivers)},
                          sc_probability=0.03, vsc_probability=0.03, red_flag_probability=0.03,
                          dnf_rates={t: 0.01 for t in teams})
    g = np.random.default_rng(100 + n).random((n, n)) + 0.05
    case['grid_probs'] = {d: [float(x) for x in g[i]] for i, d in enumerate(drivers)}
    case['base_pace'] = {d: 90.0 + 0.11 * ((7 * i) % n) for i, d in enumerate(drivers)}
    case['tire_deg'] = {d: 0.01 + 0.1 * ((i * 0.381966) % 1.0) for i, d in enumerate(drivers)}       # (all three classes of :455-462)
    case['driver_variance'] = {d: 0.12 + 0.01 * (i % 9) for i, d in enumerate(drivers)}
    case['driver_dnf_rates'] = {d: 0.004 + 0.001 * (i % 5) for i, d in enumerate(drivers)}
    return case


def seed_of(n, track):
    return 1000 * n + TRACKS.index(track)


@functools.lru_cache(maxsize=None)
def reference(n, track, n_sims, deviates=32, sim_offset=0, n_trace=0):
    """The oracle's run of field(n, track), from the back-end of the deviate width; computed once, shared, not to be modified."""
    rng = O.RNG_PHILOX53 if deviates == 53 else O.RNG_PHILOX
    return O.Problem(field(n, track)).run(n_sims, rng=rng, seed=seed_of(n, track), sim_offset=sim_offset, want_orders=True,
                                          n_trace=n_trace)


def pit_regime(remaining_laps):
    """csrc/race_kernel_reg.hip.h pit_regime: the four regimes of the pit rule (reference :471-477, :485)."""
    return 0 if remaining_laps > 30 else 1 if remaining_laps > 20 else 2 if remaining_laps > 15 else 3


def what_the_run_shows(case, trace):
    """From the oracle's trace (arrays [simulation][lap - 1][driver], the state after the lap): the compounds cars ran on,
    the pit-rule regimes in which a car stopped, whether a car retired on lap 1 / later, ran with DRS / without, ran in
    dirty air, and whether some lap was an event lap."""
    age, comp, dnf, drs, tbl, dnf_lap = (trace[k] for k in ('age', 'comp', 'dnf', 'drs', 'tbl', 'dnf_lap'))
    L = age.shape[1]
    running = dnf == 0
    both = running[:, 1:] & running[:, :-1]                      # running after this lap and after the one before
    grew = both & (age[:, 1:] > age[:, :-1])
    reset = both & (age[:, 1:] == 0) & (age[:, :-1] > 0)
    # a stop: the car's tyres are new while another running car's grew older (a red flag renews every car's)
    stop = reset & (grew.sum(axis=2, keepdims=True) > 0)
    regimes = {pit_regime(L - (k + 2)) for k in np.nonzero(stop.any(axis=(0, 2)))[0]}      # index k = lap k + 2
    # an event lap: tyres saved behind the safety car (a running car's age stands still: a racing lap adds one, a stop
    # leaves zero), or every running car of at least two on new tyres at once (red flag)
    held = both & (age[:, 1:] == age[:, :-1]) & (age[:, 1:] > 0)
    all_new = (reset.sum(axis=2) >= 2) & (reset.sum(axis=2) == both.sum(axis=2))
    thr = float(case['config'].get('dirty_air_threshold', 2.0))
    return dict(compounds=set(np.unique(comp[running]).tolist()), regimes=regimes,
                retired_lap_1=bool((dnf_lap == 1).any()), retired_later=bool((dnf_lap > 1).any()),
                drs_on=bool((drs[running] == 1).any()), drs_off=bool((drs[running] == 0).any()),
                dirty_air=bool((running & (tbl > 0) & (tbl < thr)).any()), event_lap=bool(held.any() or all_new.any()))
