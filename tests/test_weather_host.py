"""Weather scenarios, host side: the C-ABI argument checks of mcgp_run_weather (no device needed), the struct layouts,
TrackChange, WeatherModel and run_weather's ValueErrors with the two-compound check, WeatherResult's helpers on hand-made
counts, and (on a device) the identity against run_strategies through the Python front."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
import weather_ref as WR
from monte_carlo_gp_amd import PitPlan, RaceConfig, StrategyResult, TrackChange, WeatherModel, WeatherResult
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, DEFAULT_WRONG_TYRE_SECONDS, RaceSimulator, _Problem

DRY, DAMP, WET = WR.DRY, WR.DAMP, WR.WET_TRACK
H = 2
inf, nan = float('inf'), float('nan')


# ---------------------------------------------------------------- the C ABI without a device
def _prob(n=3, laps=60, deviates=32):
    c = O.load_case('S60')
    cfg = dict(c['config'], total_laps=laps)
    return _Problem(RaceConfig(**cfg), [f'D{i:02d}' for i in range(n)], {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)


def _table(**cells):
    t = [[0.0] * 5 for _ in range(3)]
    for key, sec in cells.items():
        t[int(key[1])][int(key[2])] = sec
    return t


def _call(changes=((),), plans=None, table=None, n=3, laps=60, state=None, grid=True, n_sims=100, deviates=32, null=(),
          n_scenarios=None, fill=5, device=0):
    prob = _prob(n, laps, deviates)
    changes = list(changes)
    plans = list(plans) if plans is not None else [{}] * len(changes)
    counts, c_plans = SR.c_plans(plans)
    ccounts, c_ch = WR.c_changes(changes)
    model = WR.c_model(table)
    S = len(changes) if n_scenarios is None else n_scenarios
    g = np.full((max(n, 1), max(n, 1)), 1.0 / max(n, 1))
    cs = RR.c_state(*state) if state is not None else None
    h = np.full(max(S, 1) * n * n, fill, np.uint64)
    dl = np.full(max(S, 1) * n * (2 * n - 1), fill, np.uint64)
    wl = np.full(max(S, 1) * n * (laps + 1), fill, np.uint64)
    o = np.full(max(S, 1) * max(n_sims, 1) * n, fill, np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_weather(
        None if 'cfg' in null else C.byref(prob.cfg), C.byref(prob.drv),
        g.ctypes.data_as(C.POINTER(C.c_double)) if grid else None, C.byref(cs) if cs is not None else None, n, S,
        None if 'plan_count' in null else counts, None if 'plans' in null else c_plans,
        None if 'change_count' in null else ccounts, None if 'changes' in null else c_ch,
        None if 'model' in null else C.byref(model), n_sims, 0, 1, device,
        None if 'hist' in null else u64(h), u64(dl), u64(wl), o.ctypes.data_as(C.POINTER(C.c_uint8)))
    untouched = (h == fill).all() and (dl == fill).all() and (wl == fill).all() and (o == fill).all()
    return rc, N.lib().mcgp_last_error().decode(), untouched


def _state(n=3, lap=10):
    a = dict(cumulative_time=np.array([100.0 * lap + d for d in range(n)], np.float64),
             last_lap_time=np.full(n, 91.5, np.float64), grid_slot=np.arange(n, dtype=np.uint8),
             compound=np.full(n, 1, np.uint8), used_compounds=np.full(n, 0b011, np.uint8),
             tire_age=np.full(n, 7, np.int16), retired_lap=np.zeros(n, np.int16))
    return (a, lap, 0)


BAD = [
    (dict(changes=(), n_scenarios=0), 'n_scenarios must be in [1, 64]'),
    (dict(changes=([],) * 65), 'n_scenarios must be in [1, 64]'),
    (dict(changes=([], [(5, 5, 3)])), 'scenario 1, change 0: condition must be MCGP_DRY, MCGP_DAMP or MCGP_WET_TRACK'),
    (dict(changes=([(5, 5, -1)],)), 'scenario 0, change 0: condition must be'),
    (dict(changes=([(1, 5, DAMP)],)),
     "change 0: first_lap must be in [2, total_laps] (lap 1 has the configuration's condition)"),
    (dict(changes=([(0, 5, DAMP)],)), 'first_lap must be in [2, total_laps]'),
    (dict(changes=([(61, 61, DAMP)],)), 'first_lap must be in [2, total_laps]'),
    (dict(changes=([(2, 61, DAMP)],)), "change 0: last_lap must be in [2, total_laps] (lap 1 has the configuration's"),
    (dict(changes=([(5, 0, DAMP)],)), 'last_lap must be in [2, total_laps]'),
    (dict(changes=([(9, 8, DAMP)],)), 'scenario 0, change 0: first_lap must not be above last_lap'),
    (dict(changes=([(20, 25, DAMP)],), state=_state(lap=20), grid=False),
     "change 0: first_lap must be in [21, total_laps] (after the state's lap)"),
    (dict(changes=([(21, 61, DAMP)],), state=_state(lap=20), grid=False),
     "last_lap must be in [21, total_laps] (after the state's lap)"),
    (dict(changes=([(60, 60, DAMP)],), state=_state(lap=60), grid=False), 'first_lap must be in [61, total_laps]'),
    (dict(changes=([], [(5, 9, DAMP), (20, 30, WET), (9, 10, DRY)])),
     'scenario 1, change 2: first_lap..last_lap: lap 9 has two changes in this scenario'),
    (dict(changes=([(7, 7, DAMP), (7, 7, DAMP)],)), 'change 1: first_lap..last_lap: lap 7 has two changes'),
    (dict(changes=([], [(2 + k, 2 + k, DAMP) for k in range(65)]), laps=100), 'scenario 1: change_count must be in [0, 64]'),
    (dict(table=_table(c13=inf)), 'model: wrong_tyre_sec[1][3] must be finite and in [0, 60]'),
    (dict(table=_table(c00=nan)), 'model: wrong_tyre_sec[0][0] must be finite and in [0, 60]'),
    (dict(table=_table(c24=60.001)), 'model: wrong_tyre_sec[2][4] must be finite and in [0, 60]'),
    (dict(table=_table(c02=-0.001)), 'model: wrong_tyre_sec[0][2] must be finite and in [0, 60]'),
    (dict(plans=({1: (-1, 0, [(61, H)])},)), 'scenario 0, plan 0: stop 0: stop_lap must be in [2, total_laps]'),
    (dict(plans=({0: (5, 0, [(20, H)])},)), 'plan 0: start_compound must be -1 or in [MCGP_SOFT, MCGP_WET]'),
    (dict(plans=({0: (1, 0, [(20, H)])},), state=_state(), grid=False), 'a state fixes the tyres'),
    (dict(deviates=53), 'MCGP_DEVIATES_32'),
    (dict(null=('hist',)), 'hist_out is NULL'),
    (dict(null=('plan_count',)), 'plan_count is NULL'),
    (dict(null=('change_count',)), 'change_count is NULL'),
    (dict(null=('model',)), 'model is NULL'),
    (dict(plans=({0: (-1, 0, [(20, H)])},), null=('plans',)), 'plans is NULL'),
    (dict(changes=([(5, 5, DAMP)],), null=('changes',)), 'changes is NULL'),
    (dict(null=('cfg',)), 'cfg / drv is NULL'),
    (dict(grid=False), 'grid_probs is NULL'),
    (dict(state=_state()), 'grid_probs must be NULL when a state is given'),
    (dict(state=(dict(_state()[0], compound=np.array([7, 1, 1], np.uint8)), 10, 0), grid=False),
     'state 0: car 0: compound'),
    (dict(n=0), 'n must be in [1, 32]'),
    (dict(n=33), 'n must be in [1, 32]'),
    (dict(laps=1001), 'total_laps must be in [1, 1000]'),
]


@pytest.mark.parametrize('kw,msg', BAD, ids=[f'{i}: {m}' for i, (_, m) in enumerate(BAD)])
def test_library_rejects_bad_arguments_before_any_device_lookup(kw, msg):
    """MCGP_E_BAD_ARG naming the scenario, the change and the field, on a machine with or without a GPU (device 999 is
    never looked up: the checks come first), and the outputs keep their values."""
    rc, err, untouched = _call(device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert untouched


def test_limits_are_inclusive_and_zero_simulations_need_no_device():
    singles = [(2 + k, 2 + k, k % 3) for k in range(64)]
    ok = [
        dict(changes=([],) * 64),
        dict(changes=([(2, 60, DRY)],)),                    # the configuration's own condition
        dict(changes=([(2, 30, DAMP), (31, 60, WET)],), table=_table(c00=60.0, c24=60.0, c13=0.0)),
        dict(changes=(singles, [], singles), laps=100),
        dict(changes=([(30, 60, DAMP)],), plans=({2: (-1, 0, [(30, 3)])},)),
        dict(changes=([(11, 11, WET)],), state=_state(lap=10), grid=False),
        dict(changes=([(60, 60, DAMP)],), state=_state(lap=59), grid=False),
        dict(changes=([],), state=_state(lap=60), grid=False),              # nothing left to run or to change
        dict(null=('plans', 'changes')),                    # every count is 0
    ]
    for kw in ok:
        rc, err, untouched = _call(n_sims=0, device=999, **kw)
        assert rc == 0 and untouched, (kw, err)
    # 64 changes in each of 64 scenarios, 32 cars, 1000 laps
    rc, err, untouched = _call(changes=([(2 + 15 * k, 10 + 15 * k, k % 3) for k in range(64)],) * 64, n=32, laps=1000,
                               n_sims=0, device=999)
    assert rc == 0 and untouched, err
    # with simulations, a valid call gets past the checks to the device lookup
    rc, err, untouched = _call(changes=([(5, 60, DAMP)],), n_sims=10, device=999)
    assert rc == -2 and untouched, err


def test_structs_match_the_header():
    assert C.sizeof(N.McgpTrackChange) == 12 and C.sizeof(N.McgpWeatherModel) == 120
    assert [(f, getattr(N.McgpTrackChange, f).offset) for f, _ in N.McgpTrackChange._fields_] == [
        ('first_lap', 0), ('last_lap', 4), ('condition', 8)]
    m = WR.c_model([[10 * c + k for k in range(5)] for c in range(3)])
    assert list(np.ctypeslib.as_array(m.wrong_tyre_sec).ravel()) == [10 * c + k for c in range(3) for k in range(5)]
    with open(O.ROOT + '/include/mcgp.h') as f:
        header = f.read()
    assert '#define MCGP_MAX_SCENARIO_TRACK_CHANGES 64' in header and '#define MCGP_ABI_VERSION 6' in header
    assert 'typedef struct mcgp_track_change {' in header and 'double wrong_tyre_sec[3][5];' in header
    assert (N.MAX_SCENARIO_TRACK_CHANGES, N.MAX_WRONG_TYRE_SECONDS, N.TRACKS) == (64, 60.0, ('dry', 'damp', 'wet'))
    assert [N.TRACK_ID[t] for t in N.TRACKS] == [0, 1, 2]
    assert 'mcgp_run_weather' in N.EXPORTS and hasattr(N.lib(), 'mcgp_run_weather')


# ---------------------------------------------------------------- Python layer
def test_track_change_and_weather_model():
    c = TrackChange(30, 45, 'damp').c_struct(2, 57)
    assert (c.first_lap, c.last_lap, c.condition) == (30, 45, 1)
    assert TrackChange(57, 57, 'wet').c_struct(31, 57).condition == 2
    with pytest.raises(ValueError, match="condition must be 'dry', 'damp' or 'wet'"):
        TrackChange(3, 4, 'snow').c_struct()
    with pytest.raises(ValueError, match='must not be above'):
        TrackChange(9, 8, 'damp').c_struct()
    with pytest.raises(ValueError, match=r"laps must be in \[2, 57\] \(lap 1 has the configuration's condition\)"):
        TrackChange(1, 8, 'damp').c_struct(2, 57)
    with pytest.raises(ValueError, match=r'laps must be in \[2, 57\]'):
        TrackChange(50, 58, 'damp').c_struct(2, 57)
    with pytest.raises(ValueError, match="after the state's lap"):
        TrackChange(30, 40, 'damp').c_struct(31, 57)
    # the default table is the project's; a given one holds what it names and 0.0 elsewhere
    t = WeatherModel().table()
    assert t.shape == (3, 5) and t[0, :3].tolist() == [0.0] * 3 and t[1, 3] == 0.0 and t[2, 4] == 0.0
    assert all(t[N.TRACK_ID[c], N.COMPOUND_ID[k]] == s for c, row in DEFAULT_WRONG_TYRE_SECONDS.items() for k, s in row.items())
    assert (t[1:, :3] > 0).all() and (t[0, 3:] > 0).all() and (t[2, :3] > t[1, :3]).all()
    t = WeatherModel({'damp': {'SOFT': 2.5}}).table()
    assert t[1, 0] == 2.5 and t.sum() == 2.5
    assert not WeatherModel({}).table().any()
    m = WeatherModel({'wet': {'WET': 60.0}}).c_struct()
    assert m.wrong_tyre_sec[2][4] == 60.0 and m.wrong_tyre_sec[0][0] == 0.0
    for bad, msg in (({'snow': {}}, 'condition must be'), ({'dry': {'SLICK': 1.0}}, 'compound must be one of'),
                     ({'dry': {'SOFT': -1.0}}, 'finite and in'), ({'dry': {'SOFT': 61.0}}, 'finite and in'),
                     ({'dry': {'SOFT': nan}}, 'finite and in')):
        with pytest.raises(ValueError, match=msg):
            WeatherModel(bad).table()


def _sim():
    c = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=DEFAULT_SET_POP)
    args = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    return c, sim, list(c['grid_probs']), c['config']['total_laps'], args


def test_run_weather_value_errors_and_scenario_names():
    c, sim, d, L, args = _sim()
    kw = dict(grid_probs=c['grid_probs'], seed=1)
    with pytest.raises(ValueError, match="'x'.*lap 12 has two changes"):
        sim.run_weather(0, {'x': [TrackChange(10, 12, 'damp'), TrackChange(12, 20, 'wet')]}, None, None, *args, **kw)
    with pytest.raises(ValueError, match="'x'.*laps must be in"):
        sim.run_weather(0, {'x': [TrackChange(1, 3, 'damp')]}, None, None, *args, **kw)
    with pytest.raises(ValueError, match='laps must be in'):
        sim.run_weather(0, {'x': [TrackChange(5, L + 1, 'damp')]}, None, None, *args, **kw)
    with pytest.raises(ValueError, match="'x'.*condition must be"):
        sim.run_weather(0, {'x': [TrackChange(5, 6, 'hail')]}, None, None, *args, **kw)
    with pytest.raises(ValueError, match='at most 64 changes'):
        sim.run_weather(0, {'x': [TrackChange(2, 2, 'damp')] * 65}, None, None, *args, **kw)
    with pytest.raises(ValueError, match='finite and in'):
        sim.run_weather(0, {'x': []}, None, WeatherModel({'dry': {'SOFT': 99.0}}), *args, **kw)
    with pytest.raises(ValueError, match='not one of the drivers'):
        sim.run_weather(0, {'x': []}, {'x': [PitPlan('NOBODY', [(20, 'HARD')])]}, None, *args, **kw)
    with pytest.raises(ValueError, match='1 to 64 scenarios'):
        sim.run_weather(0, {}, None, None, *args, **kw)
    with pytest.raises(ValueError, match='exactly one of'):
        sim.run_weather(0, {'x': []}, None, None, *args, seed=1)
    # the names are the union of the two dicts, changes first; zero simulations need no device
    r = sim.run_weather(0, {'as forecast': [], 'rain': [TrackChange(30, L, 'damp')]},
                        {'rain': [PitPlan(d[0], [(30, 'INTERMEDIATE')])], 'plan only': [PitPlan(d[1], [(25, 'HARD')])]},
                        None, *args, **kw)
    assert r.names == ['as forecast', 'rain', 'plan only'] and r.n_simulations == 0 and isinstance(r, WeatherResult)
    assert r.hist.shape == (3, 20, 20) and r.delta.shape == (3, 20, 39) and r.wrong_laps.shape == (3, 20, L + 1)


def test_the_two_compound_check_applies_to_scenarios_that_stay_dry():
    c, sim, d, L, args = _sim()
    kw = dict(grid_probs=c['grid_probs'], seed=1)
    one = [PitPlan(d[0], [(30, 'SOFT')], start='SOFT')]             # one dry compound
    inter = [PitPlan(d[0], [(30, 'INTERMEDIATE')], start='SOFT')]
    # dry on every lap: no change, or changes that all say 'dry'
    for changes in ({'x': []}, {'x': [TrackChange(2, L, 'dry')]}, {'rain': [TrackChange(30, L, 'damp')], 'x': []}):
        with pytest.raises(ValueError, match="scenario 'x'.*one dry compound"):
            sim.run_weather(0, changes, {'x': one}, None, *args, **kw)
        with pytest.raises(ValueError, match="scenario 'x'.*one dry compound"):
            sim.run_weather(0, changes, {'x': inter}, None, *args, **kw)
        sim.run_weather(0, changes, {'x': one}, None, *args, allow_single_compound=True, **kw)
    # one wet lap waives it for that scenario
    sim.run_weather(0, {'x': [TrackChange(L, L, 'damp')]}, {'x': inter}, None, *args, **kw)
    sim.run_weather(0, {'x': [TrackChange(2, 2, 'wet')]}, {'x': one}, None, *args, **kw)
    # a wet race that dries for a while is not dry on every lap (lap 1 from the grid has the race's condition)
    sim.run_weather(0, {'x': [TrackChange(2, L, 'dry')]}, {'x': one}, None, *args, track_condition='damp', **kw)
    # from a state, a wet race that is dry on every lap still to run is checked
    from monte_carlo_gp_amd import RaceState
    state = RaceState.from_json({'lap': 20, 'cars': [
        {'driver': x, 'cumulative_time': 2000.0 + i, 'last_lap_time': 95.0, 'tire_compound': 'INTERMEDIATE', 'tire_age': 19,
         'used_compounds': ['INTERMEDIATE']} for i, x in enumerate(d)]})
    skw = dict(state=state, seed=1, track_condition='damp')
    with pytest.raises(ValueError, match='one dry compound'):
        sim.run_weather(0, {'x': [TrackChange(21, L, 'dry')]}, {'x': [PitPlan(d[0], [(30, 'SOFT')])]}, None, *args, **skw)
    sim.run_weather(0, {'x': [TrackChange(22, L, 'dry')]}, {'x': [PitPlan(d[0], [(30, 'SOFT')])]}, None, *args, **skw)
    sim.run_weather(0, {'x': [TrackChange(21, L, 'dry')]}, {'x': [PitPlan(d[0], [(30, 'SOFT'), (45, 'HARD')])]}, None, *args,
                    **skw)


def _result():
    """3 drivers, 2 scenarios, 10 simulations, 4 laps, hand-made."""
    hist = np.zeros((2, 3, 3), np.int64)
    hist[0] = [[5, 3, 2], [3, 4, 3], [2, 3, 5]]
    hist[1] = [[7, 2, 1], [2, 5, 3], [1, 3, 6]]
    delta = np.zeros((2, 3, 5), np.int64)
    delta[0, :, 2] = 10
    delta[1, 0] = [1, 3, 5, 1, 0]
    delta[1, 1] = [0, 1, 6, 3, 0]
    delta[1, 2] = [0, 2, 7, 1, 0]
    wrong = np.zeros((2, 3, 5), np.int64)
    wrong[:, :, 0] = 10
    wrong[1, 0] = [1, 4, 3, 2, 0]
    return WeatherResult(names=['as forecast', 'rain'], drivers=['A', 'B', 'C'], n_simulations=10, hist=hist, delta=delta,
                         wrong_laps=wrong)


def test_weather_result_helpers():
    r = _result()
    assert isinstance(r, StrategyResult)
    assert r.win_probability('rain', 'A') == pytest.approx(0.7)
    assert r.compare('rain', 'A')['p_better'] == pytest.approx(0.4)
    assert r.wrong_tyre_laps_distribution('rain', 'A').tolist() == [0.1, 0.4, 0.3, 0.2, 0.0]
    assert r.wrong_tyre_laps_distribution('rain', 'B').tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert r.expected_wrong_tyre_laps('rain', 'A') == pytest.approx(0.4 + 0.6 + 0.6)
    assert r.expected_wrong_tyre_laps('as forecast', 'A') == 0.0
    with pytest.raises(KeyError):
        r.wrong_tyre_laps_distribution('late', 'A')
    with pytest.raises(KeyError):
        r.expected_wrong_tyre_laps('rain', 'Z')


# ---------------------------------------------------------------- the identity, on a device
@pytest.mark.gpu
def test_run_weather_is_run_strategies_where_the_weather_changes_nothing(require_gpu):
    """Changes that all name the race's own condition, plans of the right class and a table that is zero where it is read:
    run_strategies' counts cell for cell, and every wrong_laps row in column 0."""
    c, sim, d, L, args = _sim()
    kw = dict(grid_probs=c['grid_probs'], seed=9, return_orders=True)
    plans = {'as is': [], 'early': [PitPlan(d[0], [(12, 'HARD')])], 'two': [PitPlan(d[3], [(15, 'MEDIUM'), (40, 'HARD')])]}
    want = sim.run_strategies(3000, plans, *args, **kw)
    model = WeatherModel({'damp': {'SOFT': 4.0, 'INTERMEDIATE': 1.0}, 'wet': {'WET': 2.0}, 'dry': {'INTERMEDIATE': 3.0, 'WET': 6.0}})
    changes = {'as is': [], 'early': [TrackChange(2, L, 'dry')], 'two': [TrackChange(10, 20, 'dry'), TrackChange(L, L, 'dry')]}
    got = sim.run_weather(3000, changes, plans, model, *args, **kw)
    assert got.names == want.names
    assert np.array_equal(got.hist, want.hist) and np.array_equal(got.delta, want.delta)
    assert np.array_equal(got.orders, want.orders)
    assert (got.wrong_laps[:, :, 0] == 3000).all() and not got.wrong_laps[:, :, 1:].any()
    # ... and rain is another race
    rain = sim.run_weather(3000, {'as is': [], 'rain': [TrackChange(30, L, 'damp')]}, None, model, *args, **kw)
    assert np.array_equal(rain.hist[0], want.hist[0]) and not np.array_equal(rain.hist[1], want.hist[0])
    assert rain.expected_wrong_tyre_laps('rain', d[0]) > 0.5
