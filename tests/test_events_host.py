"""Event scenarios, host side: the C-ABI argument checks of mcgp_run_events (no device needed), the mcgp_lap_event
layout, RaceEvent and run_events' ValueErrors, EventResult's helpers on hand-made counts and the `events` CLI's parsing and
output with a stand-in predictor."""
import ctypes as C
import json

import numpy as np
import pytest

import events_ref as ER
import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
from cli_cases import event_result as _result
from monte_carlo_gp_amd import EventResult, PitPlan, RaceConfig, RaceEvent, StrategyResult, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, RaceSimulator, _Problem

NONE, RED, SC, VSC = ER.NONE, ER.RED, ER.SC, ER.VSC
H = 2


# ---------------------------------------------------------------- the C ABI without a device
def _prob(n=3, laps=60, deviates=32):
    c = O.load_case('S60')
    cfg = dict(c['config'], total_laps=laps)
    return _Problem(RaceConfig(**cfg), [f'D{i:02d}' for i in range(n)], {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)


def _call(events=((),), plans=None, n=3, laps=60, state=None, grid=True, n_sims=100, deviates=32, null=(),
          n_scenarios=None, fill=5, device=0):
    prob = _prob(n, laps, deviates)
    events = list(events)
    plans = list(plans) if plans is not None else [{}] * len(events)
    counts, c_plans = SR.c_plans(plans)
    ecounts, c_evs = ER.c_events(events)
    S = len(events) if n_scenarios is None else n_scenarios
    g = np.full((max(n, 1), max(n, 1)), 1.0 / max(n, 1))
    cs = RR.c_state(*state) if state is not None else None
    h = np.full(max(S, 1) * n * n, fill, np.uint64)
    dl = np.full(max(S, 1) * n * (2 * n - 1), fill, np.uint64)
    ev = np.full(max(S, 1) * 3 * (laps + 1), fill, np.uint64)
    o = np.full(max(S, 1) * max(n_sims, 1) * n, fill, np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_events(
        None if 'cfg' in null else C.byref(prob.cfg), C.byref(prob.drv),
        g.ctypes.data_as(C.POINTER(C.c_double)) if grid else None, C.byref(cs) if cs is not None else None, n, S,
        None if 'plan_count' in null else counts, None if 'plans' in null else c_plans,
        None if 'event_count' in null else ecounts, None if 'events' in null else c_evs, n_sims, 0, 1, device,
        None if 'hist' in null else u64(h), u64(dl), u64(ev), o.ctypes.data_as(C.POINTER(C.c_uint8)))
    untouched = (h == fill).all() and (dl == fill).all() and (ev == fill).all() and (o == fill).all()
    return rc, N.lib().mcgp_last_error().decode(), untouched


def _state(n=3, lap=10):
    a = dict(cumulative_time=np.array([100.0 * lap + d for d in range(n)], np.float64),
             last_lap_time=np.full(n, 91.5, np.float64), grid_slot=np.arange(n, dtype=np.uint8),
             compound=np.full(n, 1, np.uint8), used_compounds=np.full(n, 0b011, np.uint8),
             tire_age=np.full(n, 7, np.int16), retired_lap=np.zeros(n, np.int16))
    return (a, lap, 0)


BAD = [
    (dict(events=(), n_scenarios=0), 'n_scenarios must be in [1, 64]'),
    (dict(events=([],) * 65), 'n_scenarios must be in [1, 64]'),
    (dict(events=([], [(5, 5, 4)])), 'scenario 1, event 0: kind must be MCGP_EVT_NONE'),
    (dict(events=([(5, 5, -1)],)), 'scenario 0, event 0: kind must be'),
    (dict(events=([(5, 6, SC), (9, 8, VSC)],)), 'scenario 0, event 1: first_lap must not be above last_lap'),
    (dict(events=([(1, 5, SC)],)), 'event 0: first_lap must be in [2, total_laps] (lap 1 has no event)'),
    (dict(events=([(0, 0, NONE)],)), 'first_lap must be in [2, total_laps] (lap 1 has no event)'),
    (dict(events=([(61, 61, RED)],)), 'first_lap must be in [2, total_laps]'),
    (dict(events=([(2, 61, NONE)],)), 'event 0: last_lap must be in [2, total_laps] (lap 1 has no event)'),
    (dict(events=([(5, 1, NONE)],)), 'last_lap must be in [2, total_laps]'),
    (dict(events=([(20, 25, SC)],), state=_state(lap=20), grid=False),
     'event 0: first_lap must be in [21, total_laps] (after the state\'s lap)'),
    (dict(events=([(21, 61, SC)],), state=_state(lap=20), grid=False),
     'last_lap must be in [21, total_laps] (after the state\'s lap)'),
    (dict(events=([(60, 60, SC)],), state=_state(lap=60), grid=False), 'first_lap must be in [61, total_laps]'),
    (dict(events=([], [(5, 9, SC), (12, 12, RED), (9, 10, NONE)])),
     'scenario 1, event 2: first_lap..last_lap: lap 9 has two overrides in this scenario'),
    (dict(events=([(7, 7, SC), (7, 7, SC)],)), 'event 1: first_lap..last_lap: lap 7 has two overrides'),
    (dict(events=([], [(2 + k % 59, 2 + k % 59, SC) for k in range(65)])), 'scenario 1: event_count must be in [0, 64]'),
    (dict(plans=({1: (-1, 0, [(61, H)])},)), 'scenario 0, plan 0: stop 0: stop_lap must be in [2, total_laps]'),
    (dict(plans=({0: (5, 0, [(20, H)])},)), 'plan 0: start_compound must be -1 or in [MCGP_SOFT, MCGP_WET]'),
    (dict(plans=({0: (1, 0, [(20, H)])},), state=_state(), grid=False), 'a state fixes the tyres'),
    (dict(deviates=53), 'MCGP_DEVIATES_32'),
    (dict(null=('hist',)), 'hist_out is NULL'),
    (dict(null=('plan_count',)), 'plan_count is NULL'),
    (dict(null=('event_count',)), 'event_count is NULL'),
    (dict(plans=({0: (-1, 0, [(20, H)])},), null=('plans',)), 'plans is NULL'),
    (dict(events=([(5, 5, SC)],), null=('events',)), 'events is NULL'),
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
    """MCGP_E_BAD_ARG naming the scenario, the override and the field, on a machine with or without a GPU (device 999 is
    never looked up: the checks come first), and the outputs keep their values."""
    rc, err, untouched = _call(device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert untouched


def test_limits_are_inclusive_and_zero_simulations_need_no_device():
    singles = [(2 + k, 2 + k, k % 4) for k in range(59)]
    ok = [
        dict(events=([],) * 64),
        dict(events=([(2, 60, NONE)],)),
        dict(events=([(2, 2, RED), (60, 60, VSC), (3, 59, SC)],)),
        dict(events=(singles, [], singles)),
        dict(events=([(2, 30, SC)],), plans=({2: (-1, 0, [(30, H)])},)),
        dict(events=([(11, 11, SC), (12, 60, NONE)],), state=_state(lap=10), grid=False),
        dict(events=([(60, 60, RED)],), state=_state(lap=59), grid=False),
        dict(events=([],), state=_state(lap=60), grid=False),               # nothing left to run or to override
        dict(null=('plans', 'events')),                     # every count is 0
    ]
    for kw in ok:
        rc, err, untouched = _call(n_sims=0, device=999, **kw)
        assert rc == 0 and untouched, (kw, err)
    # 64 overrides in each of 64 scenarios, 32 cars, 1000 laps
    rc, err, untouched = _call(events=([(2 + 15 * k, 10 + 15 * k, k % 4) for k in range(64)],) * 64, n=32, laps=1000,
                               n_sims=0, device=999)
    assert rc == 0 and untouched, err
    # with simulations, a valid call gets past the checks to the device lookup
    rc, err, untouched = _call(events=([(5, 5, SC)],), n_sims=10, device=999)
    assert rc == -2 and untouched, err


def test_event_struct_matches_the_header():
    assert C.sizeof(N.McgpLapEvent) == 12
    assert [(f, getattr(N.McgpLapEvent, f).offset) for f, _ in N.McgpLapEvent._fields_] == [
        ('first_lap', 0), ('last_lap', 4), ('kind', 8)]
    with open(O.ROOT + '/include/mcgp.h') as f:
        header = f.read()
    assert 'enum { MCGP_EVT_NONE = 0, MCGP_EVT_RED_FLAG = 1, MCGP_EVT_SAFETY_CAR = 2, MCGP_EVT_VSC = 3 };' in header
    assert '#define MCGP_MAX_SCENARIO_EVENTS 64' in header and '#define MCGP_ABI_VERSION 6' in header
    assert 'int32_t first_lap, last_lap;' in header and 'int32_t kind;' in header
    assert (N.EVT_NONE, N.EVT_RED_FLAG, N.EVT_SAFETY_CAR, N.EVT_VSC, N.MAX_SCENARIO_EVENTS) == (0, 1, 2, 3, 64)
    assert N.EVENT_KIND == {'none': 0, 'red': 1, 'sc': 2, 'vsc': 3} and N.EVENT_ROWS == ('red', 'sc', 'vsc')
    assert 'mcgp_run_events' in N.EXPORTS and hasattr(N.lib(), 'mcgp_run_events')


# ---------------------------------------------------------------- Python layer
def test_race_event_c_struct():
    e = RaceEvent('sc', 31).c_struct()
    assert (e.first_lap, e.last_lap, e.kind) == (31, 31, N.EVT_SAFETY_CAR)
    e = RaceEvent('none', 31, 57).c_struct(31, 57)
    assert (e.first_lap, e.last_lap, e.kind) == (31, 57, N.EVT_NONE)
    assert RaceEvent('red', 2).c_struct(2, 60).kind == N.EVT_RED_FLAG and RaceEvent('vsc', 60).c_struct(2, 60).kind == 3
    with pytest.raises(ValueError, match='kind'):
        RaceEvent('yellow', 5).c_struct()
    with pytest.raises(ValueError, match='above to_lap'):
        RaceEvent('sc', 9, 8).c_struct()
    with pytest.raises(ValueError, match='lap 1 has no event'):
        RaceEvent('sc', 1).c_struct(2, 60)
    with pytest.raises(ValueError, match=r'laps must be in \[2, 60\]'):
        RaceEvent('sc', 50, 61).c_struct(2, 60)
    with pytest.raises(ValueError, match="after the state's lap"):
        RaceEvent('sc', 30).c_struct(31, 60)


def test_run_events_value_errors_and_scenario_names():
    c = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=DEFAULT_SET_POP)
    d = list(c['grid_probs'])
    L = c['config']['total_laps']
    args = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(grid_probs=c['grid_probs'], seed=1)
    with pytest.raises(ValueError, match="'x'.*lap 12 has two overrides"):
        sim.run_events(0, {'x': [RaceEvent('sc', 10, 12), RaceEvent('none', 12, 20)]}, None, *args, **kw)
    with pytest.raises(ValueError, match="'x'.*kind"):
        sim.run_events(0, {'x': [RaceEvent('SC', 10)]}, None, *args, **kw)
    with pytest.raises(ValueError, match='lap 1 has no event'):
        sim.run_events(0, {'x': [RaceEvent('sc', 1)]}, None, *args, **kw)
    with pytest.raises(ValueError, match='laps must be in'):
        sim.run_events(0, {'x': [RaceEvent('sc', 5, L + 1)]}, None, *args, **kw)
    with pytest.raises(ValueError, match='at most 64 overrides'):
        sim.run_events(0, {'x': [RaceEvent('sc', 2)] * 65}, None, *args, **kw)
    with pytest.raises(ValueError, match='not one of the drivers'):
        sim.run_events(0, {'x': []}, {'x': [PitPlan('NOBODY', [(20, 'HARD')])]}, *args, **kw)
    with pytest.raises(ValueError, match='1 to 64 scenarios'):
        sim.run_events(0, {}, None, *args, **kw)
    with pytest.raises(ValueError, match='exactly one of'):
        sim.run_events(0, {'x': []}, None, *args, seed=1)
    # the names are the union of the two dicts, events first; zero simulations need no device
    r = sim.run_events(0, {'as drawn': [], 'sc': [RaceEvent('sc', 31), RaceEvent('none', 32, L)]},
                       {'sc': [PitPlan(d[0], [(31, 'HARD')])], 'plan only': [PitPlan(d[1], [(25, 'HARD')])]}, *args, **kw)
    assert r.names == ['as drawn', 'sc', 'plan only'] and r.n_simulations == 0 and isinstance(r, EventResult)
    assert r.hist.shape == (3, 20, 20) and r.delta.shape == (3, 20, 39) and r.events.shape == (3, 3, L + 1)


def test_event_result_helpers():
    r = _result()
    assert isinstance(r, StrategyResult)
    assert r.win_probability('sc', 'A') == pytest.approx(0.7)
    assert r.compare('sc', 'A')['p_better'] == pytest.approx(0.4)
    dist = r.event_count_distribution('as drawn')
    assert list(dist) == ['red', 'sc', 'vsc']
    assert dist['sc'].tolist() == [0.6, 0.3, 0.1, 0.0, 0.0] and dist['red'].tolist() == [0.9, 0.1, 0.0, 0.0, 0.0]
    assert r.expected_events('as drawn') == pytest.approx({'red': 0.1, 'sc': 0.5, 'vsc': 0.0})
    assert r.expected_events('sc') == pytest.approx({'red': 0.0, 'sc': 1.2, 'vsc': 0.5})
    assert r.probability_of('as drawn', 'sc') == pytest.approx(0.4)
    assert r.probability_of('sc', 'sc') == pytest.approx(1.0) and r.probability_of('sc', 'sc', at_least=2) == pytest.approx(0.2)
    assert r.probability_of('sc', 'red') == 0.0 and r.probability_of('sc', 'vsc', at_least=0) == pytest.approx(1.0)
    with pytest.raises(KeyError):
        r.probability_of('sc', 'none')
    with pytest.raises(KeyError):
        r.expected_events('late')


# ---------------------------------------------------------------- CLI
def test_cli_event_parsing():
    assert cli.parse_event('sc=sc@31') == ('sc', RaceEvent('sc', 31))
    assert cli.parse_event('green=none@31-57') == ('green', RaceEvent('none', 31, 57))
    assert cli.parse_event(' late red = RED @ 48 - 57 ') == ('late red', RaceEvent('red', 48, 57))
    assert cli.parse_event('v=vsc@5-5') == ('v', RaceEvent('vsc', 5, 5))
    for bad in ('sc@31', '=sc@31', 'x=sc', 'x=sc@', 'x=sc@a', 'x=sc@31-', 'x=sc@-31', 'x=sc@31-30', 'x=yellow@31', 'x=@31',
                'x=sc@3.5'):
        with pytest.raises(ValueError):
            cli.parse_event(bad)
    events, plans = cli.event_scenarios(['sc=sc@31', 'green=none@31-57', 'sc=none@32-57'], 'NOR', ['sc=:31/HARD'])
    assert list(events) == ['as drawn', 'sc', 'green'] and events['as drawn'] == []
    assert events['sc'] == [RaceEvent('sc', 31), RaceEvent('none', 32, 57)] and events['green'] == [RaceEvent('none', 31, 57)]
    assert plans == {'sc': [PitPlan('NOR', [(31, 'HARD')])]}
    # a plan of a new name makes a scenario of its own; the user's own 'as drawn' stays first
    events, plans = cli.event_scenarios(['as drawn=none@2-57', 'sc=sc@31'], 'NOR', ['box=:31/HARD'])
    assert list(events) == ['as drawn', 'sc', 'box'] and events['as drawn'] == [RaceEvent('none', 2, 57)]
    assert events['box'] == [] and list(plans) == ['box']
    with pytest.raises(ValueError, match='at least one --event'):
        cli.event_scenarios([])
    with pytest.raises(ValueError, match='--driver'):
        cli.event_scenarios(['sc=sc@31'], None, ['sc=:31/HARD'])
    with pytest.raises(ValueError, match='twice'):
        cli.event_scenarios(['sc=sc@31'], 'NOR', ['sc=:31/HARD', 'sc=:32/HARD'])


def test_events_cli_with_a_stand_in_predictor(tmp_path, capsys, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, device=0):
            pass

        def predict_events(self, season, race, fixture, events, strategies=None, state=None, n_simulations=0, seed=None,
                           allow_single_compound=False):
            seen.update(events=events, strategies=strategies, n=n_simulations, seed=seed, state=state)
            if any(e.lap < 2 for evs in events.values() for e in evs):
                raise ValueError('lap 1 has no event')
            r = _result()
            return EventResult(names=list(events)[:2], drivers=r.drivers, n_simulations=10, hist=r.hist, delta=r.delta,
                               events=r.events)

    monkeypatch.setattr(cli, 'F1Predictor', Fake)
    out = tmp_path / 'e.json'
    rc = cli.main(['events', '--race', 'Bahrain', '--offline', '--event', 'sc=sc@3', '--driver', 'A', '--plan', 'sc=:3/HARD',
                   '--simulations', '10', '--seed', '3', '--json', str(out)])
    assert rc == 0
    assert list(seen['events']) == ['as drawn', 'sc'] and seen['n'] == 10 and seen['seed'] == 3
    assert seen['events']['sc'] == [RaceEvent('sc', 3)] and seen['strategies'] == {'sc': [PitPlan('A', [(3, 'HARD')])]}
    text = capsys.readouterr().out
    assert 'scenario: as drawn' in text and 'scenario: sc' in text and 'safety car 1.20' in text and '+20.0%' in text
    doc = json.load(open(out))
    assert doc['baseline'] == 'as drawn' and [r['scenario'] for r in doc['scenarios']] == ['as drawn', 'sc']
    a = doc['scenarios'][1]['drivers']['A']
    assert a['win'] == pytest.approx(0.7) and a['win_change'] == pytest.approx(0.2) and a['p_better'] == pytest.approx(0.4)
    assert doc['scenarios'][1]['expected_events'] == pytest.approx({'red': 0.0, 'sc': 1.2, 'vsc': 0.5})
    assert doc['scenarios'][0]['drivers']['A']['win_change'] == 0.0
    assert cli.main(['events', '--race', 'Bahrain', '--offline']) == 2                      # nothing given
    assert cli.main(['events', '--race', 'Bahrain', '--offline', '--event', 'sc=sc@x']) == 2
    assert cli.main(['events', '--race', 'Bahrain', '--offline', '--event', 'sc=sc@3', '--plan', 'x=:30/HARD']) == 2
    assert cli.main(['events', '--race', 'Bahrain', '--offline', '--event', 'sc=sc@1']) == 2        # the library's ValueError
