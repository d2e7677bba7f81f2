"""Pace scenarios, host side: the C-ABI argument checks of mcgp_run_paces (no device needed), the mcgp_pace_offset
layout, PaceOffset and run_paces' ValueErrors, PaceResult's helpers on hand-made counts and the `pace` CLI's parsing and
output with a stand-in predictor."""
import ctypes as C
import json

import numpy as np
import pytest

import oracle_py as O
import paces_ref as PR
import resume_ref as RR
import strategy_ref as SR
from cli_cases import pace_result as _result
from monte_carlo_gp_amd import PaceOffset, PaceResult, PitPlan, RaceConfig, StrategyResult, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, RaceSimulator, _Problem

LAPS, UNTIL = PR.LAPS, PR.UNTIL_STOP
H = 2
inf, nan = float('inf'), float('nan')


# ---------------------------------------------------------------- the C ABI without a device
def _prob(n=3, laps=60, deviates=32):
    c = O.load_case('S60')
    cfg = dict(c['config'], total_laps=laps)
    return _Problem(RaceConfig(**cfg), [f'D{i:02d}' for i in range(n)], {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)


def _call(paces=((),), plans=None, n=3, laps=60, state=None, grid=True, n_sims=100, deviates=32, null=(),
          n_scenarios=None, fill=5, device=0):
    prob = _prob(n, laps, deviates)
    paces = list(paces)
    plans = list(plans) if plans is not None else [{}] * len(paces)
    counts, c_plans = SR.c_plans(plans)
    pcounts, c_offs = PR.c_paces(paces)
    S = len(paces) if n_scenarios is None else n_scenarios
    g = np.full((max(n, 1), max(n, 1)), 1.0 / max(n, 1))
    cs = RR.c_state(*state) if state is not None else None
    h = np.full(max(S, 1) * n * n, fill, np.uint64)
    dl = np.full(max(S, 1) * n * (2 * n - 1), fill, np.uint64)
    ca = np.full(max(S, 1) * n * (laps + 1), fill, np.uint64)
    o = np.full(max(S, 1) * max(n_sims, 1) * n, fill, np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_paces(
        None if 'cfg' in null else C.byref(prob.cfg), C.byref(prob.drv),
        g.ctypes.data_as(C.POINTER(C.c_double)) if grid else None, C.byref(cs) if cs is not None else None, n, S,
        None if 'plan_count' in null else counts, None if 'plans' in null else c_plans,
        None if 'pace_count' in null else pcounts, None if 'paces' in null else c_offs, n_sims, 0, 1, device,
        None if 'hist' in null else u64(h), u64(dl), u64(ca), o.ctypes.data_as(C.POINTER(C.c_uint8)))
    untouched = (h == fill).all() and (dl == fill).all() and (ca == fill).all() and (o == fill).all()
    return rc, N.lib().mcgp_last_error().decode(), untouched


def _state(n=3, lap=10):
    a = dict(cumulative_time=np.array([100.0 * lap + d for d in range(n)], np.float64),
             last_lap_time=np.full(n, 91.5, np.float64), grid_slot=np.arange(n, dtype=np.uint8),
             compound=np.full(n, 1, np.uint8), used_compounds=np.full(n, 0b011, np.uint8),
             tire_age=np.full(n, 7, np.int16), retired_lap=np.zeros(n, np.int16))
    return (a, lap, 0)


BAD = [
    (dict(paces=(), n_scenarios=0), 'n_scenarios must be in [1, 64]'),
    (dict(paces=([],) * 65), 'n_scenarios must be in [1, 64]'),
    (dict(paces=([], [(0, 2, 5, 5, 0.5)])), 'scenario 1, offset 0: kind must be MCGP_PACE_LAPS or MCGP_PACE_UNTIL_STOP'),
    (dict(paces=([(0, -1, 5, 5, 0.5)],)), 'scenario 0, offset 0: kind must be'),
    (dict(paces=([(0, LAPS, 5, 6, 0.5), (3, LAPS, 5, 6, 0.5)],)), 'scenario 0, offset 1: driver must be in [0, n)'),
    (dict(paces=([(-1, UNTIL, 5, 0, 0.5)],)), 'offset 0: driver must be in [0, n)'),
    (dict(paces=([(0, LAPS, 0, 5, 0.5)],)), 'offset 0: first_lap must be in [1, total_laps]'),
    (dict(paces=([(0, LAPS, 61, 61, 0.5)],)), 'first_lap must be in [1, total_laps]'),
    (dict(paces=([(0, UNTIL, 0, 0, 0.5)],)), 'first_lap must be in [1, total_laps]'),
    (dict(paces=([(0, UNTIL, 61, 0, 0.5)],)), 'first_lap must be in [1, total_laps]'),
    (dict(paces=([(0, LAPS, 1, 61, 0.5)],)), 'offset 0: last_lap must be in [1, total_laps]'),
    (dict(paces=([(0, LAPS, 5, 0, 0.5)],)), 'last_lap must be in [1, total_laps]'),
    (dict(paces=([(0, LAPS, 9, 8, 0.5)],)), 'scenario 0, offset 0: first_lap must not be above last_lap'),
    (dict(paces=([(0, UNTIL, 5, 5, 0.5)],)), 'offset 0: last_lap must be 0 with MCGP_PACE_UNTIL_STOP'),
    (dict(paces=([(0, LAPS, 20, 25, 0.5)],), state=_state(lap=20), grid=False),
     "offset 0: first_lap must be in [21, total_laps] (after the state's lap)"),
    (dict(paces=([(0, UNTIL, 20, 0, 0.5)],), state=_state(lap=20), grid=False),
     "first_lap must be in [21, total_laps] (after the state's lap)"),
    (dict(paces=([(0, LAPS, 21, 61, 0.5)],), state=_state(lap=20), grid=False),
     "last_lap must be in [21, total_laps] (after the state's lap)"),
    (dict(paces=([(0, LAPS, 60, 60, 0.5)],), state=_state(lap=60), grid=False), 'first_lap must be in [61, total_laps]'),
    (dict(paces=([(0, LAPS, 5, 5, inf)],)), 'offset 0: seconds must be finite and in [-60, 60]'),
    (dict(paces=([(0, LAPS, 5, 5, nan)],)), 'seconds must be finite and in [-60, 60]'),
    (dict(paces=([(0, UNTIL, 5, 0, 60.001)],)), 'seconds must be finite and in [-60, 60]'),
    (dict(paces=([(0, LAPS, 5, 5, -60.001)],)), 'seconds must be finite and in [-60, 60]'),
    (dict(paces=([], [(1, LAPS, 5, 9, 0.5), (0, LAPS, 9, 9, 0.5), (1, LAPS, 9, 10, -0.5)])),
     'scenario 1, offset 2: first_lap..last_lap: driver 1 has two MCGP_PACE_LAPS offsets on lap 9'),
    (dict(paces=([(2, LAPS, 7, 7, 0.1), (2, LAPS, 7, 7, 0.1)],)), 'offset 1: first_lap..last_lap: driver 2 has two'),
    (dict(paces=([(1, UNTIL, 5, 0, 0.5), (0, UNTIL, 5, 0, 0.5), (1, UNTIL, 30, 0, 0.5)],)),
     'scenario 0, offset 2: driver 1 has two MCGP_PACE_UNTIL_STOP offsets in this scenario'),
    (dict(paces=([], [(k % 3, LAPS, 1 + k // 3, 1 + k // 3, 0.1) for k in range(65)])),
     'scenario 1: pace_count must be in [0, 64]'),
    (dict(plans=({1: (-1, 0, [(61, H)])},)), 'scenario 0, plan 0: stop 0: stop_lap must be in [2, total_laps]'),
    (dict(plans=({0: (5, 0, [(20, H)])},)), 'plan 0: start_compound must be -1 or in [MCGP_SOFT, MCGP_WET]'),
    (dict(plans=({0: (1, 0, [(20, H)])},), state=_state(), grid=False), 'a state fixes the tyres'),
    (dict(deviates=53), 'MCGP_DEVIATES_32'),
    (dict(null=('hist',)), 'hist_out is NULL'),
    (dict(null=('plan_count',)), 'plan_count is NULL'),
    (dict(null=('pace_count',)), 'pace_count is NULL'),
    (dict(plans=({0: (-1, 0, [(20, H)])},), null=('plans',)), 'plans is NULL'),
    (dict(paces=([(0, LAPS, 5, 5, 0.5)],), null=('paces',)), 'paces is NULL'),
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
    """MCGP_E_BAD_ARG naming the scenario, the offset and the field, on a machine with or without a GPU (device 999 is
    never looked up: the checks come first), and the outputs keep their values."""
    rc, err, untouched = _call(device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert untouched


def test_limits_are_inclusive_and_zero_simulations_need_no_device():
    singles = [(k % 3, LAPS, 1 + k // 3, 1 + k // 3, 0.1 * (k % 5 - 2)) for k in range(64)]
    ok = [
        dict(paces=([],) * 64),
        dict(paces=([(0, LAPS, 1, 60, 60.0), (1, LAPS, 1, 60, -60.0), (2, LAPS, 1, 1, 0.0)],)),
        dict(paces=([(0, LAPS, 1, 30, 0.5), (0, LAPS, 31, 60, 0.5), (0, UNTIL, 1, 0, 0.5), (1, UNTIL, 60, 0, -0.5)],)),
        dict(paces=(singles, [], singles)),
        dict(paces=([(2, UNTIL, 30, 0, 0.6)],), plans=({2: (-1, 0, [(30, H)])},)),
        dict(paces=([(0, LAPS, 11, 11, 0.3), (0, UNTIL, 11, 0, 0.3)],), state=_state(lap=10), grid=False),
        dict(paces=([(0, LAPS, 60, 60, 0.3)],), state=_state(lap=59), grid=False),
        dict(paces=([],), state=_state(lap=60), grid=False),                # nothing left to run or to offset
        dict(null=('plans', 'paces')),                      # every count is 0
    ]
    for kw in ok:
        rc, err, untouched = _call(n_sims=0, device=999, **kw)
        assert rc == 0 and untouched, (kw, err)
    # 64 offsets in each of 64 scenarios, 32 cars, 1000 laps
    rc, err, untouched = _call(paces=([(k // 2, k % 2, 1 + 15 * k, (10 + 15 * k) * (1 - k % 2), 0.01 * k)
                                       for k in range(64)],) * 64, n=32, laps=1000, n_sims=0, device=999)
    assert rc == 0 and untouched, err
    # with simulations, a valid call gets past the checks to the device lookup
    rc, err, untouched = _call(paces=([(0, UNTIL, 5, 0, 0.6)],), n_sims=10, device=999)
    assert rc == -2 and untouched, err


def test_pace_struct_matches_the_header():
    assert C.sizeof(N.McgpPaceOffset) == 24
    assert [(f, getattr(N.McgpPaceOffset, f).offset) for f, _ in N.McgpPaceOffset._fields_] == [
        ('driver', 0), ('kind', 4), ('first_lap', 8), ('last_lap', 12), ('seconds', 16)]
    with open(O.ROOT + '/include/mcgp.h') as f:
        header = f.read()
    assert 'enum { MCGP_PACE_LAPS = 0, MCGP_PACE_UNTIL_STOP = 1 };' in header
    assert '#define MCGP_MAX_SCENARIO_PACES 64' in header and '#define MCGP_ABI_VERSION 6' in header
    assert 'typedef struct mcgp_pace_offset {' in header and 'double seconds;' in header
    assert (N.PACE_LAPS, N.PACE_UNTIL_STOP, N.MAX_SCENARIO_PACES, N.MAX_PACE_SECONDS) == (0, 1, 64, 60.0)
    assert 'mcgp_run_paces' in N.EXPORTS and hasattr(N.lib(), 'mcgp_run_paces')


# ---------------------------------------------------------------- Python layer
def test_pace_offset_c_struct():
    index = {'A': 0, 'B': 1}
    p = PaceOffset('B', 0.6, until_stop_from=12).c_struct(index, 1, 57)
    assert (p.driver, p.kind, p.first_lap, p.last_lap, p.seconds) == (1, N.PACE_UNTIL_STOP, 12, 0, 0.6)
    p = PaceOffset('A', -0.15, laps=(40, 49)).c_struct(index, 31, 57)
    assert (p.driver, p.kind, p.first_lap, p.last_lap, p.seconds) == (0, N.PACE_LAPS, 40, 49, -0.15)
    assert PaceOffset('A', 0.0, laps=(1, 1)).c_struct(index).seconds == 0.0
    with pytest.raises(ValueError, match='either laps'):
        PaceOffset('A', 0.5).c_struct(index)
    with pytest.raises(ValueError, match='either laps'):
        PaceOffset('A', 0.5, laps=(1, 2), until_stop_from=1).c_struct(index)
    with pytest.raises(ValueError, match='must not be above'):
        PaceOffset('A', 0.5, laps=(9, 8)).c_struct(index)
    with pytest.raises(ValueError, match=r'laps must be in \[1, 57\]'):
        PaceOffset('A', 0.5, laps=(0, 8)).c_struct(index, 1, 57)
    with pytest.raises(ValueError, match=r'laps must be in \[1, 57\]'):
        PaceOffset('A', 0.5, until_stop_from=58).c_struct(index, 1, 57)
    with pytest.raises(ValueError, match="after the state's lap"):
        PaceOffset('A', 0.5, until_stop_from=30).c_struct(index, 31, 57)
    for sec in (61.0, -60.5, inf, nan):
        with pytest.raises(ValueError, match='seconds must be finite'):
            PaceOffset('A', sec, laps=(1, 2)).c_struct(index)


def test_run_paces_value_errors_and_scenario_names():
    c = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=DEFAULT_SET_POP)
    d = list(c['grid_probs'])
    L = c['config']['total_laps']
    args = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(grid_probs=c['grid_probs'], seed=1)
    with pytest.raises(ValueError, match="'x'.*two offsets on lap 12"):
        sim.run_paces(0, {'x': [PaceOffset(d[0], 0.5, laps=(10, 12)), PaceOffset(d[0], 0.2, laps=(12, 20))]}, None, *args, **kw)
    with pytest.raises(ValueError, match="'x'.*two until-stop offsets"):
        sim.run_paces(0, {'x': [PaceOffset(d[0], 0.5, until_stop_from=3), PaceOffset(d[0], 0.2, until_stop_from=9)]}, None,
                      *args, **kw)
    with pytest.raises(ValueError, match="'x'.*laps must be in"):
        sim.run_paces(0, {'x': [PaceOffset(d[0], 0.5, laps=(0, 3))]}, None, *args, **kw)
    with pytest.raises(ValueError, match='laps must be in'):
        sim.run_paces(0, {'x': [PaceOffset(d[0], 0.5, laps=(5, L + 1))]}, None, *args, **kw)
    with pytest.raises(ValueError, match="'x'.*seconds"):
        sim.run_paces(0, {'x': [PaceOffset(d[0], 99.0, laps=(5, 6))]}, None, *args, **kw)
    with pytest.raises(ValueError, match='at most 64 offsets'):
        sim.run_paces(0, {'x': [PaceOffset(d[0], 0.1, laps=(2, 2))] * 65}, None, *args, **kw)
    with pytest.raises(ValueError, match='not one of the drivers'):
        sim.run_paces(0, {'x': [PaceOffset('NOBODY', 0.1, laps=(2, 2))]}, None, *args, **kw)
    with pytest.raises(ValueError, match='not one of the drivers'):
        sim.run_paces(0, {'x': []}, {'x': [PitPlan('NOBODY', [(20, 'HARD')])]}, *args, **kw)
    with pytest.raises(ValueError, match='1 to 64 scenarios'):
        sim.run_paces(0, {}, None, *args, **kw)
    with pytest.raises(ValueError, match='exactly one of'):
        sim.run_paces(0, {'x': []}, None, *args, seed=1)
    # a LAPS and an until-stop offset of one driver may share laps; two drivers may share a lap; lap 1 is legal
    # the names are the union of the two dicts, paces first; zero simulations need no device
    r = sim.run_paces(0, {'as is': [], 'damage': [PaceOffset(d[0], 0.6, until_stop_from=1), PaceOffset(d[0], 0.1, laps=(1, L)),
                                                   PaceOffset(d[1], 0.1, laps=(1, L))]},
                      {'damage': [PitPlan(d[0], [(13, 'HARD')])], 'plan only': [PitPlan(d[1], [(25, 'HARD')])]}, *args, **kw)
    assert r.names == ['as is', 'damage', 'plan only'] and r.n_simulations == 0 and isinstance(r, PaceResult)
    assert r.hist.shape == (3, 20, 20) and r.delta.shape == (3, 20, 39) and r.carried.shape == (3, 20, L + 1)
    assert r.until_from == {('damage', d[0]): 1}


def test_pace_result_helpers():
    r = _result()
    assert isinstance(r, StrategyResult)
    assert r.win_probability('damage', 'A') == pytest.approx(0.7)
    assert r.compare('damage', 'A')['p_better'] == pytest.approx(0.4)
    assert r.carried_distribution('damage', 'A').tolist() == [0.1, 0.4, 0.3, 0.2, 0.0]
    assert r.carried_distribution('damage', 'B').tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert r.expected_laps_carried('damage', 'A') == pytest.approx(0.4 + 0.6 + 0.6)
    assert r.expected_laps_carried('as is', 'A') == 0.0
    assert r.probability_cleared_by('damage', 'A', 1) == 0.0                   # before the offset begins
    assert r.probability_cleared_by('damage', 'A', 2) == pytest.approx(0.5)    # carried on at most one lap
    assert r.probability_cleared_by('damage', 'A', 3) == pytest.approx(0.8)
    assert r.probability_cleared_by('damage', 'A', 4) == pytest.approx(1.0)
    with pytest.raises(KeyError):
        r.probability_cleared_by('damage', 'B', 3)
    with pytest.raises(KeyError):
        r.carried_distribution('late', 'A')
    with pytest.raises(KeyError):
        r.expected_laps_carried('damage', 'Z')


# ---------------------------------------------------------------- CLI
def test_cli_offset_parsing():
    assert cli.parse_offset('damage=NOR:0.6@12+') == ('damage', PaceOffset('NOR', 0.6, until_stop_from=12))
    assert cli.parse_offset('push=NOR:-0.15@40-49') == ('push', PaceOffset('NOR', -0.15, laps=(40, 49)))
    assert cli.parse_offset(' lift and coast = VER : 0.3 @ 43 - 57 ') == ('lift and coast', PaceOffset('VER', 0.3, laps=(43, 57)))
    assert cli.parse_offset('u=LEC:-.2@1-1') == ('u', PaceOffset('LEC', -0.2, laps=(1, 1)))
    for bad in ('NOR:0.6@12+', '=NOR:0.6@12+', 'x=NOR:0.6', 'x=NOR:0.6@', 'x=NOR:0.6@a', 'x=NOR:0.6@12', 'x=NOR:0.6@12-',
                'x=NOR:0.6@-12', 'x=NOR:0.6@12-11', 'x=NOR@12+', 'x=:0.6@12+', 'x=NOR:fast@12+', 'x=NOR:0.6@+', 'x=NOR:0.6@3.5+'):
        with pytest.raises(ValueError):
            cli.parse_offset(bad)
    paces, plans = cli.pace_scenarios(['damage=NOR:0.6@12+', 'push=NOR:-0.15@40-49', 'damage=NOR:0.1@12-20'], 'NOR',
                                      ['damage=:13/HARD'])
    assert list(paces) == ['as is', 'damage', 'push'] and paces['as is'] == []
    assert paces['damage'] == [PaceOffset('NOR', 0.6, until_stop_from=12), PaceOffset('NOR', 0.1, laps=(12, 20))]
    assert plans == {'damage': [PitPlan('NOR', [(13, 'HARD')])]}
    # a plan of a new name makes a scenario of its own; the user's own 'as is' stays first
    paces, plans = cli.pace_scenarios(['as is=NOR:0.6@12+', 'x=NOR:0.1@2-3'], 'NOR', ['box=:31/HARD'])
    assert list(paces) == ['as is', 'x', 'box'] and paces['as is'] == [PaceOffset('NOR', 0.6, until_stop_from=12)]
    assert paces['box'] == [] and list(plans) == ['box']
    with pytest.raises(ValueError, match='at least one --offset'):
        cli.pace_scenarios([])
    with pytest.raises(ValueError, match='--driver'):
        cli.pace_scenarios(['x=NOR:0.1@2-3'], None, ['x=:31/HARD'])
    with pytest.raises(ValueError, match='twice'):
        cli.pace_scenarios(['x=NOR:0.1@2-3'], 'NOR', ['x=:31/HARD', 'x=:32/HARD'])


def test_pace_cli_with_a_stand_in_predictor(tmp_path, capsys, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, device=0):
            pass

        def predict_paces(self, season, race, fixture, paces, strategies=None, state=None, n_simulations=0, seed=None,
                          allow_single_compound=False):
            seen.update(paces=paces, strategies=strategies, n=n_simulations, seed=seed, state=state)
            if any(p.seconds > 60 for ps in paces.values() for p in ps):
                raise ValueError('seconds must be finite and in [-60, 60]')
            r = _result()
            return PaceResult(names=list(paces)[:2], drivers=r.drivers, n_simulations=10, hist=r.hist, delta=r.delta,
                              carried=r.carried, until_from={(list(paces)[1], 'A'): 2})

    monkeypatch.setattr(cli, 'F1Predictor', Fake)
    out = tmp_path / 'p.json'
    rc = cli.main(['pace', '--race', 'Bahrain', '--offline', '--offset', 'damage=A:0.6@2+', '--driver', 'A', '--plan',
                   'damage=:3/HARD', '--simulations', '10', '--seed', '3', '--json', str(out)])
    assert rc == 0
    assert list(seen['paces']) == ['as is', 'damage'] and seen['n'] == 10 and seen['seed'] == 3
    assert seen['paces']['damage'] == [PaceOffset('A', 0.6, until_stop_from=2)]
    assert seen['strategies'] == {'damage': [PitPlan('A', [(3, 'HARD')])]}
    text = capsys.readouterr().out
    assert 'scenario: as is' in text and 'scenario: damage' in text and '+20.0%' in text
    assert 'offset carried 1.60 laps on average' in text and '1 laps 40.0%' in text
    doc = json.load(open(out))
    assert doc['baseline'] == 'as is' and [r['scenario'] for r in doc['scenarios']] == ['as is', 'damage']
    a = doc['scenarios'][1]['drivers']['A']
    assert a['win'] == pytest.approx(0.7) and a['win_change'] == pytest.approx(0.2) and a['p_better'] == pytest.approx(0.4)
    assert a['expected_position_change'] == pytest.approx((0.7 + 0.4 + 0.3) - (0.5 + 0.6 + 0.6))
    assert a['laps_carried'] == [0.1, 0.4, 0.3, 0.2, 0.0] and a['expected_laps_carried'] == pytest.approx(1.6)
    assert doc['scenarios'][0]['drivers']['A']['win_change'] == 0.0 and 'laps_carried' not in doc['scenarios'][0]['drivers']['A']
    assert cli.main(['pace', '--race', 'Bahrain', '--offline']) == 2                        # nothing given
    assert cli.main(['pace', '--race', 'Bahrain', '--offline', '--offset', 'x=A:0.6@x']) == 2
    assert cli.main(['pace', '--race', 'Bahrain', '--offline', '--offset', 'x=A:0.6@2+', '--plan', 'x=:30/HARD']) == 2
    assert cli.main(['pace', '--race', 'Bahrain', '--offline', '--offset', 'x=A:99@2+']) == 2       # the library's ValueError
