"""Pit-strategy comparison, host side: the Python restatement of a race with plans (strategy_ref) against the CPU
oracle's own finishing orders, the C-ABI argument checks of mcgp_run_strategies (no device needed), the mcgp_pit_plan
layout, the two-compound check, pit_window, StrategyResult's helpers on hand-made counts and the `strategy` CLI's
parsing and output with a stand-in predictor."""
import ctypes as C
import json

import numpy as np
import pytest

import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
from cli_cases import strategy_result as _result
from monte_carlo_gp_amd import PitPlan, RaceConfig, StrategyResult, cli, pit_window
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, _Problem, check_two_compounds


# ---------------------------------------------------------------- the restatement checks itself against the oracle
@pytest.mark.parametrize('name', ['S60', 'EVT', 'DMP', 'WET', 'HET'])
def test_restatement_without_plans_equals_the_oracle(name):
    case = O.load_case(name)
    seed, m = 17, 48
    ref = RR.traced_run(case, m, seed, 1000)
    orders = SR.orders(case, m, seed, 1000, grids=ref['grids'])
    assert np.array_equal(orders, ref['orders'])
    L = case['config']['total_laps']
    for k in (1, 2, L // 3, L - 1, L):
        for i in range(0, m, 3):
            st = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, 1000 + i, k))
            o = SR.orders(case, 1, seed, 1000 + i, state=st)
            assert np.array_equal(o[0], ref['orders'][i]), (name, k, i)


def test_restatement_without_plans_equals_the_oracle_on_every_fuzz_configuration():
    """The 84 configurations of tests/golden/fuzz_cases.json (the 12 corner cases among them), each with its own seed:
    the restatement's orders are the oracle's, and from the oracle's traced state of simulation i after laps 1, L // 2
    and L it ends in the oracle's order of i.  This licenses the restatement as the reference for plans there."""
    with open(O.GOLDEN_DIR + '/fuzz_cases.json') as f:
        cases = json.load(f)
    m, done, resumed = 32, 0, 0
    for name, case in cases.items():
        seed, L = case['seed'], case['config']['total_laps']
        ref = RR.traced_run(case, m, seed)
        assert np.array_equal(SR.orders(case, m, seed, grids=ref['grids']), ref['orders']), name
        done += 1
        if L < 2:
            continue
        for k in sorted({1, L // 2, L}):
            for i in range(0, m, 8):
                st = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, i, k))
                assert np.array_equal(SR.orders(case, 1, seed, i, state=st)[0], ref['orders'][i]), (name, k, i)
                resumed += 1
    assert done == 84 and resumed >= 83 * 2 * 4


def test_restatement_plans_change_the_race():
    """A plan is not a no-op in the restatement: a driver who never stops in a dry race finishes differently."""
    case = O.load_case('S60')
    ref = RR.traced_run(case, 24, 3)
    a = SR.orders(case, 24, 3, grids=ref['grids'])
    b = SR.orders(case, 24, 3, grids=ref['grids'], plans={0: (-1, 0, [])})
    assert np.array_equal(a, ref['orders']) and not np.array_equal(a, b)


# ---------------------------------------------------------------- the C ABI without a device
def _prob(n=3, laps=60, deviates=32):
    c = O.load_case('S60')
    cfg = dict(c['config'], total_laps=laps)
    return _Problem(RaceConfig(**cfg), [f'D{i:02d}' for i in range(n)], {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)


def _call(scenarios=({},), n=3, laps=60, state=None, grid=True, n_sims=100, deviates=32, null=(), n_scenarios=None,
          fill=5, device=0):
    prob = _prob(n, laps, deviates)
    counts, plans = SR.c_plans(list(scenarios))
    S = len(scenarios) if n_scenarios is None else n_scenarios
    g = np.full((max(n, 1), max(n, 1)), 1.0 / max(n, 1))
    cs = RR.c_state(*state) if state is not None else None
    h = np.full(max(S, 1) * n * n, fill, np.uint64)
    dl = np.full(max(S, 1) * n * (2 * n - 1), fill, np.uint64)
    o = np.full(max(S, 1) * max(n_sims, 1) * n, fill, np.uint8)
    rc = N.lib().mcgp_run_strategies(
        None if 'cfg' in null else C.byref(prob.cfg), C.byref(prob.drv),
        g.ctypes.data_as(C.POINTER(C.c_double)) if grid else None, C.byref(cs) if cs is not None else None, n, S,
        None if 'plan_count' in null else counts, None if 'plans' in null else plans, n_sims, 0, 1, device,
        None if 'hist' in null else h.ctypes.data_as(C.POINTER(C.c_uint64)), dl.ctypes.data_as(C.POINTER(C.c_uint64)),
        o.ctypes.data_as(C.POINTER(C.c_uint8)))
    untouched = (h == fill).all() and (dl == fill).all() and (o == fill).all()
    return rc, N.lib().mcgp_last_error().decode(), untouched


def _state(n=3, lap=10):
    a = dict(cumulative_time=np.array([100.0 * lap + d for d in range(n)], np.float64),
             last_lap_time=np.full(n, 91.5, np.float64), grid_slot=np.arange(n, dtype=np.uint8),
             compound=np.full(n, 1, np.uint8), used_compounds=np.full(n, 0b011, np.uint8),
             tire_age=np.full(n, 7, np.int16), retired_lap=np.zeros(n, np.int16))
    return (a, lap, 0)


H = 2
BAD = [
    (dict(scenarios=(), n_scenarios=0), 'n_scenarios must be in [1, 64]'),
    (dict(scenarios=({},) * 65), 'n_scenarios must be in [1, 64]'),
    (dict(scenarios=({}, {1: (-1, 0, [(10 + k, H) for k in range(9)])})), 'scenario 1, plan 0: n_stops'),
    (dict(scenarios=({1: (-1, 0, [(61, H)])},)), 'scenario 0, plan 0: stop 0: stop_lap must be in [2, total_laps]'),
    (dict(scenarios=({1: (-1, 0, [(0, H)])},)), 'stop_lap must be in [2, total_laps]'),
    (dict(scenarios=({1: (-1, 0, [(1, H)])},)), 'lap 1 has no pit step'),
    (dict(scenarios=({1: (-1, 0, [(20, H), (20, 1)])},)), 'stop 1: stop_lap must be strictly increasing'),
    (dict(scenarios=({1: (-1, 0, [(30, H), (20, 1)])},)), 'stop 1: stop_lap must be strictly increasing'),
    (dict(scenarios=({0: (-1, 0, [(20, H)])},), state=_state(lap=20), grid=False),
     'stop 0: stop_lap must be in [21, total_laps] (after the state\'s lap)'),
    (dict(scenarios=({0: (-1, 0, [(10, H)])},), state=_state(lap=20), grid=False), 'stop_lap must be in [21'),
    (dict(scenarios=({0: (-1, 0, [(20, 5)])},)), 'stop 0: stop_compound must be in [MCGP_SOFT, MCGP_WET]'),
    (dict(scenarios=({0: (5, 0, [(20, H)])},)), 'plan 0: start_compound must be -1 or in [MCGP_SOFT, MCGP_WET]'),
    (dict(scenarios=({0: (-2, 0, [(20, H)])},)), 'start_compound must be -1 or in'),
    (dict(scenarios=({0: (0, 1023 - 60 + 1, [(20, H)])},)), 'start_age must be in [0, 1023 - total_laps]'),
    (dict(scenarios=({0: (0, -1, [(20, H)])},)), 'start_age must be in [0, 1023 - total_laps]'),
    (dict(scenarios=({0: (-1, 3, [(20, H)])},)), 'start_age must be 0 with start_compound -1'),
    (dict(scenarios=({0: (1, 0, [(20, H)])},), state=_state(), grid=False), 'a state fixes the tyres'),
    (dict(scenarios=({0: (-1, 2, [(20, H)])},), state=_state(), grid=False), 'a state fixes the tyres'),
    (dict(scenarios=({3: (-1, 0, [(20, H)])},)), 'scenario 0, plan 0: driver must be in [0, n)'),
    (dict(scenarios=({-1: (-1, 0, [(20, H)])},)), 'driver must be in [0, n)'),
    (dict(deviates=53), 'MCGP_DEVIATES_32'),
    (dict(null=('hist',)), 'hist_out is NULL'),
    (dict(null=('plan_count',)), 'plan_count is NULL'),
    (dict(scenarios=({0: (-1, 0, [(20, H)])},), null=('plans',)), 'plans is NULL'),
    (dict(null=('cfg',)), 'cfg / drv is NULL'),
    (dict(grid=False), 'grid_probs is NULL'),
    (dict(state=_state()), 'grid_probs must be NULL when a state is given'),
    (dict(state=(dict(_state()[0], compound=np.array([7, 1, 1], np.uint8)), 10, 0), grid=False),
     'state 0: car 0: compound'),
    (dict(n=0), 'n must be in [1, 32]'),
    (dict(n=33), 'n must be in [1, 32]'),
]


@pytest.mark.parametrize('kw,msg', BAD, ids=[m for _, m in BAD])
def test_library_rejects_bad_arguments_before_any_device_lookup(kw, msg):
    """MCGP_E_BAD_ARG naming the scenario, plan and field, on a machine with or without a GPU (device 999 is never
    looked up: the checks come first), and the outputs keep their values."""
    rc, err, untouched = _call(device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert untouched


def test_library_rejects_a_driver_planned_twice():
    counts, _ = SR.c_plans([{}])
    p = (N.McgpPitPlan * 2)(N.McgpPitPlan(driver=1, start_compound=-1), N.McgpPitPlan(driver=1, start_compound=-1))
    prob = _prob()
    g = np.full((3, 3), 1.0 / 3)
    h = np.zeros(9 * 2, np.uint64)
    rc = N.lib().mcgp_run_strategies(C.byref(prob.cfg), C.byref(prob.drv), g.ctypes.data_as(C.POINTER(C.c_double)),
                                     None, 3, 2, (C.c_uint32 * 2)(0, 2), p, 10, 0, 1, 999,
                                     h.ctypes.data_as(C.POINTER(C.c_uint64)), None, None)
    assert rc == -1 and 'scenario 1, plan 1: driver 1 has two plans in this scenario' in N.lib().mcgp_last_error().decode()


def test_limits_are_inclusive_and_zero_simulations_need_no_device():
    ok = [
        dict(scenarios=({},) * 64),
        dict(scenarios=({1: (-1, 0, [(2 + k, H) for k in range(8)])},)),
        dict(scenarios=({1: (-1, 0, [(60, H)]), 0: (0, 1023 - 60, [(2, 1)]), 2: (4, 0, [])},)),
        dict(scenarios=({0: (-1, 0, [(11, H), (60, 0)])},), state=_state(lap=10), grid=False),
        dict(scenarios=({0: (-1, 0, [])},), state=_state(lap=60), grid=False),
    ]
    for kw in ok:
        rc, err, untouched = _call(n_sims=0, device=999, **kw)
        assert rc == 0 and untouched, (kw, err)
    # with simulations, a valid call gets past the checks to the device lookup
    rc, err, untouched = _call(n_sims=10, device=999)
    assert rc == -2 and untouched, err


def test_plan_struct_matches_the_header():
    assert C.sizeof(N.McgpPitPlan) == 40
    assert [(f, getattr(N.McgpPitPlan, f).offset) for f, _ in N.McgpPitPlan._fields_] == [
        ('driver', 0), ('start_compound', 4), ('start_age', 8), ('n_stops', 12), ('stop_lap', 16), ('stop_compound', 32)]
    with open(O.ROOT + '/include/mcgp.h') as f:
        header = f.read()
    assert '#define MCGP_MAX_PLAN_STOPS 8' in header and '#define MCGP_MAX_SCENARIOS 64' in header
    assert 'mcgp_run_strategies' in N.EXPORTS and hasattr(N.lib(), 'mcgp_run_strategies')


# ---------------------------------------------------------------- Python layer
def test_two_compound_rule():
    check_two_compounds(PitPlan('A', [(20, 'HARD')]))                     # SOFT or MEDIUM start, then HARD
    with pytest.raises(ValueError, match='one dry compound'):
        check_two_compounds(PitPlan('A', [(20, 'MEDIUM')]))               # a MEDIUM starter would run MEDIUM only
    with pytest.raises(ValueError, match='one dry compound'):
        check_two_compounds(PitPlan('A', [(20, 'SOFT')]))
    check_two_compounds(PitPlan('A', [(20, 'SOFT')], start='HARD'))
    with pytest.raises(ValueError, match="scenario 'x'"):
        check_two_compounds(PitPlan('A', [], start='HARD'), scenario='x')
    check_two_compounds(PitPlan('A', [(20, 'SOFT'), (40, 'MEDIUM')]))
    check_two_compounds(PitPlan('A', [(20, 'INTERMEDIATE'), (30, 'SOFT'), (40, 'MEDIUM')]))
    with pytest.raises(ValueError):
        check_two_compounds(PitPlan('A', [(20, 'INTERMEDIATE')], start='SOFT'))
    # from a state: its used set counts
    check_two_compounds(PitPlan('A', []), used={'SOFT', 'MEDIUM'})
    check_two_compounds(PitPlan('A', [(40, 'HARD')]), used={'SOFT'})
    with pytest.raises(ValueError):
        check_two_compounds(PitPlan('A', [(40, 'SOFT')]), used={'SOFT'})


def test_plan_c_struct():
    p = PitPlan('B', [(18, 'HARD'), (40, 'SOFT')], start='MEDIUM', start_age=3).c_struct({'A': 0, 'B': 1})
    assert (p.driver, p.start_compound, p.start_age, p.n_stops) == (1, 1, 3, 2)
    assert list(p.stop_lap[:2]) == [18, 40] and list(p.stop_compound[:2]) == [2, 0]
    assert PitPlan('A').c_struct({'A': 0}).start_compound == -1
    with pytest.raises(ValueError, match='compound'):
        PitPlan('A', [(18, 'ULTRA')]).c_struct({'A': 0})
    with pytest.raises(ValueError, match='at most 8'):
        PitPlan('A', [(k, 'SOFT') for k in range(2, 11)]).c_struct({'A': 0})
    with pytest.raises(ValueError, match='race state'):
        PitPlan('A', [(40, 'SOFT')], start='SOFT').c_struct({'A': 0}, from_state=True)


def test_pit_window():
    w = pit_window('VER', range(18, 21), 'HARD', then=[(45, 'SOFT')], start='MEDIUM')
    assert list(w) == ['VER L18', 'VER L19', 'VER L20']
    assert w['VER L19'] == [PitPlan('VER', [(19, 'HARD'), (45, 'SOFT')], start='MEDIUM')]


def test_strategy_result_helpers():
    r = _result()
    assert r.position_probabilities('early')['A'] == {1: 0.7, 2: 0.2, 3: 0.1}
    assert set(r.position_probabilities()) == {'model', 'early'}
    assert r.expected_position('model')['A'] == pytest.approx(1.7)
    assert r.expected_points('early', points=(10, 5, 1))['A'] == pytest.approx(0.7 * 10 + 0.2 * 5 + 0.1 * 1)
    assert r.expected_points('early')['A'] == pytest.approx(0.7 * 25 + 0.2 * 18 + 0.1 * 15)
    c = r.compare('early', 'A')
    gains = np.array([2] * 1 + [1] * 3 + [0] * 5 + [-1] * 1, np.float64)
    assert c['p_better'] == pytest.approx(0.4) and c['p_same'] == pytest.approx(0.5) and c['p_worse'] == pytest.approx(0.1)
    assert c['mean_gain'] == pytest.approx(gains.mean())
    assert c['se'] == pytest.approx(gains.std(ddof=1) / np.sqrt(10))
    assert c['se_unpaired'] > 0
    base = r.compare('model', 'B')
    assert (base['p_same'], base['mean_gain'], base['se']) == (1.0, 0.0, 0.0)
    assert r.best('A') == 'early' and r.best('A', by='win') == 'early' and r.best('A', by='expected_position') == 'early'
    with pytest.raises(ValueError, match='return_orders'):
        r.compare('model', 'A', against='early')
    with pytest.raises(KeyError):
        r.compare('late', 'A')
    with pytest.raises(ValueError):
        r.best('A', by='speed')


def test_compare_against_another_scenario_uses_the_orders():
    orders = np.array([[[0, 1, 2], [1, 0, 2]], [[1, 0, 2], [1, 0, 2]], [[2, 1, 0], [0, 1, 2]]], np.uint8)
    hist = np.stack([RR.counts(orders[s], 3) for s in range(3)])
    r = StrategyResult(names=['a', 'b', 'c'], drivers=['A', 'B', 'C'], n_simulations=2, hist=hist,
                       delta=SR.delta_counts(orders, 3), orders=orders)
    c = r.compare('c', 'A', against='b')          # A: position 2 vs 1 in sim 0, 0 vs 1 in sim 1
    assert (c['p_better'], c['p_worse'], c['mean_gain']) == (0.5, 0.5, 0.0)
    assert r.compare('b', 'A') == r.compare('b', 'A', against='a')


# ---------------------------------------------------------------- CLI
def test_cli_plan_parsing():
    assert cli.parse_plan('one=:25/HARD', 'VER') == ('one', PitPlan('VER', [(25, 'HARD')]))
    assert cli.parse_plan('two=s:15/m, 38/Soft', 'VER') == ('two', PitPlan('VER', [(15, 'MEDIUM'), (38, 'SOFT')],
                                                                           start='SOFT'))
    assert cli.parse_plan('none=:', 'VER') == ('none', PitPlan('VER', []))
    for bad in ('one', '=:25/HARD', 'one=25/HARD', 'one=:25', 'one=:x/HARD', 'one=:25/ULTRA', 'one=Q:25/HARD'):
        with pytest.raises(ValueError):
            cli.parse_plan(bad, 'VER')
    assert cli.parse_window('18-20/h') == (range(18, 21), 'HARD')
    for bad in ('18/HARD', '20-18/HARD', '18-20', 'a-b/HARD'):
        with pytest.raises(ValueError):
            cli.parse_window(bad)
    sc = cli.strategy_scenarios('VER', ['one=:25/HARD'], '18-19/HARD')
    assert list(sc) == ['model', 'one', 'VER L18', 'VER L19'] and sc['model'] == []
    with pytest.raises(ValueError, match='twice'):
        cli.strategy_scenarios('VER', ['one=:25/HARD', 'one=:26/HARD'])


def test_strategy_cli_with_a_stand_in_predictor(tmp_path, capsys, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, device=0):
            pass

        def predict_strategies(self, season, race, fixture, strategies, state=None, n_simulations=0, seed=None,
                               allow_single_compound=False):
            seen.update(strategies=strategies, n=n_simulations, seed=seed, state=state)
            r = _result()
            return StrategyResult(names=list(strategies)[:2], drivers=r.drivers, n_simulations=10, hist=r.hist,
                                  delta=r.delta)

    monkeypatch.setattr(cli, 'F1Predictor', Fake)
    out = tmp_path / 's.json'
    rc = cli.main(['strategy', '--race', 'Bahrain', '--offline', '--driver', 'A', '--plan', 'early=:15/HARD',
                   '--simulations', '10', '--seed', '3', '--json', str(out)])
    assert rc == 0
    assert list(seen['strategies']) == ['model', 'early'] and seen['n'] == 10 and seen['seed'] == 3
    text = capsys.readouterr().out
    assert 'early' in text and 'model' in text and 'best by expected points: early' in text
    rows = json.load(open(out))['scenarios']
    assert [r['scenario'] for r in rows] == ['model', 'early']
    assert rows[1]['win'] == pytest.approx(0.7) and rows[1]['p_better'] == pytest.approx(0.4)
    assert cli.main(['strategy', '--race', 'Bahrain', '--offline', '--driver', 'A']) == 2       # nothing to compare
    assert cli.main(['strategy', '--race', 'Bahrain', '--offline', '--driver', 'A', '--plan', 'bad']) == 2


def test_strategy_cli_reports_the_librarys_value_error(capsys, monkeypatch):
    class Fake:
        def __init__(self, device=0):
            pass

        def predict_strategies(self, season, race, fixture, strategies, state=None, n_simulations=0, seed=None,
                               allow_single_compound=False):
            raise ValueError("scenario 'early': A uses one dry compound")

    monkeypatch.setattr(cli, 'F1Predictor', Fake)
    rc = cli.main(['strategy', '--race', 'Bahrain', '--offline', '--driver', 'A', '--plan', 'early=:15/HARD'])
    assert rc == 2                                          # as the other six what-if commands: no traceback
    captured = capsys.readouterr()
    assert captured.err == "error: scenario 'early': A uses one dry compound\n"
    assert 'F1 Pit Strategy' in captured.out and 'best by expected points' not in captured.out
