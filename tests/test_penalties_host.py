"""Time penalties, host side: the Python restatement of a race with penalties (penalties_ref) against strategy_ref's
finishing orders when there is nothing to add, the C-ABI argument checks of mcgp_run_penalties (no device needed), the
mcgp_time_penalty layout, TimePenalty, PenaltyResult's helpers on hand-made counts and the `penalty` CLI's parsing and
output with a stand-in predictor."""
import ctypes as C
import json

import numpy as np
import pytest

import oracle_py as O
import penalties_ref as PR
import resume_ref as RR
import strategy_ref as SR
from cli_cases import penalty_result as _result
from monte_carlo_gp_amd import PenaltyResult, PitPlan, RaceConfig, StrategyResult, TimePenalty, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, RaceSimulator, _Problem

SERVE, FLAG, LAP = PR.SERVE, PR.FLAG, PR.LAP
H = 2


# ---------------------------------------------------------------- the restatement against strategy_ref
@pytest.mark.parametrize('name', ['S60', 'EVT', 'DMP', 'WET', 'HET'])
def test_restatement_without_penalties_equals_strategy_ref(name):
    case = O.load_case(name)
    seed, m = 17, 48
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    ref = RR.traced_run(case, m, seed, 1000)
    plans = {0: (-1, 0, [(8, H)]), 1 % n: (-1, 0, [(15, 1), (L - 5, 0)]), n - 1: (H, 2, [(L // 2, 0)])}
    for pl in ({}, plans):
        got, fates = PR.orders(case, m, seed, 1000, plans=pl, grids=ref['grids'])
        assert np.array_equal(got, SR.orders(case, m, seed, 1000, plans=pl, grids=ref['grids'])), (name, bool(pl))
        assert (fates == 0).all()
    assert np.array_equal(PR.orders(case, m, seed, 1000, grids=ref['grids'])[0], ref['orders'])
    k = L // 2
    st = (RR.state_arrays(ref, 5, k), k, RR.drs_disabled_until(case, seed, 1005, k))
    for pl in ({}, {0: (-1, 0, [(k + 1, H)])}):
        got, _ = PR.orders(case, 12, seed, 1005, plans=pl, state=st)
        assert np.array_equal(got, SR.orders(case, 12, seed, 1005, plans=pl, state=st)), (name, bool(pl))


def test_restatement_penalties_change_the_race():
    """The additions are not no-ops in the restatement, and each kind lands where the header says."""
    case = O.load_case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    m, seed = 24, 3
    ref = RR.traced_run(case, m, seed)
    base = ref['orders']
    pos = lambda o, d: np.argmax(o == d, axis=1)
    flag, f0 = PR.orders(case, m, seed, penalties=[(0, FLAG, 0, 1e6)], grids=ref['grids'])
    assert (f0 == 0).all() and (pos(flag, 0) >= pos(base, 0)).all() and not np.array_equal(flag, base)
    for i in range(m):                                      # only driver 0's key moved
        assert [d for d in flag[i] if d != 0] == [d for d in base[i] if d != 0]
    late, fl = PR.orders(case, m, seed, penalties=[(0, SERVE, L - 5, 1e6)], grids=ref['grids'])
    assert np.array_equal(late, flag) and set(fl[:, 0]) <= {PR.FATE_FLAG, PR.FATE_RETIRED} and (fl[:, 1:] == 0).all()
    early, fe = PR.orders(case, m, seed, penalties=[(0, SERVE, 2, 5.0)], grids=ref['grids'])
    assert (fe[:, 0] == PR.FATE_SERVED).sum() > m // 2 and not np.array_equal(early, base)
    lap, _ = PR.orders(case, m, seed, penalties=[(0, LAP, 10, 30.0)], grids=ref['grids'])
    assert not np.array_equal(lap, base)


# ---------------------------------------------------------------- the C ABI without a device
def _prob(n=3, laps=60, deviates=32):
    c = O.load_case('S60')
    cfg = dict(c['config'], total_laps=laps)
    return _Problem(RaceConfig(**cfg), [f'D{i:02d}' for i in range(n)], {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)


def _call(penalties=((),), plans=None, n=3, laps=60, state=None, grid=True, n_sims=100, deviates=32, null=(),
          n_scenarios=None, fill=5, device=0):
    prob = _prob(n, laps, deviates)
    penalties = list(penalties)
    plans = list(plans) if plans is not None else [{}] * len(penalties)
    counts, c_plans = SR.c_plans(plans)
    pcounts, c_pens = PR.c_penalties(penalties)
    S = len(penalties) if n_scenarios is None else n_scenarios
    g = np.full((max(n, 1), max(n, 1)), 1.0 / max(n, 1))
    cs = RR.c_state(*state) if state is not None else None
    h = np.full(max(S, 1) * n * n, fill, np.uint64)
    dl = np.full(max(S, 1) * n * (2 * n - 1), fill, np.uint64)
    ft = np.full(max(S, 1) * n * 4, fill, np.uint64)
    o = np.full(max(S, 1) * max(n_sims, 1) * n, fill, np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_penalties(
        None if 'cfg' in null else C.byref(prob.cfg), C.byref(prob.drv),
        g.ctypes.data_as(C.POINTER(C.c_double)) if grid else None, C.byref(cs) if cs is not None else None, n, S,
        None if 'plan_count' in null else counts, None if 'plans' in null else c_plans,
        None if 'penalty_count' in null else pcounts, None if 'penalties' in null else c_pens, n_sims, 0, 1, device,
        None if 'hist' in null else u64(h), u64(dl), u64(ft), o.ctypes.data_as(C.POINTER(C.c_uint8)))
    untouched = (h == fill).all() and (dl == fill).all() and (ft == fill).all() and (o == fill).all()
    return rc, N.lib().mcgp_last_error().decode(), untouched


def _state(n=3, lap=10):
    a = dict(cumulative_time=np.array([100.0 * lap + d for d in range(n)], np.float64),
             last_lap_time=np.full(n, 91.5, np.float64), grid_slot=np.arange(n, dtype=np.uint8),
             compound=np.full(n, 1, np.uint8), used_compounds=np.full(n, 0b011, np.uint8),
             tire_age=np.full(n, 7, np.int16), retired_lap=np.zeros(n, np.int16))
    return (a, lap, 0)


BAD = [
    (dict(penalties=(), n_scenarios=0), 'n_scenarios must be in [1, 64]'),
    (dict(penalties=([],) * 65), 'n_scenarios must be in [1, 64]'),
    (dict(penalties=([], [(1, 3, 5, 5.0)])), 'scenario 1, penalty 0: kind must be'),
    (dict(penalties=([(1, -1, 5, 5.0)],)), 'scenario 0, penalty 0: kind must be'),
    (dict(penalties=([(0, SERVE, 5, 5.0), (3, FLAG, 0, 5.0)],)), 'scenario 0, penalty 1: driver must be in [0, n)'),
    (dict(penalties=([(-1, LAP, 5, 5.0)],)), 'driver must be in [0, n)'),
    (dict(penalties=([(0, SERVE, 1, 5.0)],)), 'penalty 0: lap must be in [2, total_laps] (lap 1 has no pit step)'),
    (dict(penalties=([(0, SERVE, 61, 5.0)],)), 'lap must be in [2, total_laps]'),
    (dict(penalties=([(0, SERVE, 0, 5.0)],)), 'lap must be in [2, total_laps]'),
    (dict(penalties=([(0, LAP, 1, 5.0)],)), 'lap must be in [2, total_laps]'),
    (dict(penalties=([(0, LAP, 61, 5.0)],)), 'lap must be in [2, total_laps]'),
    (dict(penalties=([(0, FLAG, 60, 5.0)],)), 'lap must be 0 with MCGP_PEN_AT_FLAG'),
    (dict(penalties=([(0, SERVE, 20, 5.0)],), state=_state(lap=20), grid=False),
     'lap must be in [21, total_laps] (after the state\'s lap)'),
    (dict(penalties=([(0, LAP, 10, 5.0)],), state=_state(lap=20), grid=False), 'lap must be in [21, total_laps]'),
    (dict(penalties=([(0, LAP, 60, 5.0)],), state=_state(lap=60), grid=False), 'lap must be in [61, total_laps]'),
    (dict(penalties=([(0, FLAG, 0, 0.0)],)), 'seconds must be finite and in (0, 1e6]'),
    (dict(penalties=([(0, FLAG, 0, -5.0)],)), 'seconds must be finite and in (0, 1e6]'),
    (dict(penalties=([(0, FLAG, 0, 1000000.5)],)), 'seconds must be finite and in (0, 1e6]'),
    (dict(penalties=([(0, SERVE, 5, float('nan'))],)), 'seconds must be finite and in (0, 1e6]'),
    (dict(penalties=([(0, LAP, 5, float('inf'))],)), 'seconds must be finite and in (0, 1e6]'),
    (dict(penalties=([(1, SERVE, 5, 5.0), (1, SERVE, 9, 5.0)],)),
     'penalty 1: driver 1 has two MCGP_PEN_SERVE_AT_STOP penalties in this scenario (sum them)'),
    (dict(penalties=([(1, FLAG, 0, 5.0), (0, FLAG, 0, 5.0), (1, FLAG, 0, 10.0)],)),
     'penalty 2: driver 1 has two MCGP_PEN_AT_FLAG penalties in this scenario (sum them)'),
    (dict(penalties=([(2, LAP, 7, 5.0), (2, LAP, 8, 5.0), (2, LAP, 7, 1.0)],)),
     'penalty 2: driver 2 has two MCGP_PEN_ON_LAP penalties on lap 7 in this scenario (sum them)'),
    (dict(penalties=([], [(d % 3, LAP, 2 + k, 1.0) for k in range(59) for d in range(3)] + [(0, LAP, 2, 1.0)] * 80)),
     'scenario 1: penalty_count must be in [0, 256]'),
    (dict(plans=({1: (-1, 0, [(61, H)])},)), 'scenario 0, plan 0: stop 0: stop_lap must be in [2, total_laps]'),
    (dict(plans=({0: (5, 0, [(20, H)])},)), 'plan 0: start_compound must be -1 or in [MCGP_SOFT, MCGP_WET]'),
    (dict(plans=({0: (1, 0, [(20, H)])},), state=_state(), grid=False), 'a state fixes the tyres'),
    (dict(deviates=53), 'MCGP_DEVIATES_32'),
    (dict(null=('hist',)), 'hist_out is NULL'),
    (dict(null=('plan_count',)), 'plan_count is NULL'),
    (dict(null=('penalty_count',)), 'penalty_count is NULL'),
    (dict(plans=({0: (-1, 0, [(20, H)])},), null=('plans',)), 'plans is NULL'),
    (dict(penalties=([(0, FLAG, 0, 5.0)],), null=('penalties',)), 'penalties is NULL'),
    (dict(null=('cfg',)), 'cfg / drv is NULL'),
    (dict(grid=False), 'grid_probs is NULL'),
    (dict(state=_state()), 'grid_probs must be NULL when a state is given'),
    (dict(state=(dict(_state()[0], compound=np.array([7, 1, 1], np.uint8)), 10, 0), grid=False),
     'state 0: car 0: compound'),
    (dict(n=0), 'n must be in [1, 32]'),
    (dict(n=33), 'n must be in [1, 32]'),
]


@pytest.mark.parametrize('kw,msg', BAD, ids=[f'{i}: {m}' for i, (_, m) in enumerate(BAD)])
def test_library_rejects_bad_arguments_before_any_device_lookup(kw, msg):
    """MCGP_E_BAD_ARG naming the scenario, the penalty and the field, on a machine with or without a GPU (device 999 is
    never looked up: the checks come first), and the outputs keep their values."""
    rc, err, untouched = _call(device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert untouched


def test_limits_are_inclusive_and_zero_simulations_need_no_device():
    full = [(d, LAP, 2 + k, 1.0) for k in range(59) for d in range(3)] + [(d, SERVE, 2, 1.0) for d in range(3)] \
        + [(d, FLAG, 0, 1.0) for d in range(3)]
    assert len(full) == 183
    ok = [
        dict(penalties=([],) * 64),
        dict(penalties=([(0, SERVE, 2, 1e6), (0, FLAG, 0, 1e-300), (0, LAP, 2, 5.0), (0, LAP, 60, 5.0)],)),
        dict(penalties=([(2, SERVE, 60, 5.0)],), plans=({2: (-1, 0, [(60, H)])},)),
        dict(penalties=(full,)),
        dict(penalties=(full, [], full)),
        dict(penalties=([(0, SERVE, 11, 5.0), (1, LAP, 11, 5.0), (2, LAP, 60, 5.0)],), state=_state(lap=10), grid=False),
        dict(penalties=([(0, FLAG, 0, 5.0)],), state=_state(lap=60), grid=False),
        dict(null=('plans', 'penalties')),                  # every count is 0
    ]
    for kw in ok:
        rc, err, untouched = _call(n_sims=0, device=999, **kw)
        assert rc == 0 and untouched, (kw, err)
    # 256 penalties in one scenario: 32 cars, 8 laps each
    rc, err, untouched = _call(penalties=([(d, LAP, 2 + k, 1.0) for d in range(32) for k in range(8)],), n=32, n_sims=0,
                               device=999)
    assert rc == 0 and untouched, err
    # with simulations, a valid call gets past the checks to the device lookup
    rc, err, untouched = _call(penalties=([(0, FLAG, 0, 5.0)],), n_sims=10, device=999)
    assert rc == -2 and untouched, err


def test_penalty_struct_matches_the_header():
    assert C.sizeof(N.McgpTimePenalty) == 24
    assert [(f, getattr(N.McgpTimePenalty, f).offset) for f, _ in N.McgpTimePenalty._fields_] == [
        ('driver', 0), ('kind', 4), ('lap', 8), ('seconds', 16)]
    with open(O.ROOT + '/include/mcgp.h') as f:
        header = f.read()
    assert 'enum { MCGP_PEN_SERVE_AT_STOP = 0, MCGP_PEN_AT_FLAG = 1, MCGP_PEN_ON_LAP = 2 };' in header
    assert '#define MCGP_MAX_SCENARIO_PENALTIES 256' in header and '#define MCGP_ABI_VERSION 6' in header
    assert (N.PEN_SERVE_AT_STOP, N.PEN_AT_FLAG, N.PEN_ON_LAP, N.MAX_SCENARIO_PENALTIES) == (0, 1, 2, 256)
    assert 'mcgp_run_penalties' in N.EXPORTS and hasattr(N.lib(), 'mcgp_run_penalties')


# ---------------------------------------------------------------- Python layer
def test_time_penalty_c_struct():
    idx = {'A': 0, 'B': 1}
    p = TimePenalty('B', 5).c_struct(idx)
    assert (p.driver, p.kind, p.lap, p.seconds) == (1, N.PEN_SERVE_AT_STOP, 2, 5.0)
    assert TimePenalty('B', 5).c_struct(idx, first_lap=31).lap == 31
    assert TimePenalty('A', 10, lap=40).c_struct(idx).lap == 40
    p = TimePenalty('A', 5, 'flag').c_struct(idx)
    assert (p.kind, p.lap) == (N.PEN_AT_FLAG, 0)
    p = TimePenalty('A', 21.5, 'lap', 31).c_struct(idx)
    assert (p.kind, p.lap, p.seconds) == (N.PEN_ON_LAP, 31, 21.5)
    with pytest.raises(ValueError, match='kind'):
        TimePenalty('A', 5, 'grid').c_struct(idx)
    with pytest.raises(ValueError, match='no lap'):
        TimePenalty('A', 5, 'flag', 3).c_struct(idx)
    with pytest.raises(ValueError, match='needs its lap'):
        TimePenalty('A', 5, 'lap').c_struct(idx)


def test_two_penalties_of_one_kind_say_to_sum_them():
    c = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=DEFAULT_SET_POP)
    d = list(c['grid_probs'])
    args = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(grid_probs=c['grid_probs'], seed=1)
    for pens in ([TimePenalty(d[0], 5), TimePenalty(d[0], 10, lap=30)],
                 [TimePenalty(d[1], 5, 'flag'), TimePenalty(d[1], 5, 'flag')],
                 [TimePenalty(d[2], 5, 'lap', 9), TimePenalty(d[0], 5, 'lap', 9), TimePenalty(d[2], 7, 'lap', 9)]):
        with pytest.raises(ValueError, match='sum them'):
            sim.run_penalties(0, {'x': pens}, None, *args, **kw)
    with pytest.raises(ValueError, match='not one of the drivers'):
        sim.run_penalties(0, {'x': [TimePenalty('NOBODY', 5)]}, None, *args, **kw)
    # the names are the union of the two dicts, penalties first; zero simulations need no device
    r = sim.run_penalties(0, {'none': [], 'pen': [TimePenalty(d[0], 5), TimePenalty(d[0], 5, 'lap', 9),
                                                  TimePenalty(d[0], 5, 'lap', 10), TimePenalty(d[0], 5, 'flag')]},
                          {'pen': [PitPlan(d[0], [(20, 'HARD')])], 'plan only': [PitPlan(d[1], [(25, 'HARD')])]}, *args, **kw)
    assert r.names == ['none', 'pen', 'plan only'] and r.n_simulations == 0
    assert r.hist.shape == (3, 20, 20) and r.delta.shape == (3, 20, 39) and r.fate.shape == (3, 20, 4)


def test_penalty_result_helpers():
    r = _result()
    assert isinstance(r, StrategyResult)
    assert r.position_probabilities('penalised')['A'] == {1: 0.7, 2: 0.2, 3: 0.1}
    assert r.expected_position('none')['A'] == pytest.approx(1.7)
    assert r.win_probability('penalised', 'A') == pytest.approx(0.7)
    assert r.podium_probability('none', 'C') == pytest.approx(1.0)
    c = r.compare('penalised', 'A')
    assert c['p_better'] == pytest.approx(0.4) and c['p_same'] == pytest.approx(0.5) and c['p_worse'] == pytest.approx(0.1)
    assert r.fate_probabilities('penalised', 'A') == {'none': 0.0, 'served': 0.6, 'at_flag': 0.3, 'retired': 0.1}
    assert r.fate_probabilities('penalised', 'B') == {'none': 1.0, 'served': 0.0, 'at_flag': 0.0, 'retired': 0.0}
    assert r.fate_probabilities('none', 'A')['none'] == 1.0
    with pytest.raises(KeyError):
        r.fate_probabilities('late', 'A')
    with pytest.raises(KeyError):
        r.fate_probabilities('none', 'Z')


# ---------------------------------------------------------------- CLI
def test_cli_give_parsing():
    assert cli.parse_give('NOR:5') == TimePenalty('NOR', 5.0, 'serve', None)
    assert cli.parse_give('NOR:10:serve@31') == TimePenalty('NOR', 10.0, 'serve', 31)
    assert cli.parse_give('NOR:5@31') == TimePenalty('NOR', 5.0, 'serve', 31)
    assert cli.parse_give('VER:5:flag') == TimePenalty('VER', 5.0, 'flag', None)
    assert cli.parse_give('VER:21.5:LAP@31') == TimePenalty('VER', 21.5, 'lap', 31)
    for bad in ('NOR', ':5', 'NOR:x', 'NOR:0', 'NOR:-5', 'NOR:2e6', 'NOR:5:grid', 'NOR:5:flag@3', 'NOR:5:lap', 'NOR:5@x',
                'NOR:5:serve:3'):
        with pytest.raises(ValueError):
            cli.parse_give(bad)
    pens, plans = cli.penalty_scenarios(['NOR:5', 'VER:5:flag'], 'NOR', ['box=:30/HARD'])
    assert list(pens) == ['none', 'penalised', 'penalised + box'] and pens['none'] == []
    assert pens['penalised'] == pens['penalised + box'] == [TimePenalty('NOR', 5.0), TimePenalty('VER', 5.0, 'flag')]
    assert plans == {'penalised + box': [PitPlan('NOR', [(30, 'HARD')])]}
    with pytest.raises(ValueError, match='at least one --give'):
        cli.penalty_scenarios([])
    with pytest.raises(ValueError, match='--driver'):
        cli.penalty_scenarios(['NOR:5'], None, ['box=:30/HARD'])
    with pytest.raises(ValueError, match='twice'):
        cli.penalty_scenarios(['NOR:5'], 'NOR', ['box=:30/HARD', 'box=:31/HARD'])


def test_penalty_cli_with_a_stand_in_predictor(tmp_path, capsys, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, device=0):
            pass

        def predict_penalties(self, season, race, fixture, penalties, strategies=None, state=None, n_simulations=0,
                              seed=None, allow_single_compound=False):
            seen.update(penalties=penalties, strategies=strategies, n=n_simulations, seed=seed, state=state)
            r = _result()
            return PenaltyResult(names=list(penalties)[:2], drivers=r.drivers, n_simulations=10, hist=r.hist,
                                 delta=r.delta, fate=r.fate)

    monkeypatch.setattr(cli, 'F1Predictor', Fake)
    out = tmp_path / 'p.json'
    rc = cli.main(['penalty', '--race', 'Bahrain', '--offline', '--give', 'A:5', '--simulations', '10', '--seed', '3',
                   '--json', str(out)])
    assert rc == 0
    assert list(seen['penalties']) == ['none', 'penalised'] and seen['n'] == 10 and seen['seed'] == 3
    assert seen['penalties']['penalised'] == [TimePenalty('A', 5.0)] and seen['strategies'] == {}
    text = capsys.readouterr().out
    assert 'scenario: none' in text and 'scenario: penalised' in text and 'served' in text
    doc = json.load(open(out))
    assert doc['penalised'] == ['A'] and [r['scenario'] for r in doc['scenarios']] == ['none', 'penalised']
    a = doc['scenarios'][1]['drivers']['A']
    assert a['win'] == pytest.approx(0.7) and a['p_better'] == pytest.approx(0.4)
    assert a['fate'] == {'none': 0.0, 'served': 0.6, 'at_flag': 0.3, 'retired': 0.1}
    assert doc['scenarios'][0]['win_probabilities']['B'] == pytest.approx(0.3)
    assert doc['scenarios'][0]['expected_position']['A'] == pytest.approx(1.7)
    assert cli.main(['penalty', '--race', 'Bahrain', '--offline']) == 2                     # nothing given
    assert cli.main(['penalty', '--race', 'Bahrain', '--offline', '--give', 'A:five']) == 2
    assert cli.main(['penalty', '--race', 'Bahrain', '--offline', '--give', 'A:5', '--plan', 'x=:30/HARD']) == 2
