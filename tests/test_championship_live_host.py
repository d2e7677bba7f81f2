"""Live title odds, host side: the argument checks of mcgp_run_championship_live (none needs a device), the Python layer's
errors and ChampionshipResult's title_given methods on a hand-made table, the restatement on a season worked out by hand,
and the CLI options on a fake result."""
import ctypes as C
import json
import types

import numpy as np
import pytest

import championship_live_ref as LR
import championship_ref as CR
import oracle_py as O
from monte_carlo_gp_amd import ChampionshipResult, RaceConfig, RaceState, cli, run_championship
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import simulation as S


# ---------------------------------------------------------------- the restatement
def test_three_drivers_two_races_by_hand():
    """Table [3, 2, 1] twice, four simulations, the given race is race 1.
    sim 0: A B C, A B C -> A 6: champion A.      sim 1: A B C, B A C -> A 5, B 5, a win and a second each: A on the index.
    sim 2: B A C, B C A -> B 6: champion B.      sim 3: C B A, C A B -> C 6: champion C."""
    orders = [np.array([[0, 1, 2], [0, 1, 2], [1, 0, 2], [2, 1, 0]], np.uint8),
              np.array([[0, 1, 2], [1, 0, 2], [1, 2, 0], [2, 0, 1]], np.uint8)]
    out = LR.title_given(orders, [[3, 2, 1]] * 2, [1, 1], 1)
    want = np.zeros((3, 3, 3), np.int64)
    for d, p, e in ((0, 0, 0), (1, 1, 0), (2, 2, 0), (1, 0, 0), (0, 1, 0), (2, 2, 0), (1, 0, 1), (2, 1, 1), (0, 2, 1),
                    (2, 0, 2), (0, 1, 2), (1, 2, 2)):
        want[d, p, e] += 1
    assert np.array_equal(out, want)
    # a bonus of 2 points for B in race 0 of sim 1 makes B champion there
    bonus = np.zeros((2, 4, 3), np.int64)
    bonus[0, 1, 1] = 2
    with_bonus = LR.title_given(orders, [[3, 2, 1]] * 2, [1, 1], 1, bonus=bonus)
    assert np.array_equal(LR.title_given_of(orders[1], LR.champions(orders, [[3, 2, 1]] * 2, [1, 1], bonus=bonus)), with_bonus)
    rng = np.random.default_rng(1)
    many = [rng.permuted(np.tile(np.arange(7, dtype=np.uint8), (300, 1)), axis=1) for _ in range(3)]
    for rank in (CR.rank, CR.rank_grouped, CR.rank_lexsort):
        champ = LR.champions(many, [[3, 2, 1]] * 3, [1, 0, 1], rank=rank)
        assert np.array_equal(LR.title_given_of(many[2], champ), LR.title_given(many, [[3, 2, 1]] * 3, [1, 0, 1], 2))
    assert with_bonus[1, 0].tolist() == [0, 2, 0] and with_bonus[0, 1].tolist() == [0, 1, 1]


# ---------------------------------------------------------------- the Python result
def _result(**kw):
    base = dict(drivers=['A', 'B', 'C'], teams=['X', 'Y'], n_simulations=10, champ_hist=np.zeros((3, 3), np.int64),
                team_hist=np.zeros((2, 2), np.int64), gain_hist=np.zeros((3, 1), np.int64), initial_points={})
    base.update(kw)
    return ChampionshipResult(**base)


def test_title_methods_on_a_hand_made_table():
    table = np.zeros((3, 3, 3), np.int64)
    table[0, 0] = [4, 0, 0]                 # A wins 4 times: champion every time
    table[0, 1] = [1, 3, 0]                 # A second 4 times: champion once, B three times
    table[0, 2] = [0, 1, 1]                 # A third twice: never champion
    table[1, 0] = [1, 4, 1]                 # B wins 6 times (and never finishes third)
    table[1, 1] = [4, 0, 0]
    res = _result(title_given=table, given_race=0)
    assert res.title_probability_given('A', 1) == 1.0 and res.title_probability_given('A', 2) == 0.25
    assert res.title_probability_given('A', 2, champion='B') == 0.75 and res.title_probability_given('A', 3) == 0.0
    assert res.title_probability_given('B', 3) is None                 # no simulation has that finish
    assert res.title_probability_given('C', 1, champion='A') is None
    assert res.title_needs('A') == {1: 1.0, 2: 0.25, 3: 0.0} and res.title_needs('B') == {1: 4 / 6, 2: 0.0}
    assert res.title_needs('C') == {}
    with pytest.raises(ValueError, match='position'):
        res.title_probability_given('A', 4)
    with pytest.raises(KeyError):
        res.title_needs('Z')
    assert cli.title_needs_table(res, 'A')[2] == dict(p_finish=0.4, count=4, title={'A': 0.25, 'B': 0.75})


def test_title_methods_need_the_table():
    res = _result()
    assert res.title_given is None and res.given_race is None
    with pytest.raises(ValueError, match='not counted'):
        res.title_probability_given('A', 1)
    with pytest.raises(ValueError, match='not counted'):
        res.title_needs('A')


# ---------------------------------------------------------------- the Python layer
def _race(name, **kw):
    case = O.load_case(name)
    race = dict(config=RaceConfig(**case['config']), grid_probs=case['grid_probs'], base_pace=case['base_pace'],
                tire_deg=case['tire_deg'], driver_variance=case['driver_variance'],
                driver_dnf_rates=case['driver_dnf_rates'], track_condition=case['track_condition'])
    race.update(kw)
    return race


def _state(drivers, lap=30, **kw):
    """A plain state after `lap` laps: the cars in `drivers` order a second apart, on 20-lap-old mediums."""
    cars = [dict(driver=d, cumulative_time=90.0 * lap + i, last_lap_time=90.0, tire_compound='MEDIUM', tire_age=20,
                 used_compounds=['MEDIUM'], retired_lap=0) for i, d in enumerate(drivers)]
    obj = dict(lap=lap, drs_disabled_until=0, cars=cars)
    obj.update(kw)
    return RaceState.from_json(obj)


def _live_race(name, state, **kw):
    race = _race(name, **kw)
    del race['grid_probs']
    race['state'] = state
    return race


def test_python_layer_without_running():
    """n_simulations = 0 goes through every argument check of the new entry point and returns before any device."""
    drivers = [str(d) for d in O.load_case('S60')['grid_probs']]
    st = _state(drivers[::-1])
    res = run_championship([_live_race('S60', st, seed=5), _race('S78', seed=6)], 0, given_race=1, by_round=True)
    assert res.drivers == drivers[::-1]                                 # the state's grid order
    assert res.title_given.shape == (20, 20, 20) and res.given_race == 1 and res.round_hist.shape == (2, 20, 20)
    res = run_championship([_live_race('S60', st, seed=5), _race('S78', seed=6, fastest_lap_points=1)], 0, drivers=drivers)
    assert res.drivers == drivers and res.title_given is None and res.bonus_counts.shape == (2, 20)
    res = run_championship([_race('S60', seed=5), _race('S78', seed=6)], 0, given_race=0)
    assert res.title_given.shape == (20, 20, 20) and res.given_race == 0 and res.bonus_counts is None
    plain = run_championship([_race('S60', seed=5), _race('S78', seed=6)], 0)
    assert plain.title_given is None and plain.given_race is None


def test_python_layer_errors():
    drivers = [str(d) for d in O.load_case('S60')['grid_probs']]
    st = _state(drivers)
    with pytest.raises(ValueError, match='either state or grid_probs'):
        run_championship([_race('S60', state=st)], 0)
    with pytest.raises(ValueError, match='race 1: only the first race'):
        run_championship([_race('S60'), _live_race('S78', st)], 0)
    with pytest.raises(ValueError, match='deviates=32'):
        run_championship([_live_race('S60', st, deviates=53)], 0)
    with pytest.raises(ValueError, match='fastest-lap bonus'):
        run_championship([_live_race('S60', st, fastest_lap_points=1)], 0)
    for bad in (-1, 2, 99):
        with pytest.raises(ValueError, match='given_race'):
            run_championship([_race('S60'), _race('S78')], 0, given_race=bad)
    with pytest.raises(ValueError, match="differ from the first race's"):
        run_championship([_live_race('S60', _state(drivers[:19] + ['ZZZ'])), _race('S78')], 0)
    # the state's own messages are RaceState.arrays'
    with pytest.raises(ValueError, match=r'lap must be in \[1, total_laps\]'):
        run_championship([_live_race('S60', _state(drivers, lap=61))], 0)
    with pytest.raises(ValueError, match='are not the drivers'):
        run_championship([_live_race('S60', st)], 0, drivers=drivers[:19] + ['ZZZ'])
    bad = _state(drivers)
    bad.cars[3].tire_compound = 'SUPERSOFT'
    with pytest.raises(ValueError, match='tire_compound'):
        run_championship([_live_race('S60', bad)], 0)


def test_a_library_without_the_symbol_is_a_clear_error(monkeypatch):
    real = N.lib()
    assert 'mcgp_run_championship_live' in N.EXPORTS and hasattr(real, 'mcgp_run_championship_live')
    old = types.SimpleNamespace(**{k: getattr(real, k) for k in N.EXPORTS if k != 'mcgp_run_championship_live'})
    monkeypatch.setattr(S.N, 'lib', lambda: old)
    drivers = [str(d) for d in O.load_case('S60')['grid_probs']]
    with pytest.raises(N.McgpError, match='mcgp_run_championship_live'):
        run_championship([_race('S60', seed=5)], 0, given_race=0)
    with pytest.raises(N.McgpError, match='mcgp_run_championship_live'):
        run_championship([_live_race('S60', _state(drivers), seed=5)], 0)
    # the other calls do not need it
    assert run_championship([_race('S60', seed=5, fastest_lap_points=1)], 0, by_round=True).title_given is None


# ---------------------------------------------------------------- the library's argument checks
ROUND_TRIO = ('round_hist', 'contend_out', 'secure_out')
TEAM_TRIO = ('team_round_hist', 'team_contend_out', 'team_secure_out')
NAMES = ('champ_hist', 'team_hist', 'gain_hist', 'race_hist') + ROUND_TRIO + TEAM_TRIO + ('bonus_hist', 'fastest_hist',
                                                                                          'title_given_out')


def _abi_call(drop=(), n=3, n_races=2, n_sims=100, bonus=(0, 1), within=(0, 3), deviates=0, state=None, given_race=-1,
              grid0=None, state_edit=None):
    """mcgp_run_championship_live on a small season.  state: None (from the grid) or a lap; grid0: whether grid_probs[0] is
    given (default: exactly when there is no state); title_given_out is given exactly when given_race != -1 unless `drop`
    / 'keep_title' say otherwise; state_edit(arrays, c_state) spoils the state."""
    lib = N.lib()
    case = O.load_case('S60')
    drivers = [f'D{i:02d}' for i in range(n)]
    prob = S._Problem(RaceConfig(**case['config']), drivers, {}, {}, {}, None, 'dry', S.DEFAULT_SET_POP, 32)
    prob0 = S._Problem(RaceConfig(**case['config']), drivers, {}, {}, {}, None, 'dry', S.DEFAULT_SET_POP, 53 if deviates else 32)
    g = np.full((n, n), 1.0 / n)
    R = n_races
    cfgs = (N.McgpConfig * R)(*([prob0.cfg] + [prob.cfg] * (R - 1)))
    drvs = (N.McgpDrivers * R)(*[prob.drv] * R)
    if grid0 is None:
        grid0 = state is None
    grids = (C.POINTER(C.c_double) * R)(*([S._dptr(g) if grid0 else C.POINTER(C.c_double)()] + [S._dptr(g)] * (R - 1)))
    seeds = (C.c_uint64 * R)(*range(R))
    pts = np.ascontiguousarray([[3, 2, 1][:n] + [0] * max(0, n - 3)] * R, np.int32)
    cb = np.ones(R, np.uint8)
    tm = np.ascontiguousarray([i % 2 for i in range(n)], np.int32)
    bp, bw = np.ascontiguousarray(bonus, np.int32), np.ascontiguousarray(within, np.int32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    bufs = {k: np.full(64 * 32 * 32, 0xDEAD, np.uint64) for k in NAMES}
    title = ('keep_title' in drop) or (given_race != -1 and 'title_given_out' not in drop)
    ptr = lambda k: None if k in drop or (k == 'title_given_out' and not title) else bufs[k].ctypes.data_as(C.POINTER(C.c_uint64))
    c_state = arrays = None
    if state is not None:
        st = _state(drivers, lap=state)
        arrays = st.arrays(drivers)
        c_state = st.c_struct(arrays)
        if state_edit:
            state_edit(arrays, c_state)
    rc = lib.mcgp_run_championship_live(
        R, cfgs, drvs, grids, n, n_sims, 0, seeds, i32(pts), cb.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, i32(tm),
        min(n, 2), 0, *[ptr(k) for k in NAMES[:10]], None if 'bonus_points' in drop else i32(bp),
        None if 'bonus_within' in drop else i32(bw), ptr('bonus_hist'), ptr('fastest_hist'),
        C.byref(c_state) if c_state is not None else None, given_race, ptr('title_given_out'))
    err = lib.mcgp_last_error().decode()
    assert all((b == 0xDEAD).all() for b in bufs.values())          # no call here reaches a device: nothing is written
    if state is not None and rc != 0:
        # what mcgp_run_from_state says about the same race and state
        hist = np.zeros((n, n), np.uint64)
        rc2 = lib.mcgp_run_from_state(C.byref(prob0.cfg), C.byref(prob.drv), n, 1, C.byref(c_state), 0, None, 0, 0,
                                      hist.ctypes.data_as(C.POINTER(C.c_uint64)), None)
        return rc, err, (rc2, lib.mcgp_last_error().decode())
    return rc, err, None


def test_library_names_the_argument():
    cases = [(dict(given_race=-2), 'given_race'), (dict(given_race=2), 'given_race'), (dict(given_race=64), 'given_race'),
             (dict(given_race=-1, drop=('keep_title',)), 'title_given_out'),
             (dict(given_race=0, drop=('title_given_out',)), 'title_given_out'),
             (dict(state=30, grid0=True), 'grid_probs'), (dict(state=30, deviates=1), 'deviates'),
             (dict(state=30, bonus=(1, 0), within=(3, 0)), 'bonus_points[0]'),
             (dict(grid0=False), 'grid_probs'),                              # without a state the grid is required, as before
             (dict(bonus=(0, -1)), 'bonus_points[1]'), (dict(drop=('bonus_points',)), 'bonus_points'),
             (dict(drop=('round_hist',)), 'round_hist'), (dict(drop=ROUND_TRIO), 'team_round_hist'),
             (dict(drop=('champ_hist',)), 'NULL')]
    for kw, msg in cases:
        rc, err, _ = _abi_call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    assert 'MCGP_DEVIATES_32' in _abi_call(state=30, deviates=1)[1]


def test_state_fields_are_rejected_with_the_resumed_race_s_own_messages():
    def lap0(arrays, st):
        st.lap = 0

    def lap_past(arrays, st):
        st.lap = 61

    def drs(arrays, st):
        st.drs_disabled_until = 63

    def slots(arrays, st):
        arrays['grid_slot'][:] = 0

    def compound(arrays, st):
        arrays['compound'][1] = 7

    def used(arrays, st):
        arrays['used_compounds'][2] = 1

    def age(arrays, st):
        arrays['tire_age'][0] = 1023

    def retired(arrays, st):
        arrays['retired_lap'][1] = 31

    def time(arrays, st):
        arrays['cumulative_time'][2] = np.inf

    def null(arrays, st):
        st.tire_age = None

    for edit in (lap0, lap_past, drs, slots, compound, used, age, retired, time, null):
        rc, err, resumed = _abi_call(state=30, state_edit=edit)
        assert rc == -1 and resumed == (-1, err), (edit.__name__, rc, err, resumed)
    assert _abi_call(state=30, deviates=1)[2] == (-1, _abi_call(state=30, deviates=1)[1])


def test_what_passes_the_checks_without_a_device():
    """Zero simulations: every check runs and no device is looked up."""
    assert _abi_call(n_sims=0)[0] == 0
    assert _abi_call(n_sims=0, state=30)[0] == 0
    assert _abi_call(n_sims=0, state=60)[0] == 0 and _abi_call(n_sims=0, state=1)[0] == 0
    for g in (0, 1):
        assert _abi_call(n_sims=0, state=30, given_race=g)[0] == 0 and _abi_call(n_sims=0, given_race=g)[0] == 0
    assert _abi_call(n_sims=0, state=30, drop=('bonus_points', 'bonus_within', 'bonus_hist', 'fastest_hist'))[0] == 0
    assert _abi_call(n_sims=0, drop=('bonus_points', 'bonus_within') + ROUND_TRIO + TEAM_TRIO, given_race=1)[0] == 0
    assert _abi_call(n_sims=0, state=30, bonus=(0, 0), drop=TEAM_TRIO + ('race_hist',))[0] == 0
    assert _abi_call(n_sims=0, n=1, n_races=1, bonus=(0,), within=(0,), state=5, given_race=0)[0] == 0


# ---------------------------------------------------------------- the CLI options
def test_cli_parses_state_and_needs(monkeypatch, tmp_path, capsys):
    seen = []

    def fake_run(races, n_simulations, **kw):
        seen.append((kw, [('state' in r, 'grid_probs' in r) for r in races]))
        drivers = kw.get('drivers') or [str(d) for d in races[0]['grid_probs']]
        n, R = len(drivers), len(races)
        hist = np.zeros((n, n), np.int64)
        hist[np.arange(n), np.arange(n)] = n_simulations
        table = None
        if kw.get('given_race') is not None:
            table = np.zeros((n, n, n), np.int64)
            table[np.arange(n), np.arange(n), 0] = n_simulations - 4    # everybody always finishes in index order
            table[np.arange(n), np.arange(n), 1] = 3
            table[np.arange(n), np.arange(n), 2] = 1
        return ChampionshipResult(
            drivers=drivers, teams=['X', 'Y'], n_simulations=n_simulations, champ_hist=hist,
            team_hist=np.diag([n_simulations] * 2), gain_hist=np.full((n, 1), n_simulations, np.int64), initial_points={},
            race_histograms=[hist] * R, team_index=[i % 2 for i in range(n)], title_given=table, given_race=kw.get('given_race'))

    monkeypatch.setattr(S, 'run_championship', fake_run)
    out = tmp_path / 'c.json'
    base = ['championship', '--season', '2024', '--from-round', '23', '--simulations', '10', '--seed', '3', '--json', str(out)]
    assert cli.main(base) == 0
    plain = json.loads(out.read_text())
    assert 'drivers' not in seen[-1][0] and 'given_race' not in seen[-1][0] and 'title_needs' not in plain
    field = plain['drivers']
    state_file = tmp_path / 'lap40.json'
    state_file.write_text(json.dumps(_state(field[::-1], lap=40).to_json()))
    a, b = field[0], field[1]
    capsys.readouterr()
    assert cli.main(base + ['--state', str(state_file), '--needs', a, '--needs', b]) == 0
    text = capsys.readouterr().out
    kw, shape = seen[-1]
    assert kw['given_race'] == 0 and kw['drivers'] == field and shape == [(True, False), (False, True)]
    assert f'WHAT {a} NEEDS (round 23' in text and f'WHAT {b} NEEDS (round 23' in text and 'after lap 40' in text
    assert "finish  P(finish)  P(title | finish)  rivals' title odds given that finish" in text
    block = json.loads(out.read_text())
    assert {k: block[k] for k in plain} == plain                     # every other key keeps its value
    assert block['state_lap'] == 40 and block['given_round'] == 23 and sorted(block['title_needs']) == sorted([a, b])
    assert block['title_needs'][a] == {'1': {'p_finish': 1.0, 'title': {a: 0.6, b: 0.3, field[2]: 0.1}}}
    assert block['title_needs'][b]['2']['title'][b] == 0.3
    assert cli.main(base + ['--needs', a, '--needs-round', '24']) == 0
    assert seen[-1][0]['given_race'] == 1 and 'drivers' not in seen[-1][0]
    assert json.loads(out.read_text())['given_round'] == 24 and 'state_lap' not in json.loads(out.read_text())
    for bad in (['--needs', a, '--needs-round', '22'], ['--needs', a, '--needs-round', '25'], ['--needs-round', '23'],
                ['--needs', 'NOBODY']):
        with pytest.raises(ValueError):
            cli.main(base + bad)
