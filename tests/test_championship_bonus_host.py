"""The fastest-lap bonus, host side: the restatement's own consistency (championship_bonus_ref) on seasons worked out by
hand and against the figures the rule was priced with, the bounds with the bonuses still to come, ChampionshipResult's
bonus properties on fabricated counts, the Python layer and the CLI flag without a device, and the argument checks of
mcgp_run_championship_bonus, which need none."""
import ctypes as C
import types

import numpy as np
import pytest

import championship_bonus_ref as BR
import championship_cases as CC
import championship_ref as CR
import championship_rounds_ref as RR
import oracle_py as O
import resume_ref as RS
from monte_carlo_gp_amd import ChampionshipResult, RaceConfig, cli, run_championship
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import simulation as S

F1 = [25, 18, 15, 12, 10, 8, 6, 4, 2, 1]


# ---------------------------------------------------------------- the restatement
def _hand_race(orders, fl_driver):
    orders = np.array(orders, np.uint8)
    d = np.array(fl_driver, np.int64)
    pos = np.where(d >= 0, (orders.astype(np.int64) == d[:, None]).argmax(axis=1), BR.NONE)
    return dict(orders=orders, fl_driver=d, fl_pos=pos, fl_retired=np.zeros(len(d), bool))


def test_three_drivers_two_races_by_hand():
    """Table [3, 2, 1], bonus 1 within 2 in both races, four simulations.
    sim 0: A B C twice, A fastest twice            -> A 8, B 4, C 2.
    sim 1: A B C then B A C, C fastest (3rd: none) -> A 5, B 5, C 2; one win each, one second each: A on the index.
    sim 2: as sim 1, B fastest in race 1           -> A 5, B 6, C 2: the bonus makes B champion.
    sim 3: no fastest lap in race 0, A in race 1 (2nd: inside) -> A 6, B 5."""
    races = [_hand_race([[0, 1, 2]] * 4, [0, 2, 2, -1]), _hand_race([[0, 1, 2], [1, 0, 2], [1, 0, 2], [1, 0, 2]], [0, 2, 1, 0])]
    out = BR.season(races, [[3, 2, 1]] * 2, [1, 1], [0, 1, 0], 2, [1, 1], [2, 2])
    assert out['final'][0].tolist() == [[8, 4, 2], [5, 5, 2], [5, 6, 2], [6, 5, 2]]
    assert out['champ_hist'].tolist() == [[3, 1, 0], [1, 3, 0], [0, 0, 4]]
    assert out['fastest_hist'].tolist() == [[1, 0, 2], [2, 1, 1]] and out['bonus_hist'].tolist() == [[1, 0, 0], [2, 1, 0]]
    assert out['gain_hist'].shape == (3, 3 + 3 + 2 + 1) and out['gain_hist'][0].tolist() == [0, 0, 0, 0, 0, 2, 1, 0, 1]
    # by round: M_0 = 3 + 1: after race 0 of sim 0 A has 4, B 2, C 1: all within 4; without the bonus to come C (3
    # behind) would be the last one in, with it nobody is out
    assert out['contend'][0].tolist() == [4, 4, 4] and out['secure'][1].tolist() == [3, 1, 0]
    changed = BR.changed_by_the_bonus(races, [[3, 2, 1]] * 2, [1, 1], [0, 1, 0], 2, [1, 1], [2, 2])
    assert changed == dict(champions=1, standings=1, champ_cells=4)


def test_the_loop_and_the_lap_at_a_time_version_agree():
    for name, m, seed in (('S60', 40, 1), ('EVT', 64, 42), ('WET', 24, 9), ('N10', 40, 42)):
        ref = RS.traced_run(O.load_case(name), m, seed, 11)
        for a, b in zip(BR.fastest_lap(ref), BR.fastest_lap_loop(ref)):
            assert np.array_equal(a, b), name


@pytest.fixture(scope='module')
def s60_races():
    case = O.load_case('S60')
    return case, [BR.race(case, 256, s) for s in (1, 2, 3)]


def test_the_price_of_leaving_the_rule_out(s60_races):
    """The figures of the feature's motivation: S60 under seeds 1, 2, 3, 256 simulations, 1 point within the top ten."""
    case, races = s60_races
    team, T = CC.team_of(dict(case=case))
    changed = BR.changed_by_the_bonus(races, [F1] * 3, [1] * 3, team, T, [1] * 3, [10] * 3)
    assert changed == dict(champions=6, standings=31, champ_cells=37)


def test_zero_bonus_is_the_plain_season(s60_races):
    case, races = s60_races
    team, T = CC.team_of(dict(case=case))
    orders = [r['orders'] for r in races]
    out = BR.season(races, [F1] * 3, [1, 0, 1], team, T, [0] * 3, [10] * 3)
    champ, teams, gain, rh = CR.championship(orders, [F1] * 3, [1, 0, 1], team, T, grouped='lexsort')
    assert np.array_equal(out['champ_hist'], champ) and np.array_equal(out['team_hist'], teams)
    assert np.array_equal(out['gain_hist'], gain) and np.array_equal(out['race_hist'], rh)
    plain = RR.rounds(orders, [F1] * 3, [1, 0, 1], team, T)
    for k in RR.KEYS:
        assert np.array_equal(out[k], plain[k]), k
    assert not out['bonus_hist'].any() and not out['fastest_hist'].any()


def test_identities_with_the_bonus(s60_races):
    case, races = s60_races
    team, T = CC.team_of(dict(case=case))
    out = BR.season(races, [F1] * 3, [1] * 3, team, T, [1, 0, 2], [10, 10, 3])
    RR.assert_identities(out, 256, out['champ_hist'], out['team_hist'])
    assert (out['gain_hist'].sum(axis=1) == 256).all() and out['gain_hist'].shape[1] == 75 + 3 + 1
    assert (out['bonus_hist'] <= out['fastest_hist']).all() and (out['fastest_hist'].sum(axis=1) == [256, 0, 256]).all()
    g = np.arange(out['gain_hist'].shape[1])
    table_points = sum(F1) * 3 * 256
    assert int((out['gain_hist'] * g).sum()) == table_points + int(out['bonus_hist'][0].sum()) + 2 * int(out['bonus_hist'][2].sum())
    for s in out['per']:                                            # whoever is secure at r is the final champion
        assert not (s['secure'] & ~out['per'][-1]['secure']).any()


def test_remaining_points_include_the_bonuses_to_come():
    M, B = BR.remaining([[3, 2, 1]] * 3, 4, [0, 0, 1, 1], 2, [1, 0, 2])
    assert list(M) == [3 + 3 + 2, 3 + 2, 0] and B.tolist() == [[10 + 2] * 2, [5 + 2] * 2, [0, 0]]


# ---------------------------------------------------------------- the Python result
def _result(**kw):
    base = dict(drivers=['A', 'B', 'C'], teams=['X', 'Y'], n_simulations=10, champ_hist=np.zeros((3, 3), np.int64),
                team_hist=np.zeros((2, 2), np.int64), gain_hist=np.zeros((3, 1), np.int64), initial_points={})
    base.update(kw)
    return ChampionshipResult(**base)


def test_bonus_properties_from_fabricated_counts():
    res = _result(bonus_counts=np.array([[5, 3, 0], [0, 0, 0], [2, 2, 4]]), fastest_lap_counts=np.array([[6, 3, 1], [0, 0, 0], [2, 3, 5]]),
                  bonus_points=[1, 0, 2], team_index=[0, 1, 0])
    assert res.bonus_probabilities_by_round == [{'A': 0.5, 'B': 0.3, 'C': 0.0}, {'A': 0.0, 'B': 0.0, 'C': 0.0},
                                                {'A': 0.2, 'B': 0.2, 'C': 0.4}]
    assert res.expected_bonus_points == {'A': 0.9, 'B': 0.7, 'C': 0.8}
    assert res.expected_constructor_bonus_points == {'X': pytest.approx(1.7), 'Y': 0.7}


def test_bonus_properties_need_a_bonus():
    res = _result()
    assert res.bonus_counts is None and res.fastest_lap_counts is None
    for name in ('bonus_probabilities_by_round', 'expected_bonus_points', 'expected_constructor_bonus_points'):
        with pytest.raises(ValueError, match='fastest_lap_points'):
            getattr(res, name)


def _race(name, **kw):
    case = O.load_case(name)
    return dict(config=RaceConfig(**case['config']), grid_probs=case['grid_probs'], base_pace=case['base_pace'],
                tire_deg=case['tire_deg'], driver_variance=case['driver_variance'],
                driver_dnf_rates=case['driver_dnf_rates'], track_condition=case['track_condition'], **kw)


def test_python_layer_reads_the_two_keys_without_running():
    """n_simulations = 0 goes through every argument check of the new entry point and returns before any device."""
    races = [_race('S60', seed=5, fastest_lap_points=1), _race('S78', seed=6), _race('S50', seed=7, fastest_lap_points=2, fastest_lap_within=99)]
    res = run_championship(races, 0, by_round=True)
    assert res.bonus_counts.shape == (3, 20) == res.fastest_lap_counts.shape and res.bonus_points == [1, 0, 2]
    assert res.gain_hist.shape == (20, 75 + 3 + 1) and res.round_hist.shape == (3, 20, 20)
    assert res.team_index == [res.teams.index(races[0]['config'].driver_teams.get(d, 'Unknown')) for d in res.drivers]
    assert run_championship(races, 0).round_hist is None
    plain = run_championship([_race('S60', seed=5), _race('S78', seed=6)], 0)
    assert plain.bonus_counts is None and plain.gain_hist.shape == (20, 51)
    with pytest.raises(ValueError, match='fastest_lap_points'):
        run_championship([_race('S60', seed=5, fastest_lap_points=-1)], 0)
    with pytest.raises(ValueError, match='fastest_lap_within'):
        run_championship([_race('S60', seed=5, fastest_lap_points=1, fastest_lap_within=0)], 0)
    with pytest.raises(ValueError, match='65535'):
        run_championship([_race('S60', seed=5, fastest_lap_points=1)], 0, standings={res.drivers[0]: 65535 - 25})
    with pytest.raises(N.McgpError, match='MCGP_DEVIATES_32'):
        run_championship([_race('S60', seed=5, fastest_lap_points=1, deviates=53)], 0)


def test_a_library_without_the_symbol_is_a_clear_error(monkeypatch):
    real = N.lib()
    assert 'mcgp_run_championship_bonus' in N.EXPORTS and hasattr(real, 'mcgp_run_championship_bonus')
    old = types.SimpleNamespace(**{k: getattr(real, k) for k in N.EXPORTS if k != 'mcgp_run_championship_bonus'})
    monkeypatch.setattr(S.N, 'lib', lambda: old)
    with pytest.raises(N.McgpError, match='mcgp_run_championship_bonus'):
        run_championship([_race('S60', seed=5, fastest_lap_points=1)], 0)
    assert run_championship([_race('S60', seed=5)], 0, by_round=True).bonus_counts is None   # the other calls do not need it


# ---------------------------------------------------------------- the CLI flag on a fake result
def test_cli_fastest_lap_point_on_a_fake_result(monkeypatch, tmp_path, capsys):
    import json
    seen = []

    def fake_run(races, n_simulations, **kw):
        seen.append([(r.get('fastest_lap_points', 0), r.get('fastest_lap_within')) for r in races])
        drivers = [str(d) for d in races[0]['grid_probs']]
        n, R = len(drivers), len(races)
        teams = ['X', 'Y']
        hist = np.zeros((n, n), np.int64)
        hist[np.arange(n), np.arange(n)] = n_simulations
        bonus = seen[-1][0][0] > 0
        counts = np.zeros((R, n), np.int64)
        counts[:, 0], counts[:, 1] = 6, 4
        return ChampionshipResult(
            drivers=drivers, teams=teams, n_simulations=n_simulations, champ_hist=hist, team_hist=np.diag([n_simulations] * 2),
            gain_hist=np.full((n, 1), n_simulations, np.int64), initial_points={}, race_histograms=[hist] * R,
            team_index=[i % 2 for i in range(n)], bonus_counts=counts // 2 if bonus else None,
            fastest_lap_counts=counts if bonus else None, bonus_points=[1] * R if bonus else None)

    monkeypatch.setattr(S, 'run_championship', fake_run)
    out = tmp_path / 'c.json'
    base = ['championship', '--season', '2024', '--from-round', '23', '--simulations', '10', '--seed', '3', '--json', str(out)]
    assert cli.main(base) == 0
    text = capsys.readouterr().out
    plain = json.loads(out.read_text())
    assert 'FASTEST-LAP POINT' not in text and 'fastest_lap_point' not in plain
    assert cli.main(base + ['--fastest-lap-point']) == 0
    text = capsys.readouterr().out
    assert seen == [[(0, None)] * 2, [(1, 10)] * 2]
    assert 'FASTEST-LAP POINT (1 point within the top 10, every round)' in text
    block = json.loads(out.read_text())
    assert {k: block[k] for k in plain} == plain                     # every other key keeps its value
    fl = block['fastest_lap_point']
    first, second = list(fl['expected_bonus_points'])[:2]
    assert fl['points'] == 1 and fl['within'] == 10 and fl['expected_bonus_points'][first] == 0.6
    assert fl['expected_constructor_bonus_points'] == {'X': 0.6, 'Y': 0.4}
    assert len(fl['bonus_probabilities_by_round']) == 2 and fl['fastest_lap_probabilities_by_round'][1][second] == 0.4


# ---------------------------------------------------------------- the library's argument checks
def _abi_call(drop=(), n=3, n_races=2, n_sims=100, bonus=(1, 0), within=(3, 0), deviates=0, init=None, **kw):
    lib = N.lib()
    case = O.load_case('S60')
    drivers = [f'D{i:02d}' for i in range(n)]
    prob = S._Problem(RaceConfig(**case['config']), drivers, {}, {}, {}, None, 'dry', S.DEFAULT_SET_POP, 53 if deviates else 32)
    g = np.full((n, n), 1.0 / n)
    R = n_races
    cfgs = (N.McgpConfig * R)(*[prob.cfg] * R)
    drvs = (N.McgpDrivers * R)(*[prob.drv] * R)
    grids = (C.POINTER(C.c_double) * R)(*[S._dptr(g)] * R)
    seeds = (C.c_uint64 * R)(*range(R))
    pts = np.ascontiguousarray(kw.get('points', [[3, 2, 1][:n] + [0] * max(0, n - 3)] * R), np.int32)
    cb = np.ones(R, np.uint8)
    tm = np.ascontiguousarray([i % 2 for i in range(n)], np.int32)
    ip = None if init is None else np.ascontiguousarray(init, np.int32)
    bp, bw = np.ascontiguousarray(bonus, np.int32), np.ascontiguousarray(within, np.int32)
    i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    names = ('champ_hist', 'team_hist', 'gain_hist', 'race_hist', 'round_hist', 'contend_out', 'secure_out',
             'team_round_hist', 'team_contend_out', 'team_secure_out', 'bonus_hist', 'fastest_hist')
    bufs = {k: np.full(64 * 32 * 32, 0xDEAD, np.uint64) for k in names}
    ptr = lambda k: None if k in drop else bufs[k].ctypes.data_as(C.POINTER(C.c_uint64))
    rc = lib.mcgp_run_championship_bonus(R, cfgs, drvs, grids, n, n_sims, 0, seeds, i32(pts),
                                         cb.ctypes.data_as(C.POINTER(C.c_uint8)), i32(ip), None, i32(tm), min(n, 2), 0,
                                         *[ptr(k) for k in names[:10]], None if 'bonus_points' in drop else i32(bp),
                                         None if 'bonus_within' in drop else i32(bw), ptr('bonus_hist'), ptr('fastest_hist'))
    assert all((b == 0xDEAD).all() for b in bufs.values())          # no call here reaches a device: nothing is written
    return rc, lib.mcgp_last_error().decode()


ROUND_TRIO = ('round_hist', 'contend_out', 'secure_out')
TEAM_TRIO = ('team_round_hist', 'team_contend_out', 'team_secure_out')


def test_library_names_the_field_and_the_race():
    cases = [(dict(bonus=(1, -1)), 'bonus_points[1]'), (dict(bonus=(65536, 0)), 'bonus_points[0]'),
             (dict(bonus=(0, 2), within=(0, 0)), 'bonus_within[1]'), (dict(bonus=(1, 0), within=(4, 1)), 'bonus_within[0]'),
             (dict(drop=('bonus_points',)), 'bonus_points'), (dict(drop=('bonus_within',)), 'bonus_within'),
             (dict(bonus=(0, 1), within=(0, 1), deviates=1), 'bonus_points[1]'),
             (dict(init=[65535 - 6, 0, 0]), '65535'), (dict(drop=('round_hist',)), 'round_hist'),
             (dict(drop=ROUND_TRIO), 'team_round_hist'), (dict(drop=('champ_hist',)), 'NULL')]
    for kw, msg in cases:
        rc, err = _abi_call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    assert 'MCGP_DEVIATES_32' in _abi_call(bonus=(0, 1), within=(0, 1), deviates=1)[1]


def test_what_passes_the_checks_without_a_device():
    """Zero simulations: every check runs and no device is looked up."""
    assert _abi_call(n_sims=0)[0] == 0
    assert _abi_call(n_sims=0, init=[65535 - 6 - 1, 0, 0])[0] == 0                      # init + G = 65 535 exactly
    assert _abi_call(n_sims=0, bonus=(0, 0), within=(0, -5))[0] == 0                    # within is ignored without a bonus
    assert _abi_call(n_sims=0, bonus=(0, 0), deviates=1)[0] == 0                        # ... and so is the deviate width
    assert _abi_call(n_sims=0, drop=ROUND_TRIO + TEAM_TRIO)[0] == 0                     # no per-round work
    assert _abi_call(n_sims=0, drop=TEAM_TRIO)[0] == 0
    assert _abi_call(n_sims=0, drop=('bonus_hist', 'fastest_hist', 'race_hist'))[0] == 0
    assert _abi_call(n_sims=0, n=1, bonus=(5, 5), within=(1, 1), points=[[3], [3]])[0] == 0
