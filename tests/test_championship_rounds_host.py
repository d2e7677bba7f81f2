"""Championship by round, host side: the definitions restated (championship_rounds_ref) on seasons worked out by hand,
the identities every season's counts obey, ChampionshipResult's by-round properties on fabricated histograms, and the
argument checks of mcgp_run_championship_rounds, which need no device."""
import ctypes as C
import types

import numpy as np
import pytest

import championship_rounds_ref as RR
import oracle_py as O
from monte_carlo_gp_amd import ChampionshipResult, RaceConfig, cli, run_championship
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import simulation as S


def _o(*rows):
    return np.array(rows, np.uint8)


# ---------------------------------------------------------------- seasons by hand
def test_two_drivers_three_races_by_hand():
    """Table [2, 1], three Grands Prix, two simulations.  M = [4, 2, 0].
    sim 0: A wins all three.   after race 0: 2-1 (gap 1 <= 4: both in); race 1: 4-2 (gap 2 <= 2: both in, B can draw
           level); race 2: 6-3, A champion.
    sim 1: A, B, B.            race 0: 2-1; race 1: 3-3, one win each, one second each: full tie, lower index A leads,
           gap 0: both in; race 2: 4-5, B champion."""
    orders = [_o([0, 1], [0, 1]), _o([0, 1], [1, 0]), _o([0, 1], [1, 0])]
    M, B = RR.remaining([[2, 1]] * 3, 2, [0, 1], 2)
    assert list(M) == [4, 2, 0] and B.tolist() == [[4, 4], [2, 2], [0, 0]]
    out = RR.rounds(orders, [[2, 1]] * 3, [1, 1, 1], [0, 1], 2)
    assert out['round_hist'].tolist() == [[[2, 0], [0, 2]], [[2, 0], [0, 2]], [[1, 1], [1, 1]]]
    assert out['contend'].tolist() == [[2, 2], [2, 2], [1, 1]]
    assert out['secure'].tolist() == [[0, 0], [0, 0], [1, 1]]
    # singleton teams: the team tables are the drivers'
    for k in ('round_hist', 'contend', 'secure'):
        assert np.array_equal(out['team_' + k], out[k])


def test_three_drivers_with_a_head_start_by_hand():
    """Table [3, 2, 1], a Grand Prix and a sprint with table [1]; A carries in 2 points.  M = [1, 0].
    Teams: {A, C} and {B}.  B_r(team of 2) = [1, 0] (the sprint pays one place), B_r(team of 1) = [1, 0].
    sim 0: GP A B C -> A 5, B 2, C 1: gaps 3 and 4 > 1: A secure after race 0.   teams: 6 v 2, gap 4 > 1: secure.
    sim 1: GP B C A -> A 3, B 3, C 2: B leads on its win; A gap 0 in, C gap 1 <= 1 in: three in contention.
           teams: {A, C} 5, {B} 3: gap 2 > 1: team 0 secure.
    sim 2: GP C B A -> A 3, B 2, C 3: C leads on its win; A gap 0 in; B gap 1 in.
    Sprint (no countback): sim 0 B wins: A 5, B 3, C 1.  sim 1 A wins: A 4, B 3: A champion.  sim 2 B wins: A 3, B 3,
    C 3: all level, C has the only Grand Prix win: C champion, then B (a second place), then A."""
    gp, sprint = [3, 2, 1], [1]
    orders = [_o([0, 1, 2], [1, 2, 0], [2, 1, 0]), _o([1, 0, 2], [0, 1, 2], [1, 0, 2])]
    team = [0, 1, 0]
    M, B = RR.remaining([gp, sprint], 3, team, 2)
    assert list(M) == [1, 0] and B.tolist() == [[1, 1], [0, 0]]
    out = RR.rounds(orders, [gp, sprint], [1, 0], team, 2, init_points=[2, 0, 0])
    assert out['round_hist'][0].tolist() == [[1, 2, 0], [1, 1, 1], [1, 0, 2]]
    assert out['contend'].tolist() == [[3, 2, 2], [2, 0, 1]]
    assert out['secure'].tolist() == [[1, 0, 0], [2, 0, 1]]
    assert out['round_hist'][1].tolist() == [[2, 0, 1], [0, 3, 0], [1, 0, 2]]
    # teams after the Grand Prix: 6 v 2, 5 v 3, 6 v 2; after the sprint: 6 v 3, 6 v 3, 6 v 3
    assert out['team_round_hist'].tolist() == [[[3, 0], [0, 3]]] * 2
    assert out['team_contend'].tolist() == [[3, 0], [3, 0]] and out['team_secure'].tolist() == [[3, 0], [3, 0]]


def test_the_bound_is_inclusive_and_the_last_race_is_not_a_bound():
    """One simulation, table [3, 2, 1].  After race 0 of two: 3-2-1, M = 3: the third driver, 2 behind, and a fourth
    with nothing, exactly 3 behind, are in.  After the last race: A 5, B 5 (one win each, one second each: the index
    decides): only A is in contention although B is level on points, and A is secure."""
    orders = [_o([0, 1, 2, 3]), _o([1, 0, 2, 3])]
    out = RR.rounds(orders, [[3, 2, 1]] * 2, [1, 1], [0, 0, 1, 1], 2)
    assert out['contend'].tolist() == [[1, 1, 1, 1], [1, 0, 0, 0]]
    assert out['secure'].tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]]
    # one point less to be had: the fourth driver (3 behind, M = 2) is out, the third (2 behind) exactly on the bound
    out = RR.rounds(orders, [[3, 2, 1], [2, 1]], [1, 1], [0, 0, 1, 1], 2)
    assert out['contend'][0].tolist() == [1, 1, 1, 0]
    # teams: 5 v 1 after race 0, B(team of two) = 2 + 1 = 3 < 4: team 0 secure; with [3, 2, 1] to come B = 5: both in
    assert out['team_secure'][0].tolist() == [1, 0]
    out = RR.rounds(orders, [[3, 2, 1]] * 2, [1, 1], [0, 0, 1, 1], 2)
    assert out['team_contend'][0].tolist() == [1, 1] and out['team_secure'][0].tolist() == [0, 0]


# ---------------------------------------------------------------- identities
@pytest.mark.parametrize('seed', range(6))
def test_identities_on_random_seasons(seed):
    import championship_ref as CR
    rng = np.random.default_rng(seed)
    n, R, sims = int(rng.integers(2, 9)), int(rng.integers(1, 6)), 300
    T = int(rng.integers(1, n + 1))
    team = rng.integers(0, T, n)
    team[rng.permutation(n)[:T]] = np.arange(T)
    tables = [sorted((int(x) for x in rng.integers(0, 6, int(rng.integers(1, n + 1)))), reverse=True) for _ in range(R)]
    cb = [int(x) for x in rng.integers(0, 2, R)]
    ip = rng.integers(0, 5, n)
    orders = [rng.permuted(np.tile(np.arange(n, dtype=np.uint8), (sims, 1)), axis=1) for _ in range(R)]
    out = RR.rounds(orders, tables, cb, team, T, ip)
    champ, teams, _, _ = CR.championship(orders, tables, cb, team, T, init_points=ip)
    RR.assert_identities(out, sims, champ, teams)
    # whoever is secure at r is the final champion
    per = RR.per_simulation(orders, tables, cb, team, T, ip)
    for s in per:
        assert not (s['secure'] & ~per[-1]['secure']).any() and not (s['tsecure'] & ~per[-1]['tsecure']).any()


# ---------------------------------------------------------------- the Python properties
def _result(**kw):
    base = dict(drivers=['A', 'B', 'C'], teams=['X', 'Y'], n_simulations=10, champ_hist=np.zeros((3, 3), np.int64),
                team_hist=np.zeros((2, 2), np.int64), gain_hist=np.zeros((3, 1), np.int64), initial_points={})
    base.update(kw)
    return ChampionshipResult(**base)


def test_by_round_properties_from_fabricated_histograms():
    round_hist = np.array([[[6, 4, 0], [4, 5, 1], [0, 1, 9]], [[7, 3, 0], [3, 7, 0], [0, 0, 10]]])
    contend = np.array([[10, 8, 1], [7, 3, 0]])
    secure = np.array([[2, 0, 0], [7, 3, 0]])
    t_round = np.array([[[10, 0], [0, 10]], [[9, 1], [1, 9]]])
    t_contend, t_secure = np.array([[10, 5], [9, 1]]), np.array([[5, 0], [9, 1]])
    res = _result(round_hist=round_hist, contend=contend, secure=secure, team_round_hist=t_round, team_contend=t_contend,
                  team_secure=t_secure)
    assert res.leader_probabilities_by_round == [{'A': 0.6, 'B': 0.4, 'C': 0.0}, {'A': 0.7, 'B': 0.3, 'C': 0.0}]
    assert res.contention_probabilities_by_round == [{'A': 1.0, 'B': 0.8, 'C': 0.1}, {'A': 0.7, 'B': 0.3, 'C': 0.0}]
    assert res.decided_by_round == [0.2, 1.0]
    assert res.clinch_round_probabilities == {'A': {0: 0.2, 1: 0.5}, 'B': {1: 0.3}, 'C': {}}
    assert res.constructor_leader_probabilities_by_round == [{'X': 1.0, 'Y': 0.0}, {'X': 0.9, 'Y': 0.1}]
    assert res.constructor_contention_probabilities_by_round == [{'X': 1.0, 'Y': 0.5}, {'X': 0.9, 'Y': 0.1}]
    assert res.constructor_decided_by_round == [0.5, 1.0]
    assert res.constructor_clinch_round_probabilities == {'X': {0: 0.5, 1: 0.4}, 'Y': {1: 0.1}}


def test_by_round_properties_need_by_round():
    res = _result()
    assert res.round_hist is None and res.secure is None and res.team_contend is None
    for name in ('leader_probabilities_by_round', 'contention_probabilities_by_round', 'decided_by_round',
                 'clinch_round_probabilities', 'constructor_decided_by_round'):
        with pytest.raises(ValueError, match='by_round=True'):
            getattr(res, name)


def _race(name, **kw):
    case = O.load_case(name)
    return dict(config=RaceConfig(**case['config']), grid_probs=case['grid_probs'], base_pace=case['base_pace'],
                tire_deg=case['tire_deg'], driver_variance=case['driver_variance'],
                driver_dnf_rates=case['driver_dnf_rates'], track_condition=case['track_condition'], **kw)


def test_python_layer_shapes_without_running():
    """n_simulations = 0 goes through every argument check of the new entry point and returns before any device."""
    races = [_race('S60', seed=5), _race('S78', seed=6, countback=False, points=[8, 7, 6])]
    res = run_championship(races, 0, by_round=True)
    T = len(res.teams)
    assert res.round_hist.shape == (2, 20, 20) and res.contend.shape == (2, 20) and res.secure.shape == (2, 20)
    assert res.team_round_hist.shape == (2, T, T) and res.team_contend.shape == (2, T) and res.team_secure.shape == (2, T)
    assert not res.round_hist.any() and res.round_hist.dtype == np.int64
    plain = run_championship(races, 0)
    assert plain.round_hist is None and plain.team_secure is None


def test_a_library_without_the_symbol_is_a_clear_error(monkeypatch):
    real = N.lib()
    old = types.SimpleNamespace(**{k: getattr(real, k) for k in N.EXPORTS if k != 'mcgp_run_championship_rounds'})
    monkeypatch.setattr(S.N, 'lib', lambda: old)
    with pytest.raises(N.McgpError, match='mcgp_run_championship_rounds'):
        run_championship([_race('S60', seed=5)], 0, by_round=True)
    assert run_championship([_race('S60', seed=5)], 0).round_hist is None        # the plain call does not need it


def test_cli_takes_by_round():
    ap_args = ['championship', '--season', '2024', '--from-round', '0', '--simulations', '10', '--by-round']
    with pytest.raises(ValueError, match='from-round'):             # parsed; the round check comes before any device
        cli.main(ap_args)


# ---------------------------------------------------------------- the library's argument checks
def _abi_call(drop=(), n=3, n_teams=2, n_races=2, n_sims=100, **kw):
    lib = N.lib()
    case = O.load_case('S60')
    drivers = [f'D{i:02d}' for i in range(max(n, 1))]
    prob = S._Problem(RaceConfig(**case['config']), drivers, {}, {}, {}, None, 'dry', S.DEFAULT_SET_POP)
    g = np.full((max(n, 1), max(n, 1)), 1.0 / max(n, 1))
    R = max(n_races, 1)
    cfgs = (N.McgpConfig * R)(*[prob.cfg] * R)
    drvs = (N.McgpDrivers * R)(*[prob.drv] * R)
    grids = (C.POINTER(C.c_double) * R)(*[S._dptr(g)] * R)
    seeds = (C.c_uint64 * R)(*range(R))
    pts = np.ascontiguousarray(kw.get('points', np.zeros((R, max(n, 1)))), np.int32)
    cb = np.ones(R, np.uint8)
    tm = np.ascontiguousarray(kw.get('team', [i % max(n_teams, 1) for i in range(max(n, 1))]), np.int32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    names = ('champ_hist', 'team_hist', 'gain_hist', 'race_hist', 'round_hist', 'contend_out', 'secure_out',
             'team_round_hist', 'team_contend_out', 'team_secure_out')
    bufs = {k: np.full(64 * 32 * 32, 0xDEAD, np.uint64) for k in names}
    ptr = lambda k: None if k in drop else bufs[k].ctypes.data_as(C.POINTER(C.c_uint64))
    rc = lib.mcgp_run_championship_rounds(n_races, cfgs, drvs, grids, n, n_sims, 0, seeds, i32(pts),
                                          cb.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, i32(tm), n_teams, 0,
                                          *[ptr(k) for k in names])
    assert all((b == 0xDEAD).all() for b in bufs.values()) or rc == 0       # a call that fails writes nothing
    return rc, lib.mcgp_last_error().decode()


def test_library_names_the_missing_round_argument():
    for k in ('round_hist', 'contend_out', 'secure_out'):
        rc, err = _abi_call(drop=(k,))
        assert rc == -1 and k in err and 'NULL' in err, (k, rc, err)
    trio = ('team_round_hist', 'team_contend_out', 'team_secure_out')
    for drop in [trio[:1], trio[1:2], trio[2:], trio[:2], trio[1:], (trio[0], trio[2])]:
        rc, err = _abi_call(drop=drop)
        assert rc == -1 and all(k in err for k in trio), (drop, rc, err)
    # all three NULL, or all given: the checks pass (zero simulations: no device is looked up)
    assert _abi_call(drop=trio, n_sims=0)[0] == 0
    assert _abi_call(n_sims=0)[0] == 0
    assert _abi_call(drop=('race_hist',), n_sims=0)[0] == 0


def test_the_base_calls_limits_hold_before_any_device_lookup():
    cases = [(dict(n_races=65), 'n_races must be in [1, 64]'), (dict(n=33), 'n must be in [1, 32]'),
             (dict(n_teams=0), 'n_teams must be in [1, n]'), (dict(n_teams=4), 'n_teams must be in [1, n]'),
             (dict(team=[0, 2, 1]), 'team index'), (dict(points=[[25, -1, 0], [0, 0, 0]]), 'negative'),
             (dict(drop=('champ_hist',)), 'NULL')]
    for kw, msg in cases:
        rc, err = _abi_call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
