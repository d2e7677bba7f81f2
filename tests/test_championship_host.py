"""Championship simulation, host side: the semantics restated (championship_ref) on hand-built orders, the Python and
C-ABI argument checks (no device needed), and the CLI's race list against the backtest's."""
import ctypes as C

import numpy as np
import pytest

import championship_cases as CC
import championship_ref as CR
import oracle_py as O
from monte_carlo_gp_amd import RaceConfig, cli, run_championship
from monte_carlo_gp_amd import _native as N

F1 = [25, 18, 15, 12, 10, 8, 6, 4, 2, 1]


def _o(*rows):
    return np.array(rows, np.uint8)


def _ranked(orders_list, points_list, countback, **kw):
    pts, cnt = CR.standings(orders_list, points_list, countback, kw.get('init_points'), kw.get('init_counts'))
    return pts, cnt, CR.rank(pts, cnt)


def test_equal_points_decided_by_wins():
    # race 1: A (0) wins, B (1) 2nd, C 3rd; race 2: B wins, C 2nd, A 3rd
    table = [10, 10, 1]
    pts, cnt, pos = _ranked([_o([0, 1, 2]), _o([1, 2, 0])], [table, table], [1, 1])
    assert list(pts[0]) == [11, 20, 11]
    assert list(pos[0]) == [1, 0, 2]                 # B leads on points; A and C tie at 11, A has a win
    # one win and one P3 each, equal points: the key is equal, the lower index ranks higher
    pts, cnt, pos = _ranked([_o([0, 2, 1]), _o([1, 2, 0])], [[10, 5, 5], [10, 5, 5]], [1, 1])
    assert list(pts[0]) == [15, 15, 10] and list(pos[0]) == [0, 1, 2]


def test_then_by_second_places():
    # A: P1, P2, P2; B: P3, P1, P3 -- equal points under a table that pays P2 and P3 alike, one win each
    table = [10, 4, 4]
    orders = [_o([0, 2, 1]), _o([1, 0, 2]), _o([2, 0, 1])]
    pts, cnt, pos = _ranked(orders, [table] * 3, [1, 1, 1])
    assert pts[0, 0] == pts[0, 1] == 18
    assert cnt[0, 0, 0] == cnt[0, 1, 0] == 1 and cnt[0, 0, 1] == 2 and cnt[0, 1, 1] == 0
    assert pos[0, 0] < pos[0, 1]                     # A (two P2s) ahead of B (no P2)
    orders = [_o([0, 1, 2]), _o([1, 0, 2]), _o([2, 1, 0])]
    pts, cnt, pos = _ranked(orders, [table] * 3, [1, 1, 1])
    assert pts[0, 0] == pts[0, 1] and cnt[0, 1, 1] > cnt[0, 0, 1] and pos[0, 1] < pos[0, 0]


def test_a_sprint_scores_but_does_not_count_back():
    # GP: A wins, B 2nd. Sprint: B wins, A 2nd. Table pays the same total; tie-break counts the GP only
    gp, sprint = [10, 5], [5, 10]
    pts, cnt, pos = _ranked([_o([0, 1]), _o([1, 0])], [gp, sprint], [1, 0])
    assert list(pts[0]) == [20, 10]
    pts, cnt, pos = _ranked([_o([1, 0]), _o([1, 0])], [[10, 5], [5, 10]], [1, 0])
    # B: GP win 10 + sprint P1 5 = 15; A: GP P2 5 + sprint P2 10 = 15: B has the only countback win
    assert list(pts[0]) == [15, 15] and cnt[0].tolist() == [[0, 1], [1, 0]] and list(pos[0]) == [1, 0]
    # a sprint win does not break a tie: B won the Grand Prix, A the sprint; both on 8 points, A with a GP 2nd place.
    # Counted, the sprint win would level the wins and the index would put A ahead.
    pts, cnt, pos = _ranked([_o([1, 0]), _o([0, 1])], [[5, 5], [3, 3]], [1, 0])
    assert list(pts[0]) == [8, 8] and list(pos[0]) == [1, 0]
    pts, cnt, pos = _ranked([_o([1, 0]), _o([0, 1])], [[5, 5], [3, 3]], [1, 1])
    assert list(pos[0]) == [0, 1]


def test_full_tie_goes_to_the_lower_index():
    pts, cnt, pos = _ranked([_o([2, 1, 0])], [[0, 0, 0]], [0])
    assert list(pos[0]) == [0, 1, 2]
    pts, cnt, pos = _ranked([_o([2, 1, 0])], [[0, 0, 0]], [1])
    assert list(pos[0]) == [2, 1, 0]                 # counts decide before the index


def test_carried_in_standings():
    init_p = [100, 110, 0]
    init_c = [[3, 0, 0], [0, 5, 0], [0, 0, 0]]
    pts, cnt, pos = _ranked([_o([0, 1, 2])], [[10, 0, 0]], [1], init_points=init_p, init_counts=init_c)
    assert list(pts[0]) == [110, 110, 0] and list(cnt[0, 0]) == [4, 0, 0] and list(pos[0]) == [0, 1, 2]
    champ, teams, gain, races = CR.championship([_o([0, 1, 2])], [[10, 0, 0]], [1], [0, 1, 2], 3,
                                                init_points=init_p, init_counts=init_c)
    assert gain.tolist() == [[0] * 10 + [1], [1] + [0] * 10, [1] + [0] * 10]


def test_constructors_are_sums_of_their_drivers():
    # teams: {0, 3} and {1, 2}
    team = [0, 1, 1, 0]
    orders = [_o([0, 1, 2, 3]), _o([1, 0, 3, 2])]
    champ, teams, gain, races = CR.championship(orders, [F1, F1], [1, 1], team, 2)
    pts, cnt = CR.standings(orders, [F1, F1], [1, 1])
    tp, tc = CR.team_standings(pts, cnt, team, 2)
    assert tp[0].tolist() == [25 + 12 + 18 + 15, 18 + 15 + 25 + 12]
    assert tc[0].tolist() == [[1, 1, 1, 1], [1, 1, 1, 1]]
    assert teams.tolist() == [[1, 0], [0, 1]]        # equal on every field: the lower team index wins
    champ, teams, gain, races = CR.championship([_o([1, 0, 3, 2])] * 2, [F1, F1], [1, 1], team, 2)
    assert teams.tolist() == [[0, 1], [1, 0]]


def test_points_table_shorter_than_the_field():
    orders = [_o([4, 3, 2, 1, 0])]
    pts, cnt, pos = _ranked(orders, [[3, 1]], [1])
    assert list(pts[0]) == [0, 0, 0, 1, 3]
    assert list(pos[0]) == [4, 3, 2, 1, 0]           # the non-scorers are split by their countback places
    champ, teams, gain, races = CR.championship(orders, [[3, 1]], [1], [0] * 5, 1)
    assert gain.shape == (5, 4) and races[0].tolist() == np.fliplr(np.eye(5, dtype=np.int64)).tolist()


def test_one_driver():
    champ, teams, gain, races = CR.championship([_o([0], [0])] * 3, [[25], [25], [8]], [1, 1, 0], [0], 1)
    assert champ.tolist() == [[2]] and teams.tolist() == [[2]] and gain.tolist() == [[0] * 58 + [2]]


def test_grouped_ranking_equals_the_per_simulation_sort():
    rng = np.random.default_rng(3)
    for n, races in ((1, 3), (5, 4), (12, 2), (20, 6)):
        orders = [np.array([rng.permutation(n) for _ in range(700)], np.uint8) for _ in range(races)]
        tables = [F1[:rng.integers(1, 11)] for _ in range(races)]
        cb = [int(x) for x in rng.integers(0, 2, races)]
        pts, cnt = CR.standings(orders, tables, cb, rng.integers(0, 5, n), rng.integers(0, 2, (n, n)))
        assert np.array_equal(CR.rank(pts, cnt), CR.rank_grouped(pts, cnt, block=256))


# ---------------------------------------------------------------- the Python and C-ABI layers, without a device
def _race(case_name='S60', **kw):
    c = O.load_case(case_name)
    return dict(config=RaceConfig(**c['config']), grid_probs=c['grid_probs'], base_pace=c['base_pace'],
                tire_deg=c['tire_deg'], driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'],
                track_condition=c['track_condition'], **kw)


def test_python_layer_checks_its_arguments():
    a, b = _race('S60'), _race('N10')
    with pytest.raises(ValueError, match='drivers differ'):
        run_championship([a, b], 10)
    drivers = list(a['grid_probs'])
    # 24 countback races + 8 earlier wins = 32 > 31
    with pytest.raises(ValueError, match='31'):
        run_championship([_race('S60', seed=i) for i in range(24)], 10,
                         standings={drivers[0]: {'points': 100, 'finishes': [8]}})
    with pytest.raises(ValueError, match='65535'):
        run_championship([_race('S60', seed=1)], 10, standings={drivers[0]: 65530})
    with pytest.raises(ValueError, match='not in the field'):
        run_championship([_race('S60', seed=1)], 10, standings={'NOBODY': 3})
    with pytest.raises(ValueError, match='at most 64'):
        run_championship([_race('S60', seed=1)] * 65, 10)


def test_python_layer_resolves_drivers_teams_and_standings_without_running():
    """n_simulations = 0 goes through every argument check of the library and returns before any device is used."""
    races = [_race('S60', seed=5), _race('S78', countback=False, points=[8, 7, 6, 5, 4, 3, 2, 1])]
    drivers = list(races[0]['grid_probs'])
    res = run_championship(races, 0, standings={drivers[1]: 7, drivers[2]: {'points': 3, 'finishes': [1]}})
    teams = []
    for d in drivers:
        t = races[0]['config'].driver_teams.get(d, 'Unknown')
        if t not in teams:
            teams.append(t)
    assert res.drivers == drivers and res.teams == teams
    assert res.champ_hist.shape == (20, 20) and res.team_hist.shape == (len(teams), len(teams))
    assert res.gain_hist.shape == (20, 25 + 8 + 1) and not res.champ_hist.any()
    assert res.initial_points[drivers[1]] == 7 and res.initial_points[drivers[2]] == 3


def _abi_call(n=3, n_races=1, n_teams=1, team=None, points=None, countback=None, init_points=None, init_counts=None,
              n_sims=100):
    lib = N.lib()
    case = O.load_case('S60')
    from monte_carlo_gp_amd.simulation import _Problem, DEFAULT_SET_POP, _dptr
    drivers = [f'D{i:02d}' for i in range(max(n, 1))]       # (arrays as long as the n the call names)
    prob = _Problem(RaceConfig(**case['config']), drivers, {}, {}, {}, None, 'dry', DEFAULT_SET_POP)
    g = np.full((max(n, 1), max(n, 1)), 1.0 / max(n, 1))
    R = max(n_races, 1)
    cfgs = (N.McgpConfig * R)(*[prob.cfg] * R)
    drvs = (N.McgpDrivers * R)(*[prob.drv] * R)
    grids = (C.POINTER(C.c_double) * R)(*[_dptr(g)] * R)
    seeds = (C.c_uint64 * R)(*range(R))
    pts = np.zeros((R, max(n, 1)), np.int32) if points is None else np.ascontiguousarray(points, np.int32)
    cb = np.ones(R, np.uint8) if countback is None else np.ascontiguousarray(countback, np.uint8)
    tm = np.zeros(max(n, 1), np.int32) if team is None else np.ascontiguousarray(team, np.int32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
    ip = None if init_points is None else np.ascontiguousarray(init_points, np.int32)
    ic = None if init_counts is None else np.ascontiguousarray(init_counts, np.int32)
    h = np.zeros(64 * 64 * 64, np.uint64)
    hp = h.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = lib.mcgp_run_championship(n_races, cfgs, drvs, grids, n, n_sims, 0, seeds, i32(pts),
                                   cb.ctypes.data_as(C.POINTER(C.c_uint8)), i32(ip), i32(ic), i32(tm), n_teams, 0,
                                   hp, hp, hp, None)
    return rc, lib.mcgp_last_error().decode()


def test_library_rejects_out_of_envelope_calls_before_any_device_lookup():
    """MCGP_E_BAD_ARG, naming the limit, on a machine with or without a GPU (the checks come first)."""
    cases = [
        (dict(n_races=65), 'n_races must be in [1, 64]'),
        (dict(n_races=0), 'n_races must be in [1, 64]'),
        (dict(n=33), 'n must be in [1, 32]'),
        (dict(n=0), 'n must be in [1, 32]'),
        (dict(n_teams=4), 'n_teams must be in [1, n]'),
        (dict(n_teams=2, team=[0, 2, 1]), 'team index'),
        (dict(countback=[2]), 'countback'),
        (dict(points=[[25, -1, 0]]), 'negative'),
        (dict(init_points=[65000, 0, 0], points=[[600, 0, 0]]), '65535'),
        (dict(init_counts=[[31, 0, 0], [0, 0, 0], [0, 0, 0]]), '31'),
        (dict(n_races=32, countback=[1] * 32), '31'),
    ]
    for kw, msg in cases:
        rc, err = _abi_call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    # at the limits exactly, the checks pass (a call of zero simulations then returns without a device)
    rc, err = _abi_call(init_counts=[[0, 0, 30], [0, 0, 0], [0, 0, 0]], init_points=[65535 - 600, 0, 0],
                        points=[[600, 0, 0]], n_sims=0)
    assert rc == 0, err
    rc, err = _abi_call(n=32, n_teams=1, n_races=31, countback=[1] * 31, n_sims=0)
    assert rc == 0, err


# ---------------------------------------------------------------- the CLI's races
def test_cli_races_are_the_backtest_races_with_their_seeds():
    full = cli.backtest_jobs([2024], 7)
    jobs = cli.championship_jobs(2024, 7, from_round=21)
    assert len(jobs) == 4 and [j[2] for j in jobs] == [j[2] for j in full[20:]]
    assert [j[1]['race'] for j in jobs] == [j[1]['race'] for j in full[20:]]
    assert cli.championship_jobs(2024, 7) == full
    with pytest.raises(ValueError):
        cli.championship_jobs(2024, 7, from_round=25)
    from monte_carlo_gp_amd.predictor import F1Predictor
    races = cli.championship_races(jobs)
    for (season, entry, seed, fixture), race in zip(jobs, races):
        inp = F1Predictor().simulator_inputs(fixture, entry['race'])
        assert race['seed'] == seed and race['grid_probs'] == inp['grid_probs']
        assert race['base_pace'] == inp['base_pace'] and race['config'] == inp['config']
        assert 'points' not in race and 'countback' not in race       # every round a Grand Prix, default table
    # the drivers come in one order for every race
    assert all(list(r['grid_probs']) == list(races[0]['grid_probs']) for r in races)


def test_cli_championship_parses_and_checks_the_round(capsys):
    with pytest.raises(ValueError, match='from-round'):
        cli.main(['championship', '--season', '2024', '--from-round', '0', '--simulations', '10'])


# ---------------------------------------------------------------- the seasons of championship_cases reach their edges
# (the half of tests/test_gpu_championship_limits.py that needs no device: the CPU oracle and championship_ref alone)
def test_decision_depth_names_the_first_field_that_differs():
    # three entrants: 0 and 1 differ in points; 1 and 2 tie on points and P1s and differ in P2s
    pts = np.array([[9, 5, 5]])
    cnt = np.array([[[0, 0, 1], [1, 1, 0], [1, 0, 0]]])
    assert CR.decision_depth(pts, cnt).tolist() == [1, 0, 1, 0, 0]
    # a full tie is decided by the index: the last cell
    assert CR.decision_depth(np.array([[4, 4]]), np.zeros((1, 2, 2), np.int64)).tolist() == [0, 0, 0, 1]


def test_lexsort_ranking_equals_the_per_simulation_sort():
    rng = np.random.default_rng(4)
    for n, races in ((1, 3), (5, 4), (12, 2), (23, 3)):
        orders = [np.array([rng.permutation(n) for _ in range(400)], np.uint8) for _ in range(races)]
        pts, cnt = CR.standings(orders, [CC.SHORT] * races, [1] * races, rng.integers(0, 3, n), rng.integers(0, 2, (n, n)))
        assert np.array_equal(CR.rank(pts, cnt), CR.rank_lexsort(pts, cnt))


@pytest.mark.parametrize('n', list(range(1, 33)))
def test_tie_rich_seasons_reach_the_word_boundaries(n):
    season = CC.tie_rich(n)
    pts, cnt, _, _ = CC.reference_standings(season, CC.oracle_orders(season))
    CC.assert_tie_rich_edges(n, pts, cnt, CC.standings_arrays(season)[0])


def test_the_layout_restated():
    assert [n for n in range(1, 33) if CC.points_low_bits(n)] == list(CC.POINTS_STRADDLE)
    assert [CC.points_low_bits(n) for n in CC.POINTS_STRADDLE] == [14, 9, 4, 13, 8, 3]
    for n in CC.POINTS_STRADDLE:            # 3 short of a full lower piece
        p, low = CC.tie_rich_points(n), CC.points_low_bits(n)
        assert (p + 2) >> low == p >> low and (p + 3) >> low == (p >> low) + 1


@pytest.mark.parametrize('n', [20, 32])
def test_procession_seasons_reach_31_wins_and_65535_points(n):
    season = CC.procession(n)
    pts, cnt, _, _ = CC.reference_standings(season, CC.oracle_orders(season))
    CC.assert_procession_edges(pts, cnt)


def test_long_calendar_season():
    season = CC.long_calendar()
    assert len(season['plan']) == 64 and sum(p[4] for p in season['plan']) == 31
    pts, cnt, _, _ = CC.reference_standings(season, CC.oracle_orders(season))
    assert cnt.sum(axis=2).max() == 31 and len(np.unique(pts)) > 100


@pytest.mark.parametrize('name', list(CC.team_seasons()))
def test_team_seasons_reach_their_layouts(name):
    season, words = CC.team_seasons()[name]
    _, _, tp, tc = CC.reference_standings(season, CC.oracle_orders(season))
    CC.assert_team_edges(name, season, tp, tc)
    assert sorted(set(CC.team_seasons_words().values())) == [1, 3, 4, 5, 6]


@pytest.mark.parametrize('name', list(CC.gain_seasons()))
def test_gain_seasons_take_their_path_and_reach_both_ends(name):
    season, path = CC.gain_seasons()[name]
    assert CC.gain_path(season, 64 * 1024) == path and CC.gain_path(season, 160 * 1024) == path
    pts, _, _, _ = CC.reference_standings(season, CC.oracle_orders(season))
    gain = pts - CC.standings_arrays(season)[0][None, :]
    G = sum(max(p[3]) for p in season['plan'])
    assert (gain == 0).sum() >= 50 and (gain == G).sum() >= 50


def test_uneven_teams_season_tells_the_bounds_apart():
    e = CC.assert_uneven_team_edges(CC.reference_rounds(CC.uneven_teams()))
    assert list(e.values()) == [151, 899, 916, 262], e


@pytest.mark.parametrize('n', [20, 32])
def test_procession_duel_sits_on_the_bound_in_row_20(n):
    assert CC.assert_duel_edges(CC.reference_rounds(CC.procession_duel(n))) == 200


def test_long_calendar_by_round():
    season = CC.long_calendar()
    CC.assert_long_calendar_rounds(CC.reference_rounds(season), season['n_sims'])


@pytest.mark.parametrize('name', list(CC.team_seasons()))
def test_team_seasons_need_the_whole_points_field_by_round(name):
    season, _ = CC.team_seasons()[name]
    pbits = CC.assert_team_round_edges(name, season, CC.reference_rounds(season))
    assert pbits == {'six_words': 21, 'one_team_32': 21, 'one_team_20': 20, 'quads_27': 18}.get(name, 16 if 'singletons' in name else 17)


def test_team_points_borrow_season_straddles_bit_16():
    season = CC.team_points_borrow()
    assert CC.team_layout(season) == (6, 3) and CC.team_points_bits(season) == 17
    assert CC.assert_team_borrow_edges(season, CC.reference_rounds(season)) == 882 + 3603 + 3905 + 637


def test_round_lds_restated():
    """DESIGN 3.7.1's two figures: 32 drivers in 32 teams with six-word team keys; 20 drivers in 10 teams of two."""
    assert CC.round_lds_bytes(32, 32, 6) == 157696 and CC.round_lds_bytes(20, 10, 2) == 34496
    assert CC.round_lds_bytes(3, 0, 1) == (3 * 64 * 8 + 6 * 64 * 4 + (9 + 6) * 4 + 15) // 16 * 16


def test_tail_seasons_leave_one_two_and_three_bytes():
    for n in (9, 23, 31):
        assert sorted(CC.tail_bytes(n, k) for k in (501, 502, 503)) == [1, 2, 3]
