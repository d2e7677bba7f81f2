"""Championship simulation on the device (mcgp_run_championship) against championship_ref fed with the CPU oracle's
finishing orders: every histogram equal, count for count."""
import json

import numpy as np
import pytest

import championship_ref as CR
import oracle_py as O
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, cli, run_championship

pytestmark = pytest.mark.gpu

F1 = [25, 18, 15, 12, 10, 8, 6, 4, 2, 1]
SPRINT = [8, 7, 6, 5, 4, 3, 2, 1]


def _race(case, seed, **kw):
    return dict(config=RaceConfig(**case['config']), grid_probs=case['grid_probs'], base_pace=case['base_pace'],
                tire_deg=case['tire_deg'], driver_variance=case['driver_variance'],
                driver_dnf_rates=case['driver_dnf_rates'], track_condition=case['track_condition'], seed=seed, **kw)


def _teams(case, drivers):
    names = []
    for d in drivers:
        t = case['config']['driver_teams'].get(d, 'Unknown')
        if t not in names:
            names.append(t)
    return names, [names.index(case['config']['driver_teams'].get(d, 'Unknown')) for d in drivers]


def _standings_arrays(standings, drivers):
    n = len(drivers)
    p, c = np.zeros(n, np.int64), np.zeros((n, n), np.int64)
    for d, v in standings.items():
        i = drivers.index(d)
        if isinstance(v, dict):
            p[i] = v['points']
            c[i, :len(v['finishes'])] = v['finishes']
        else:
            p[i] = v
    return p, c


def _check(res, cases, plan, n_sims, sim_offset, standings, grouped=False, orders=None):
    """plan: [(case name or case dict, seed, deviates, points table, countback)].  orders: the oracle's orders of the
    plan's races, when the caller has them already."""
    drivers = res.drivers
    orders = [] if orders is None else orders
    for case, seed, dev, _, _ in plan[len(orders):]:
        case = cases[case] if isinstance(case, str) else case
        assert list(case['grid_probs']) == drivers
        rng = O.RNG_PHILOX53 if dev == 53 else O.RNG_PHILOX
        orders.append(O.Problem(case).run(n_sims, rng=rng, seed=seed, sim_offset=sim_offset, want_orders=True)['orders'])
    first = cases[plan[0][0]] if isinstance(plan[0][0], str) else plan[0][0]
    names, team = _teams(first, drivers)
    assert res.teams == names
    ip, ic = _standings_arrays(standings, drivers)
    champ, teams, gain, races = CR.championship(orders, [p[3] for p in plan], [int(p[4]) for p in plan], team, len(names),
                                                init_points=ip, init_counts=ic, grouped=grouped)
    assert np.array_equal(res.champ_hist, champ)
    assert np.array_equal(res.team_hist, teams)
    assert np.array_equal(res.gain_hist, gain)
    for r, h in enumerate(res.race_histograms):
        assert np.array_equal(h, races[r]), r
    return champ


def test_six_race_season_equals_the_oracle(require_gpu):
    """The six golden cases of one 20-driver field, distinct seeds, one at the reference's deviate width, one a sprint,
    carried-in standings, a non-zero sim_offset."""
    names = ['S60', 'S78', 'S50', 'EVT', 'DMP', 'WET']
    cases = {k: O.load_case(k) for k in names}
    plan = [('S60', 101, 32, F1, True), ('S78', 202, 32, F1, True), ('S50', 303, 32, F1, True),
            ('EVT', 404, 53, F1, True), ('DMP', 505, 32, SPRINT, False), ('WET', 606, 32, F1, True)]
    drivers = list(cases['S60']['grid_probs'])
    standings = {drivers[0]: {'points': 51, 'finishes': [2, 0, 0, 1]}, drivers[2]: {'points': 51, 'finishes': [2, 0, 1]},
                 drivers[4]: 33, drivers[6]: {'points': 18, 'finishes': [0, 1]}, drivers[19]: 1}
    races = [_race(cases[c], seed, deviates=dev, points=pts, countback=cb) for c, seed, dev, pts, cb in plan]
    n_sims, offset = 3000, 98765
    res = run_championship(races, n_sims, standings=standings, sim_offset=offset, set_pop=O.load_cases()['set_pop'],
                           return_race_histograms=True)
    champ = _check(res, cases, plan, n_sims, offset, standings)
    assert (champ.sum(axis=0) == n_sims).all() and (champ.sum(axis=1) == n_sims).all()
    assert abs(sum(res.title_probabilities.values()) - 1.0) < 1e-12
    assert abs(sum(res.constructor_title_probabilities.values()) - 1.0) < 1e-12
    exp = res.expected_points
    assert exp[drivers[0]] > 51 and all(v >= 0 for v in exp.values())


def _field(n):
    """An n-car field with S60's parameters, 25 laps and an all-zero grid column (the builder of test_gpu_parity)."""
    rng = np.random.default_rng(n)
    drivers = [f'D{i:02d}' for i in range(n)]
    base = O.load_case('S60')
    case = dict(base)
    case['config'] = dict(base['config'], total_laps=25,
                          driver_teams={d: list(base['config']['dnf_rates'])[i % 10] for i, d in enumerate(drivers)})
    g = rng.random((n, n))
    g[:, n // 2] = 0.0
    case['grid_probs'] = {d: [float(x) for x in g[i]] for i, d in enumerate(drivers)}
    case['base_pace'] = {d: 90.0 + 0.2 * i for i, d in enumerate(drivers)}
    case['tire_deg'] = {d: 0.05 for d in drivers}
    case['driver_variance'] = {d: 0.2 for d in drivers}
    case['driver_dnf_rates'] = {d: 0.01 for d in drivers}
    return case


@pytest.mark.parametrize('n', [1, 2, 9, 22, 23, 32])
def test_field_sizes_equal_the_oracle(require_gpu, n):
    """Both key widths (2 words up to 22 drivers, 3 above; 1 up to 9) and a team layout of up to 10 teams."""
    case = _field(n)
    rng = np.random.default_rng(100 + n)
    drivers = list(case['grid_probs'])
    standings = {d: {'points': int(rng.integers(0, 60)), 'finishes': [int(x) for x in rng.integers(0, 3, min(n, 4))]}
                 for d in drivers[::2]}
    plan = [(case, 11 + n, 32, F1, True), (case, 22 + n, 32, SPRINT, False), (case, 33 + n, 32, F1[:3], True)]
    races = [_race(case, seed, points=pts, countback=cb) for _, seed, _, pts, cb in plan]
    res = run_championship(races, 500, standings=standings, sim_offset=7, set_pop=O.load_cases()['set_pop'],
                           return_race_histograms=True)
    _check(res, {}, plan, 500, 7, standings)


def test_across_the_chunk_boundary(require_gpu):
    """2^22 + 1000 simulations x 3 races: the second chunk starts its keys from the standings again.  Reference orders
    from run_monte_carlo(return_orders=True), themselves pinned to the oracle."""
    case = _field(6)
    n_sims = (1 << 22) + 1000
    drivers = list(case['grid_probs'])
    standings = {drivers[1]: {'points': 20, 'finishes': [0, 1]}, drivers[3]: 4}
    plan = [(11, F1, True), (12, SPRINT, False), (13, F1, True)]
    set_pop = O.load_cases()['set_pop']
    res = run_championship([_race(case, s, points=p, countback=cb) for s, p, cb in plan], n_sims, standings=standings,
                           set_pop=set_pop, return_race_histograms=True)
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=set_pop)
    orders = [sim.run_monte_carlo(n_sims, case['grid_probs'], case['base_pace'], case['tire_deg'],
                                  case['driver_variance'], case['driver_dnf_rates'], seed=s,
                                  track_condition=case['track_condition'], return_orders=True)[1] for s, _, _ in plan]
    names, team = _teams(case, drivers)
    ip, ic = _standings_arrays(standings, drivers)
    block = 1 << 19
    tot = None
    for s0 in range(0, n_sims, block):
        part = CR.championship([o[s0:s0 + block] for o in orders], [p for _, p, _ in plan], [int(c) for _, _, c in plan],
                               team, len(names), init_points=ip, init_counts=ic, grouped=True)
        tot = part if tot is None else tuple(a + b for a, b in zip(tot, part))
    champ, teams, gain, races = tot
    assert np.array_equal(res.champ_hist, champ)
    assert np.array_equal(res.team_hist, teams)
    assert np.array_equal(res.gain_hist, gain)
    assert all(np.array_equal(a, b) for a, b in zip(res.race_histograms, races))


def test_splits_over_calls_and_devices_sum_to_the_whole(require_gpu):
    names = ['S60', 'EVT', 'WET']
    cases = {k: O.load_case(k) for k in names}
    races = [_race(cases[k], 40 + i, countback=(i != 1), points=(SPRINT if i == 1 else F1)) for i, k in enumerate(names)]
    set_pop = O.load_cases()['set_pop']
    whole = run_championship(races, 20000, sim_offset=500, set_pop=set_pop, return_race_histograms=True)
    a = run_championship(races, 7777, sim_offset=500, set_pop=set_pop, return_race_histograms=True)
    b = run_championship(races, 20000 - 7777, sim_offset=500 + 7777, set_pop=set_pop, return_race_histograms=True)
    two = run_championship(races, 20000, sim_offset=500, set_pop=set_pop, device=[0, 0], return_race_histograms=True)
    for part in ('champ_hist', 'team_hist', 'gain_hist'):
        assert np.array_equal(getattr(a, part) + getattr(b, part), getattr(whole, part)), part
        assert np.array_equal(getattr(two, part), getattr(whole, part)), part
    for r in range(3):
        assert np.array_equal(a.race_histograms[r] + b.race_histograms[r], whole.race_histograms[r])
        assert np.array_equal(two.race_histograms[r], whole.race_histograms[r])
    # seeds drawn from `seed` for races without one: reproducible, and distinct per race
    unseeded = [dict(r, seed=None) for r in races]
    x = run_championship(unseeded, 3000, seed=9, set_pop=set_pop)
    y = run_championship(unseeded, 3000, seed=9, set_pop=set_pop)
    assert np.array_equal(x.champ_hist, y.champ_hist) and np.array_equal(x.gain_hist, y.gain_hist)


def test_cli_championship_end_to_end(require_gpu, tmp_path, capsys):
    out = tmp_path / 'champ.json'
    assert cli.main(['championship', '--season', '2024', '--from-round', '21', '--simulations', '20000', '--seed', '7',
                     '--json', str(out)]) == 0
    text = capsys.readouterr().out
    assert 'points from round 21 on' in text and "DRIVERS' TITLE PROBABILITIES" in text
    res = json.loads(out.read_text())
    assert abs(sum(res['title_probabilities'].values()) - 1.0) < 1e-9
    assert abs(sum(res['constructor_title_probabilities'].values()) - 1.0) < 1e-9
    assert res['points_from_round_only'] is True and len(res['races']) == 4
    bt = cli.backtest([2024], seed=7, n_simulations=20000)
    for row, race in zip(bt['races'][20:], res['races']):
        assert row['race'] == race['race'] and row['seed'] == race['seed']
        assert race['win_probabilities'] == row['win'], race['race']
