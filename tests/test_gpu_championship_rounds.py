"""mcgp_run_championship_rounds on the device: the standings, contention and secure titles after every race equal
championship_rounds_ref fed with the CPU oracle's finishing orders, count for count, and the four season outputs equal
mcgp_run_championship's.  No tolerance anywhere.

Wall time on one MI355X, behind test_gpu_championship_rounds_limits.py in one pytest command: 2.3 s for the 12 tests
here, 1.5 s of it the six-race season of 3000 simulations with its oracle runs."""
import ctypes as C
import json

import numpy as np
import pytest

import championship_cases as CC
import championship_ref as CR
import championship_rounds_ref as RR
import oracle_py as O
from monte_carlo_gp_amd import RaceConfig, cli, run_championship
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import simulation as S
from test_gpu_championship import F1, SPRINT, _race, _standings_arrays, _teams

pytestmark = pytest.mark.gpu

SET_POP = O.load_cases()['set_pop']
OLD = ('champ_hist', 'team_hist', 'gain_hist')


def _assert_rounds(res, orders, tables, cb, team, T, ip, ic, n_sims):
    per = RR.per_simulation(orders, tables, cb, team, T, ip, ic)
    ref = RR.rounds(orders, tables, cb, team, T, sims=per)
    for k in RR.KEYS:
        assert np.array_equal(getattr(res, k), ref[k]), k
    RR.assert_identities({k: getattr(res, k) for k in RR.KEYS}, n_sims, res.champ_hist, res.team_hist)
    return per


def _assert_old_outputs_equal(res, plain):
    for k in OLD:
        assert np.array_equal(getattr(res, k), getattr(plain, k)), k
    for a, b in zip(res.race_histograms, plain.race_histograms):
        assert np.array_equal(a, b)


def _run_season(season, by_round=True):
    races = [_race(case, seed, points=table, countback=cb) for case, seed, _, table, cb in season['plan']]
    return run_championship(races, season['n_sims'], standings=season['standings'], sim_offset=season['sim_offset'],
                            set_pop=SET_POP, return_race_histograms=True, by_round=by_round)


def _compare_season(season):
    orders = CC.oracle_orders(season)
    team, T = CC.team_of(season)
    ip, ic = CC.standings_arrays(season)
    tables, cb = [p[3] for p in season['plan']], [int(p[4]) for p in season['plan']]
    res = _run_season(season)
    per = _assert_rounds(res, orders, tables, cb, team, T, ip, ic, season['n_sims'])
    _assert_old_outputs_equal(res, _run_season(season, by_round=False))
    return res, per


def test_six_race_season_equals_the_oracle(require_gpu):
    """The golden season of test_gpu_championship: six cases of one 20-driver field, one race at the reference's deviate
    width, one sprint, carried-in standings, a non-zero sim_offset, 3000 simulations."""
    names = ['S60', 'S78', 'S50', 'EVT', 'DMP', 'WET']
    cases = {k: O.load_case(k) for k in names}
    plan = [('S60', 101, 32, F1, True), ('S78', 202, 32, F1, True), ('S50', 303, 32, F1, True),
            ('EVT', 404, 53, F1, True), ('DMP', 505, 32, SPRINT, False), ('WET', 606, 32, F1, True)]
    drivers = list(cases['S60']['grid_probs'])
    standings = {drivers[0]: {'points': 51, 'finishes': [2, 0, 0, 1]}, drivers[2]: {'points': 51, 'finishes': [2, 0, 1]},
                 drivers[4]: 33, drivers[6]: {'points': 18, 'finishes': [0, 1]}, drivers[19]: 1}
    races = [_race(cases[c], seed, deviates=dev, points=pts, countback=cb) for c, seed, dev, pts, cb in plan]
    n_sims, offset = 3000, 98765
    kw = dict(standings=standings, sim_offset=offset, set_pop=SET_POP, return_race_histograms=True)
    res = run_championship(races, n_sims, by_round=True, **kw)
    orders = [O.Problem(cases[c]).run(n_sims, rng=O.RNG_PHILOX53 if dev == 53 else O.RNG_PHILOX, seed=seed,
                                      sim_offset=offset, want_orders=True)['orders'] for c, seed, dev, _, _ in plan]
    team_names, team = _teams(cases['S60'], drivers)
    assert res.teams == team_names
    ip, ic = _standings_arrays(standings, drivers)
    _assert_rounds(res, orders, [p[3] for p in plan], [int(p[4]) for p in plan], team, len(team_names), ip, ic, n_sims)
    _assert_old_outputs_equal(res, run_championship(races, n_sims, **kw))
    champ, teams, gain, _ = CR.championship(orders, [p[3] for p in plan], [int(p[4]) for p in plan], team, len(team_names),
                                            init_points=ip, init_counts=ic)
    assert np.array_equal(res.champ_hist, champ) and np.array_equal(res.team_hist, teams) and np.array_equal(res.gain_hist, gain)
    dec = res.decided_by_round
    assert all(a <= b for a, b in zip(dec, dec[1:])) and dec[-1] == 1.0
    assert abs(sum(sum(v.values()) for v in res.clinch_round_probabilities.values()) - 1.0) < 1e-12


@pytest.mark.parametrize('n', [1, 2, 9, 10, 22, 23, 32])
def test_field_sizes_equal_the_oracle(require_gpu, n):
    """1, 2 and 3 key words, the points field in one word (9, 22, 32) and across two (10, 23); 5 races of 25 laps, a
    short table and close carried-in totals, so that contention is decided near the bound; 600 simulations: 10 tiles."""
    rng = np.random.default_rng(300 + n)
    season = CC.tie_rich(n, n_sims=600, points=[int(CC.tie_rich_points(n) - x) for x in rng.integers(0, 10, n)])
    assert len(season['plan']) == 5 and season['case']['config']['total_laps'] == 25
    _, per = _compare_season(season)
    if n >= 9:
        assert 0 < per[2]['contend'].sum() < 600 * n and RR.edges(per, 600)['driver_on_bound'] > 0


def decisive_season():
    """Six cars 0.3 s a step apart, teams of two, five short Grands Prix, a two-place sprint and a last Grand Prix; the
    fastest driver carries in 4 points.  Tuned on the CPU oracle: the title is secure in 97, 261 and 369 of 500 seasons
    after races 3, 4 and 5."""
    n, races = 6, 7
    case = CC.field(n, pace_step=0.3, team=[i // 2 for i in range(n)])
    drivers = list(case['grid_probs'])
    tables = [CC.SHORT] * (races - 2) + [[2, 1]] + [CC.SHORT]
    cb = [True] * (races - 2) + [False, True]
    plan = [(case, 900 + r, 32, tables[r], cb[r]) for r in range(races)]
    return dict(case=case, plan=plan, standings={drivers[0]: {'points': 4, 'finishes': []}}, n_sims=500, sim_offset=11)


def test_decisive_season(require_gpu):
    """A season decided at different rounds, from race-kernel orders: first the reference alone proves that some but
    not all titles are secure at three rounds, that non-leaders sit exactly on the bound among drivers and among teams,
    that seasons end level on points and that a sprint has a shorter table; then every count is compared."""
    season = decisive_season()
    orders = CC.oracle_orders(season)
    team, T = CC.team_of(season)
    ip, ic = CC.standings_arrays(season)
    tables, cb = [p[3] for p in season['plan']], [int(p[4]) for p in season['plan']]
    per = RR.per_simulation(orders, tables, cb, team, T, ip, ic)
    RR.assert_decisive(per, season['n_sims'], tables, cb)
    res, _ = _compare_season(season)
    dec = res.decided_by_round
    assert 0 < dec[3] < dec[4] < dec[5] < dec[6] == 1.0


# ---------------------------------------------------------------- properties that need no oracle run
class _Abi:
    """mcgp_run_championship_rounds called directly on caller-owned arrays: races of one 3-car, 5-lap field."""

    def __init__(self, n_races=2):
        case = CC.field(3, laps=5, team=[0, 1, 0])
        drivers = list(case['grid_probs'])
        prob = S._Problem(RaceConfig(**case['config']), drivers, case['base_pace'], case['tire_deg'], case['driver_variance'],
                          case['driver_dnf_rates'], case['track_condition'], SET_POP)
        self.keep = (prob, S.RaceSimulator._grid_matrix(case['grid_probs'], drivers))
        R = self.R = n_races
        self.cfgs = (N.McgpConfig * R)(*[prob.cfg] * R)
        self.drvs = (N.McgpDrivers * R)(*[prob.drv] * R)
        self.grids = (C.POINTER(C.c_double) * R)(*[S._dptr(self.keep[1])] * R)
        self.seeds = (C.c_uint64 * R)(*[71 + r for r in range(R)])
        self.points = np.ascontiguousarray([[3, 2, 1], [2, 1, 0]][:R], np.int32)
        self.cb = np.ascontiguousarray([1, 0][:R], np.uint8)
        self.team = np.ascontiguousarray([0, 1, 0], np.int32)
        self.ip = np.ascontiguousarray([2, 0, 0], np.int32)

    def arrays(self, fill=0):
        R, n, T, G = self.R, 3, 2, int(self.points.max(axis=1).sum())
        shapes = [(n, n), (T, T), (n, G + 1), (R, n, n), (R, n, n), (R, n), (R, n), (R, T, T), (R, T), (R, T)]
        return [np.full(s, fill, np.uint64) for s in shapes]

    def run(self, arrays, n_sims, offset=0, n_teams=2):
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        lib = N.lib()
        rc = lib.mcgp_run_championship_rounds(self.R, self.cfgs, self.drvs, self.grids, 3, n_sims, offset, self.seeds,
                                              i32(self.points), self.cb.ctypes.data_as(C.POINTER(C.c_uint8)), i32(self.ip),
                                              None, i32(self.team), n_teams, 0,
                                              *[a.ctypes.data_as(C.POINTER(C.c_uint64)) for a in arrays])
        return rc, lib.mcgp_last_error().decode()


def test_across_the_chunk_boundary(require_gpu):
    """2^22 + 1000 simulations of two races equal the sum of two calls split at 2^22: the second chunk's per-round
    kernels start from the standings again, in a key buffer the first chunk has used, with a last tile of 40."""
    abi = _Abi()
    cut, n_sims = 1 << 22, (1 << 22) + 1000
    whole, parts = abi.arrays(), abi.arrays()
    assert abi.run(whole, n_sims, 5)[0] == 0
    assert abi.run(parts, cut, 5)[0] == 0
    first = [a.copy() for a in parts]
    assert abi.run(parts, 1000, 5 + cut)[0] == 0                  # two calls into the same arrays accumulate
    for w, p, f in zip(whole, parts, first):
        assert np.array_equal(w, p) and (p >= f).all() and p.sum() > f.sum()
    round_hist, secure = whole[4].astype(np.int64), whole[6].astype(np.int64)
    assert (round_hist.sum(axis=2) == n_sims).all() and np.array_equal(round_hist[-1], whole[0].astype(np.int64))
    assert np.array_equal(secure[-1], round_hist[-1][:, 0]) and (np.diff(secure, axis=0) >= 0).all()
    assert 0 < secure[0].sum() < n_sims                           # race 0 settles some seasons and not others


def test_a_call_that_fails_leaves_its_outputs_untouched(require_gpu):
    abi = _Abi()
    poison = 0xDEADBEEFDEADBEEF
    arrays = abi.arrays(poison)
    rc, err = abi.run(arrays, 1000, n_teams=0)
    assert rc == -1 and 'n_teams' in err
    assert all((a == poison).all() for a in arrays)
    assert abi.run(arrays, 1000)[0] == 0
    assert all((a >= poison).all() for a in arrays) and (arrays[4] > poison).any()


def test_cli_by_round_end_to_end(require_gpu, tmp_path, capsys):
    out = tmp_path / 'rounds.json'
    assert cli.main(['championship', '--season', '2024', '--from-round', '22', '--simulations', '2000', '--seed', '7',
                     '--by-round', '--json', str(out)]) == 0
    text = capsys.readouterr().out
    assert 'BY ROUND' in text and 'in contention' in text
    res = json.loads(out.read_text())
    dec = res['decided_by_round']
    assert len(dec) == 3 == len(res['races']) and all(a <= b for a, b in zip(dec, dec[1:])) and dec[-1] == 1.0
    assert len(res['leader_probabilities_by_round']) == 3 and len(res['contention_probabilities_by_round']) == 3
    assert abs(sum(res['leader_probabilities_by_round'][0].values()) - 1.0) < 1e-9
    assert abs(sum(sum(v.values()) for v in res['clinch_round_probabilities'].values()) - 1.0) < 1e-9
    assert res['constructor_decided_by_round'][-1] == 1.0
