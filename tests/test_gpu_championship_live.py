"""mcgp_run_championship_live on the device: a championship whose first race resumes from a mid-race state, and the title
odds by finishing position.  The live race's orders are RaceSimulator.run_from_state's (pinned to the CPU oracle by
tests/test_gpu_resume.py) or the oracle's own, the other races' the oracle's; every histogram equals championship_ref,
championship_rounds_ref and championship_live_ref fed with them, count for count.  No tolerance anywhere."""
import ctypes as C
import dataclasses
import json

import numpy as np
import pytest

import championship_bonus_ref as BR
import championship_live_ref as LR
import championship_ref as CR
import championship_rounds_ref as RR
import oracle_py as O
import resume_ref as RS
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, cli, run_championship
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import simulation as S
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP
from test_gpu_championship import F1, SPRINT, _race, _standings_arrays, _teams
from test_gpu_championship_rounds import _assert_rounds

pytestmark = pytest.mark.gpu

SET_POP = O.load_cases()['set_pop']


def _live(case, seed, state, **kw):
    race = _race(case, seed, **kw)
    del race['grid_probs']
    race['state'] = state
    return race


def _traced_state(case, seed, sim, lap, m=None, edit=None):
    """The RaceState of the oracle's simulation `sim` after `lap` laps, and the oracle's run it comes from."""
    ref = RS.traced_run(case, m or sim + 1, seed)
    arrays = RS.state_arrays(ref, sim, lap)
    if edit:
        edit(arrays)
    return RS.race_state(arrays, lap, RS.drs_disabled_until(case, seed, sim, lap), list(case['grid_probs'])), ref


def _resumed_orders(case, state, seed, n_sims, sim_offset):
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=SET_POP)
    _, orders = sim.run_from_state(n_sims, state, case['base_pace'], case['tire_deg'], case['driver_variance'],
                                   case['driver_dnf_rates'], seed=seed, track_condition=case['track_condition'],
                                   sim_offset=sim_offset, drivers=list(case['grid_probs']), return_orders=True)
    return orders, sim.last_histogram


def _oracle_orders(case, seed, dev, n_sims, sim_offset):
    rng = O.RNG_PHILOX53 if dev == 53 else O.RNG_PHILOX
    return O.Problem(case).run(n_sims, rng=rng, seed=seed, sim_offset=sim_offset, want_orders=True)['orders']


def _given_lds(n):
    """The dynamic LDS of the last champ_given launch, and what it is in the two modes: (lds, with table, without)."""
    vals = [C.c_uint32() for _ in range(3)]
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::champ_given'
    assert N.lib().mcgp_last_launch_info(0, *[C.byref(v) for v in vals]) == 0
    tile = (256 * n + 15) // 16 * 16
    return vals[2].value, tile + 4 * n ** 3, tile


def _check_live(plan, state, n_sims, sim_offset, standings, given, by_round=False, orders=None, bonus=None, **kw):
    """plan: [(case, seed, deviates, table, countback)], race 0 from `state` (from the grid when state is None).  Every
    given race of `given` in a call of its own against the references; returns (the last result, the races' reference
    orders).  bonus: None, or [(fastest-lap points, within)] per race (0 points: none); the references are then
    championship_bonus_ref's on the oracle's traced runs of the bonus races, title_given's with the bonus matrix."""
    case0 = plan[0][0]
    drivers = list(case0['grid_probs'])
    extra = [{}] * len(plan) if bonus is None else [dict(fastest_lap_points=b, fastest_lap_within=w) for b, w in bonus]
    if state is None:
        races = [_race(case0, plan[0][1], deviates=plan[0][2], points=plan[0][3], countback=plan[0][4], **extra[0])]
    else:
        races = [_live(case0, plan[0][1], state, points=plan[0][3], countback=plan[0][4], **extra[0])]
    races += [_race(c, seed, deviates=dev, points=pts, countback=cb, **e) for (c, seed, dev, pts, cb), e in zip(plan[1:], extra[1:])]
    traced = {}
    if orders is None:
        if state is None:
            orders = [_oracle_orders(case0, plan[0][1], plan[0][2], n_sims, sim_offset)]
        else:
            orders = [_resumed_orders(case0, state, plan[0][1], n_sims, sim_offset)[0]]
        for r, (c, seed, dev, _, _) in enumerate(plan[1:], 1):
            if bonus is not None and bonus[r][0] > 0:
                traced[r] = BR.race(c, n_sims, seed, sim_offset)          # (a bonus race runs at 32-bit deviates only)
                orders.append(traced[r]['orders'])
            else:
                orders.append(_oracle_orders(c, seed, dev, n_sims, sim_offset))
    else:
        orders = list(orders)
        for r, o in enumerate(orders):
            if isinstance(o, dict):                                       # a championship_bonus_ref race the caller has
                traced[r], orders[r] = o, o['orders']
    names, team = _teams(case0, drivers)
    ip, ic = _standings_arrays(standings, drivers)
    tables, cb = [p[3] for p in plan], [int(p[4]) for p in plan]
    matrix = ref = None
    if bonus is None:
        champ, teams, gain, race_hists = CR.championship(orders, tables, cb, team, len(names), init_points=ip, init_counts=ic)
    else:
        assert bonus[0][0] == 0 or state is None
        none = np.full(n_sims, BR.NONE, np.int64)
        if state is None and bonus[0][0] > 0:
            traced[0] = BR.race(case0, n_sims, plan[0][1], sim_offset)
            assert np.array_equal(traced[0]['orders'], orders[0])
        ref_races = [traced.get(r, dict(orders=o, fl_driver=none, fl_pos=none)) for r, o in enumerate(orders)]
        assert all(b == 0 or r in traced for r, (b, _) in enumerate(bonus))
        bp, bw = [b for b, _ in bonus], [w for _, w in bonus]
        matrix = BR.bonus_matrix(ref_races, bp, bw)
        ref = BR.season(ref_races, tables, cb, team, len(names), bp, bw, ip, ic, by_round=by_round)
        champ, teams, gain, race_hists = (ref[k] for k in BR.SEASON_KEYS)
    res = None
    for g in given:
        res = run_championship(races, n_sims, standings=standings, sim_offset=sim_offset, set_pop=SET_POP, drivers=drivers,
                               return_race_histograms=True, by_round=by_round, given_race=g, **kw)
        assert res.drivers == drivers and res.teams == names and res.given_race == g
        assert np.array_equal(res.champ_hist, champ) and np.array_equal(res.team_hist, teams)
        assert np.array_equal(res.gain_hist, gain)
        for r, h in enumerate(res.race_histograms):
            assert np.array_equal(h, race_hists[r]), r
        if ref is not None and any(b > 0 for b, _ in bonus):
            assert np.array_equal(res.bonus_counts, ref['bonus_hist']), g
            assert np.array_equal(res.fastest_lap_counts, ref['fastest_hist']), g
        if g is None:
            assert res.title_given is None
            continue
        assert np.array_equal(res.title_given, LR.title_given(orders, tables, cb, g, ip, ic, bonus=matrix)), g
        LR.check_invariants(res.title_given, res.race_histograms[g], res.champ_hist)
        if by_round and ref is not None:
            for k in RR.KEYS:
                assert np.array_equal(getattr(res, k), ref[k]), (g, k)
            RR.assert_identities({k: getattr(res, k) for k in RR.KEYS}, n_sims, res.champ_hist, res.team_hist)
        elif by_round:
            _assert_rounds(res, orders, tables, cb, team, len(names), ip, ic, n_sims)
    return res, orders


# ---------------------------------------------------------------- 1. the live race equals the oracle
def test_live_race_equals_the_oracle(require_gpu):
    """S60 under seed 42: the state of the oracle's simulation i after lap 30, resumed as simulation i of a two-race
    season, finishes race 0 in the oracle's order of i; the standings are championship_ref's on the two oracle orders."""
    case, later = O.load_case('S60'), O.load_case('S78')
    seed, m, k = 42, 8, 30
    drivers = list(case['grid_probs'])
    ref = RS.traced_run(case, m, seed)
    second = _oracle_orders(later, 202, 32, m, 0)
    names, team = _teams(case, drivers)
    for i in range(m):
        state = RS.race_state(RS.state_arrays(ref, i, k), k, RS.drs_disabled_until(case, seed, i, k), drivers)
        res = run_championship([_live(case, seed, state), _race(later, 202)], 1, sim_offset=i, set_pop=SET_POP,
                               drivers=drivers, return_race_histograms=True)
        assert np.array_equal(res.race_histograms[0], RS.counts(ref['orders'][i:i + 1], 20)), i
        champ, teams, gain, hists = CR.championship([ref['orders'][i:i + 1], second[i:i + 1]], [F1, F1], [1, 1], team, len(names))
        assert np.array_equal(res.champ_hist, champ) and np.array_equal(res.team_hist, teams), i
        assert np.array_equal(res.gain_hist, gain) and np.array_equal(res.race_histograms[1], hists[1]), i


# ---------------------------------------------------------------- 2. a season with a live race
def _season():
    cases = {k: O.load_case(k) for k in ('S60', 'EVT', 'DMP', 'WET')}
    plan = [(cases['S60'], 42, 32, F1, True), (cases['EVT'], 404, 53, F1, True), (cases['DMP'], 505, 32, SPRINT, False),
            (cases['WET'], 606, 32, F1, True)]
    drivers = list(cases['S60']['grid_probs'])
    standings = {drivers[0]: {'points': 51, 'finishes': [2, 0, 0, 1]}, drivers[2]: {'points': 51, 'finishes': [2, 0, 1]},
                 drivers[4]: 33, drivers[6]: {'points': 18, 'finishes': [0, 1]}, drivers[19]: 1}
    return plan, standings


def test_season_with_a_live_race(require_gpu):
    """S60 from the lap-30 state of the oracle's simulation 3, then EVT at the reference's deviate width, a DMP sprint and
    WET; carried-in standings with countback finishes, a non-zero sim_offset, by round, title odds by the finish of the
    live race."""
    plan, standings = _season()
    state, _ = _traced_state(plan[0][0], 42, 3, 30)
    res, orders = _check_live(plan, state, 3000, 98765, standings, [0], by_round=True)
    assert _given_lds(20)[0] == _given_lds(20)[1]                      # 20 cars: the table is in LDS
    assert len({tuple(o) for o in orders[0]}) > 100                  # the rest of the live race is open
    needs = res.title_needs(res.drivers[0])
    assert needs and all(0.0 <= v <= 1.0 for v in needs.values())


# ---------------------------------------------------------------- 3. field sizes and both histogram modes
def _field_plan(n):
    case = RS.field_case(n)
    return [(case, 70 + n, 32, F1, True), (case, 22 + n, 32, SPRINT, False), (case, 33 + n, 32, F1[:3], True)]


def _field_standings(n, drivers):
    rng = np.random.default_rng(100 + n)
    return {d: {'points': int(rng.integers(0, 60)), 'finishes': [int(x) for x in rng.integers(0, 3, min(n, 4))]}
            for d in drivers[::2]}


@pytest.mark.parametrize('n', [1, 2, 9, 22, 23, 32])
def test_field_sizes(require_gpu, n):
    """1, 2 and 3 key words; 25 laps, a state after lap 20, three races, 500 simulations (two tiles of champ_given), each
    race as the given one.  The table is in LDS when it fits the device's LDS per block next to the tile."""
    plan = _field_plan(n)
    drivers = list(plan[0][0]['grid_probs'])
    state, _ = _traced_state(plan[0][0], plan[0][1], 0, 20)
    _check_live(plan, state, 500, 7, _field_standings(n, drivers), [0, 1, 2])
    lds, with_table, without = _given_lds(n)
    assert lds in (with_table, without)
    print(f'n = {n}: champ_given with {lds} bytes of LDS ({"LDS table" if lds == with_table else "global atomics"})')
    if with_table <= 64 * 1024:
        assert lds == with_table


@pytest.mark.parametrize('n', [9, 22])
def test_small_lds_budget(require_gpu, monkeypatch, n):
    """MCGP_LDS_PER_BLOCK=16384, read per call: at 22 cars the table (42 592 bytes) no longer fits and every count is a
    global atomic; at 9 cars tile and table (5 220 bytes) still fit, and the results are the same either way."""
    monkeypatch.setenv('MCGP_LDS_PER_BLOCK', '16384')
    plan = _field_plan(n)
    drivers = list(plan[0][0]['grid_probs'])
    state, _ = _traced_state(plan[0][0], plan[0][1], 0, 20)
    _check_live(plan, state, 500, 7, _field_standings(n, drivers), [0, 1, 2])
    lds, with_table, without = _given_lds(n)
    assert lds == (with_table if with_table <= 16384 else without)


# ---------------------------------------------------------------- 4. state edges
def _classified(arrays):
    """The classification of a state with no lap left: running cars by (time, grid slot), then the retired ones by lap and
    time descending, the lower grid slot first on equal ones."""
    n = len(arrays['grid_slot'])
    running = sorted((d for d in range(n) if arrays['retired_lap'][d] == 0),
                     key=lambda d: (arrays['cumulative_time'][d], arrays['grid_slot'][d]))
    retired = sorted((d for d in range(n) if arrays['retired_lap'][d] != 0),
                     key=lambda d: (-int(arrays['retired_lap'][d]), -arrays['cumulative_time'][d], arrays['grid_slot'][d]))
    return running + retired


def test_state_edges(require_gpu):
    """A state after the last lap (race 0 is the state's own classification in every simulation), after lap 1, and one in
    which all cars but one have retired."""
    n, n_sims = 9, 300
    plan = _field_plan(n)[:2]
    case, seed = plan[0][0], plan[0][1]
    drivers = list(case['grid_probs'])
    standings = _field_standings(n, drivers)
    ref = RS.traced_run(case, 8, seed)
    sim = max(range(8), key=lambda i: int((ref['trace']['dnf'][i, 24] != 0).sum()))     # the most retirements
    last = RS.state_arrays(ref, sim, 25)
    assert (last['retired_lap'] != 0).any() and (last['retired_lap'] == 0).sum() >= 2
    want = _classified(last)
    assert want == [int(d) for d in ref['orders'][sim]]
    state = RS.race_state(last, 25, RS.drs_disabled_until(case, seed, sim, 25), drivers)
    res, orders = _check_live(plan, state, n_sims, 11, standings, [0, 1])
    assert (orders[0] == np.array(want, np.uint8)).all()
    assert res.race_histograms[0][want, np.arange(n)].tolist() == [n_sims] * n
    state, _ = _traced_state(case, seed, 0, 1)
    _check_live(plan, state, n_sims, 11, standings, [0])

    def all_but_one_retired(arrays):
        arrays['retired_lap'][:] = [0] + [3 + d % 5 for d in range(1, n)]
    state, _ = _traced_state(case, seed, 0, 10, edit=all_but_one_retired)
    res, orders = _check_live(plan, state, n_sims, 11, standings, [0])
    assert (orders[0][:, 0] == 0).all() and res.race_histograms[0][0, 0] == n_sims


# ---------------------------------------------------------------- 5. the chunk boundary
def test_across_the_chunk_boundary(require_gpu):
    """2^22 + 1000 simulations of a 4-car field: a live race and a grid race, the grid race the given one.  The second chunk
    starts the kept orders and the keys afresh.  Reference orders from run_from_state and run_monte_carlo, themselves
    pinned to the oracle; the reference ranks in blocks (the drivers' standings: the constructors' have no part in the
    table, and tests/test_gpu_championship.py holds them across the boundary)."""
    case = RS.field_case(4)
    n_sims = (1 << 22) + 1000
    drivers = list(case['grid_probs'])
    standings = {drivers[1]: {'points': 20, 'finishes': [0, 1]}, drivers[3]: 4}
    state, _ = _traced_state(case, 74, 0, 20)
    races = [_live(case, 74, state), _race(case, 12, points=SPRINT, countback=False)]
    res = run_championship(races, n_sims, standings=standings, set_pop=SET_POP, drivers=drivers, return_race_histograms=True,
                           given_race=1)
    first, _ = _resumed_orders(case, state, 74, n_sims, 0)
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=SET_POP)
    second = sim.run_monte_carlo(n_sims, case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'],
                                 case['driver_dnf_rates'], seed=12, track_condition=case['track_condition'],
                                 return_orders=True)[1]
    ip, ic = _standings_arrays(standings, drivers)
    tables, cb = [F1, SPRINT], [1, 0]
    n, G, block = 4, 25 + 8, 1 << 19
    champ, gain, given = np.zeros((n, n), np.int64), np.zeros((n, G + 1), np.int64), np.zeros((n, n, n), np.int64)
    for s0 in range(0, n_sims, block):
        part = [first[s0:s0 + block], second[s0:s0 + block]]
        pts, cnt = CR.standings(part, tables, cb, ip, ic)
        pos = CR.rank_lexsort(pts, cnt)                    # (rank_grouped's positions, several times as fast)
        if len(pos) < block:
            assert np.array_equal(pos, CR.rank_grouped(pts, cnt)) and np.array_equal(pos, CR.rank(pts, cnt))
        champ += CR.histogram(pos, n)
        for d in range(n):
            gain[d] += np.bincount(pts[:, d] - ip[d], minlength=G + 1)
        given += LR.title_given_of(part[1], np.argmin(pos, axis=1))
    assert np.array_equal(res.champ_hist, champ) and np.array_equal(res.gain_hist, gain)
    assert np.array_equal(res.race_histograms[0], CR.race_histogram(first))
    assert np.array_equal(res.race_histograms[1], CR.race_histogram(second))
    assert np.array_equal(res.title_given, given)
    LR.check_invariants(res.title_given, res.race_histograms[1], res.champ_hist)
    assert res.team_hist.sum() == n_sims * len(res.teams)


# ---------------------------------------------------------------- 6. splits
def test_splits_over_calls_and_devices_sum_to_the_whole(require_gpu):
    cases = {k: O.load_case(k) for k in ('S60', 'EVT', 'WET')}
    state, _ = _traced_state(cases['S60'], 42, 3, 30)
    drivers = list(cases['S60']['grid_probs'])
    races = [_live(cases['S60'], 42, state), _race(cases['EVT'], 41, points=SPRINT, countback=False),
             _race(cases['WET'], 43, fastest_lap_points=1)]
    kw = dict(set_pop=SET_POP, drivers=drivers, return_race_histograms=True, by_round=True, given_race=0)
    whole = run_championship(races, 20000, sim_offset=500, **kw)
    a = run_championship(races, 7777, sim_offset=500, **kw)
    b = run_championship(races, 20000 - 7777, sim_offset=500 + 7777, **kw)
    two = run_championship(races, 20000, sim_offset=500, device=[0, 0], **kw)
    fields = [f.name for f in dataclasses.fields(whole) if isinstance(getattr(whole, f.name), np.ndarray)]
    assert {'title_given', 'round_hist', 'team_secure', 'bonus_counts', 'fastest_lap_counts'} <= set(fields)
    for part in fields:
        assert np.array_equal(getattr(a, part) + getattr(b, part), getattr(whole, part)), part
        assert np.array_equal(getattr(two, part), getattr(whole, part)), part
    for r in range(3):
        assert np.array_equal(a.race_histograms[r] + b.race_histograms[r], whole.race_histograms[r])
        assert np.array_equal(two.race_histograms[r], whole.race_histograms[r])
    assert whole.title_given.sum() == 20000 * 20
    LR.check_invariants(whole.title_given, whole.race_histograms[0], whole.champ_hist)


# ---------------------------------------------------------------- 7. without a state and a given race: the old call
def test_no_state_and_no_given_race_is_the_bonus_call(require_gpu):
    """mcgp_run_championship_live with state0 = NULL and given_race = -1 against mcgp_run_championship_bonus on the season
    of test 2 from the grid, with a bonus on the first race: every output equal."""
    plan, standings = _season()
    drivers = list(plan[0][0]['grid_probs'])
    n, R, n_sims = 20, len(plan), 3000
    probs = [S._Problem(RaceConfig(**c['config']), drivers, c['base_pace'], c['tire_deg'], c['driver_variance'],
                        c['driver_dnf_rates'], c['track_condition'], SET_POP, dev) for c, _, dev, _, _ in plan]
    grids = [S.RaceSimulator._grid_matrix(c['grid_probs'], drivers) for c, _, _, _, _ in plan]
    cfgs = (N.McgpConfig * R)(*[p.cfg for p in probs])
    drvs = (N.McgpDrivers * R)(*[p.drv for p in probs])
    gptrs = (C.POINTER(C.c_double) * R)(*[S._dptr(g) for g in grids])
    seeds = (C.c_uint64 * R)(*[p[1] for p in plan])
    points = np.zeros((R, n), np.int32)
    for r, p in enumerate(plan):
        points[r, :len(p[3])] = p[3]
    cb = np.ascontiguousarray([int(p[4]) for p in plan], np.uint8)
    names, team = _teams(plan[0][0], drivers)
    T = len(names)
    team = np.ascontiguousarray(team, np.int32)
    ip, ic = _standings_arrays(standings, drivers)
    ip, ic = np.ascontiguousarray(ip, np.int32), np.ascontiguousarray(ic, np.int32)
    bp, bw = np.ascontiguousarray([1, 0, 0, 0], np.int32), np.ascontiguousarray([10, 1, 1, 1], np.int32)
    G = int(points.max(axis=1).sum()) + 1
    shapes = [(n, n), (T, T), (n, G + 1), (R, n, n), (R, n, n), (R, n), (R, n), (R, T, T), (R, T), (R, T), (R, n), (R, n)]
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    lib = N.lib()

    def call(fn, tail):
        out = [np.zeros(s, np.uint64) for s in shapes]
        rc = fn(R, cfgs, drvs, gptrs, n, n_sims, 98765, seeds, i32(points), cb.ctypes.data_as(C.POINTER(C.c_uint8)), i32(ip),
                i32(ic), i32(team), T, 0, *[u64(a) for a in out[:10]], i32(bp), i32(bw), u64(out[10]), u64(out[11]), *tail)
        assert rc == 0, lib.mcgp_last_error()
        return out

    old = call(lib.mcgp_run_championship_bonus, ())
    new = call(lib.mcgp_run_championship_live, (None, -1, None))
    for k, (a, b) in enumerate(zip(old, new)):
        assert np.array_equal(a, b), k
    assert old[0].sum() == n_sims * n and old[10][0].sum() > 0 and not old[10][1:].any()


# ---------------------------------------------------------------- 8. the CLI end to end
def test_cli_end_to_end(require_gpu, tmp_path, capsys):
    jobs = cli.championship_jobs(2024, 7, 24)
    assert len(jobs) == 1
    inp = cli.championship_races(jobs)[0]
    case = dict(config=dataclasses.asdict(inp['config']), grid_probs=inp['grid_probs'], base_pace=inp['base_pace'],
                tire_deg=inp['tire_deg'], driver_variance=inp['driver_variance'], driver_dnf_rates=inp['driver_dnf_rates'],
                track_condition=inp['track_condition'])
    drivers = [str(d) for d in case['grid_probs']]
    assert 'NOR' in drivers and 'VER' in drivers
    k = 40
    assert case['config']['total_laps'] > k
    ref = O.Problem(case, set_pop=DEFAULT_SET_POP).run(1, rng=O.RNG_PHILOX, seed=inp['seed'], want_orders=True,
                                                       want_grids=True, n_trace=1)
    state = RS.race_state(RS.state_arrays(ref, 0, k), k, RS.drs_disabled_until(case, inp['seed'], 0, k), drivers)
    state_file, standings_file, out = tmp_path / 'lap40.json', tmp_path / 'before24.json', tmp_path / 'live.json'
    state_file.write_text(json.dumps(state.to_json()))
    standings_file.write_text(json.dumps({'VER': {'points': 393, 'finishes': [9, 3]}, 'NOR': {'points': 380, 'finishes': [4, 8]},
                                          'LEC': 372}))
    n_sims = 20000
    assert cli.main(['championship', '--season', '2024', '--from-round', '24', '--standings', str(standings_file), '--state',
                     str(state_file), '--needs', 'NOR', '--needs', 'VER', '--simulations', str(n_sims), '--seed', '7',
                     '--json', str(out)]) == 0
    text = capsys.readouterr().out
    assert 'after lap 40' in text and 'WHAT NOR NEEDS (round 24' in text and 'WHAT VER NEEDS (round 24' in text
    assert "finish  P(finish)  P(title | finish)  rivals' title odds given that finish" in text
    res = json.loads(out.read_text())
    assert res['state_lap'] == 40 and res['given_round'] == 24 and sorted(res['title_needs']) == ['NOR', 'VER']
    for d in ('NOR', 'VER'):
        titles = finishes = 0
        for row in res['title_needs'][d].values():
            count = round(row['p_finish'] * n_sims)
            assert abs(row['p_finish'] * n_sims - count) < 1e-6
            won = round(row['title'][d] * count)
            assert abs(row['title'][d] * count - won) < 1e-6
            titles += won
            finishes += count
        assert finishes == n_sims and titles == round(res['title_probabilities'][d] * n_sims), d
    assert abs(sum(res['title_probabilities'].values()) - 1.0) < 1e-9
