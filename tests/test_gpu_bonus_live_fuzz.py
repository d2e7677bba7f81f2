"""race_fastest_kernel with champ_bonus, and champ_given behind mcgp_run_championship_live, on the device: the fuzz
configurations of the generic kernel family, ties of the fastest lap, the given race as a bonus race (its orders then go
through race_fastest_kernel into the kept staging buffer), bonuses that carry across the key's word boundary, tail tiles
whose byte count is no multiple of 4, and full ties at the top of the standings.

References, none of which shares code with the kernels: championship_bonus_ref on the CPU oracle's per-lap trace,
championship_live_ref.title_given with the bonus matrix, championship_ref's standings.  Every comparison is on counts,
cell for cell; every "at least" is computed from the oracle or the numpy references before a kernel's output is looked
at.  The oracle side runs on the host in a pool of at most 16 threads.

Wall time on one MI355X: about 3 s for the 21 tests, references included, none above 0.6 s."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import championship_bonus_ref as BR
import championship_cases as CC
import championship_live_ref as LR
import championship_ref as CR
import championship_rounds_ref as RR
import generic_cases as G
import oracle_py as O
import resume_ref as RS
from monte_carlo_gp_amd import run_championship
from test_fastest_host_build import assert_ties_of_the_fastest_lap
from test_gpu_championship import F1, SPRINT, _race, _teams
from test_gpu_championship_bonus import KERNEL, _kernel
from test_gpu_championship_live import (SET_POP, _check_live, _field_standings, _given_lds, _resumed_orders,
                                        _traced_state)

pytestmark = pytest.mark.gpu

SLICES = 4
SHORT = [5, 3, 1]


def _pool():
    return ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))


# ---------------------------------------------------------------- 1. race_fastest_kernel on the fuzz configurations
def _sims(name):
    return 64 if name == 'X_no_noise' else 32


@pytest.mark.parametrize('part', range(SLICES))
def test_fastest_kernel_on_every_fuzz_configuration(require_gpu, part):
    """Every input of generic_cases.run_inputs() (8 golden, 84 fuzz, two with tiny lap times, six field sizes), dealt into
    SLICES tests; 32 simulations under the case's own seed, sim_offset 3, 64 for X_no_noise, whose fastest laps tie.

    First call: one race with an all-zero table, no countback, a bonus of 1 within n, and the race itself as the given
    race.  The bonus is the season's only point, so the champion is the fastest-lap driver (driver 0 where there is
    none), and title_given[e][p][e] is the joint count of (fastest-lap driver e, classified p + 1-th), which no histogram
    gives.  The host accepts the all-zero table.  With a given race the launch the library describes last is
    champ_given's, so the race kernel's name is asserted after the second call, which has no given race.

    Second call: three races of the same case and seed, 5-3-1, countback, bonuses 1, 2, 3 within 1, (n + 1) // 2, n, by
    round: every season, round and bonus output equals championship_bonus_ref."""
    inputs = G.run_input_slices(SLICES)[part]
    O.lib()
    with _pool() as pool:
        refs = list(pool.map(lambda a: BR.race(a[1], _sims(a[0]), a[2], 3), inputs))
    done = 0
    for (name, case, seed), r in zip(inputs, refs):
        m = _sims(name)
        if name == 'X_no_noise':
            assert_ties_of_the_fastest_lap(case, m, seed, 3)
        drivers = list(case['grid_probs'])
        n = len(drivers)
        names, team = _teams(case, drivers)
        kw = dict(sim_offset=3, set_pop=SET_POP, drivers=drivers, return_race_histograms=True)
        # ---- the bonus alone
        ref = BR.season([r], [[0]], [0], team, len(names), [1], [n], by_round=False)
        matrix = BR.bonus_matrix([r], [1], [n])
        champ = LR.champions([r['orders']], [[0]], [0], bonus=matrix)
        assert np.array_equal(champ, np.where(r['fl_driver'] != BR.NONE, r['fl_driver'], 0)), name
        want = LR.title_given([r['orders']], [[0]], [0], 0, bonus=matrix)
        res = run_championship([_race(case, seed, points=[0], countback=False, fastest_lap_points=1, fastest_lap_within=n)],
                               m, given_race=0, **kw)
        assert _given_lds(n)[0] == _given_lds(n)[1], name                  # (champ_given's launch, its table in LDS)
        assert np.array_equal(res.race_histograms[0], ref['race_hist'][0]), name
        assert np.array_equal(res.fastest_lap_counts, ref['fastest_hist']), name
        assert np.array_equal(res.bonus_counts, ref['bonus_hist']), name
        assert np.array_equal(res.champ_hist, ref['champ_hist']) and np.array_equal(res.gain_hist, ref['gain_hist']), name
        assert np.array_equal(res.team_hist, ref['team_hist']), name
        assert np.array_equal(res.title_given, want), name
        LR.check_invariants(res.title_given, res.race_histograms[0], res.champ_hist)
        # ---- three races, three limits
        table = SHORT[:n]
        bp, bw = [1, 2, 3], [1, (n + 1) // 2, n]
        ref = BR.season([r] * 3, [table] * 3, [1] * 3, team, len(names), bp, bw, by_round=True)
        races = [_race(case, seed, points=table, countback=True, fastest_lap_points=b, fastest_lap_within=w)
                 for b, w in zip(bp, bw)]
        res = run_championship(races, m, by_round=True, **kw)
        assert _kernel() == KERNEL, name
        got = dict(champ_hist=res.champ_hist, team_hist=res.team_hist, gain_hist=res.gain_hist,
                   race_hist=np.array(res.race_histograms), bonus_hist=res.bonus_counts, fastest_hist=res.fastest_lap_counts,
                   **{k: getattr(res, k) for k in RR.KEYS})
        for k in BR.SEASON_KEYS + BR.BONUS_KEYS + RR.KEYS:
            assert np.array_equal(got[k], ref[k]), (name, k)
        done += name in G.fuzz_cases()
    assert done == sum(name in G.fuzz_cases() for name, _, _ in inputs) >= G.N_FUZZ // SLICES


# ---------------------------------------------------------------- 2. the given race is a bonus race
BONUS_SIMS = 517                                   # champ_given's tail tile has 5 simulations


@functools.lru_cache(maxsize=None)
def _bonus_season(n):
    """Three races of field_case(n), 5-3-1 with countback: race 0 from the lap-20 state of the oracle's simulation 0,
    race 1 with a bonus of 7 within n // 2, race 2 with 40 within n.  Every driver carries in top - (17 .. 39) points,
    the pattern of test_gpu_championship_bonus._layout_season, so whoever takes race 2's bonus ends at `top` or above.

    top is a boundary of the key's points field: where the field straddles two words with b >= 6 bits in the lower one
    (n = 10: 2^14, n = 23: 2^13), top = 2^b, the first total whose upper-word part is not zero.  At n = 12 and 25 (b = 4
    and 3) 2^b - 39 would be negative, and at the other sizes the field lies in one word: there top = 0x8000, bit 15 of
    the field -- also a multiple of 2^b, so the add still carries out of the lower word at n = 12 and 25.

    Shared by the tests below and never changed: (plan, state, standings, bonus, reference races, top)."""
    case = RS.field_case(n)
    table = SHORT[:n]
    plan = [(case, 31 + n, 32, table, True), (case, 62 + n, 32, table, True), (case, 93 + n, 32, table, True)]
    b = CC.points_low_bits(n)
    top = 1 << b if b >= 6 else 0x8000
    rng = np.random.default_rng(900 + n)
    ip = top - rng.integers(17, 40, n)
    ic = rng.integers(0, 29, (n, n))                                   # 28 + three countback races = 31, the limit
    drivers = list(case['grid_probs'])
    standings = {d: {'points': int(ip[i]), 'finishes': [int(x) for x in ic[i]]} for i, d in enumerate(drivers)}
    bonus = [(0, 1), (7, max(1, n // 2)), (40, n)]
    state, _ = _traced_state(case, plan[0][1], 0, 20)
    first = _resumed_orders(case, state, plan[0][1], BONUS_SIMS, 7)[0]          # (pinned to the oracle by test_gpu_resume)
    with _pool() as pool:
        later = list(pool.map(lambda p: BR.race(p[0], BONUS_SIMS, p[1], 7), plan[1:]))
    none = np.full(BONUS_SIMS, BR.NONE, np.int64)
    races = [dict(orders=first, fl_driver=none, fl_pos=none)] + later
    # ---- what the season is there for, from the references alone
    tables, cb = [table] * 3, [1, 1, 1]
    bp, bw = [x for x, _ in bonus], [w for _, w in bonus]
    _, team = _teams(case, drivers)
    changed = BR.changed_by_the_bonus(races, tables, cb, team, max(team) + 1, bp, bw, ip, ic)
    matrix = BR.bonus_matrix(races, bp, bw)
    pts, _ = CR.standings([r['orders'] for r in races], tables, cb, ip, ic)
    before = pts + matrix[:2].sum(axis=0)
    took = matrix[2] > 0
    carried = int((took & (before < top) & (before + 40 >= top)).any(axis=1).sum())
    print(f'n = {n}, top = {top:#x}: the bonuses change the champion in {changed["champions"]} of {BONUS_SIMS} simulations; '
          f"race 2's bonus carries its taker across top in {carried}")
    assert changed['champions'] >= 1
    # a taker ends on top + 1 at least; it was below top unless it had gained 17 of the 22 points to be had before
    assert (before[took] + 40 >= top).all() and carried >= BONUS_SIMS // 2
    assert ((before + matrix[2] >= top).sum(axis=1) < n).all()            # ... and never the whole field with it
    return plan, state, standings, bonus, races, top


@pytest.mark.parametrize('n', [9, 10, 12, 23, 25, 32])
def test_given_race_is_a_bonus_race(require_gpu, n):
    """517 simulations, each race the given one in a call of its own, by round: every output equals the references with
    the bonuses included.  With given race 1 or 2 race_fastest_kernel writes the kept orders champ_given reads."""
    plan, state, standings, bonus, races, _ = _bonus_season(n)
    _check_live(plan, state, BONUS_SIMS, 7, standings, [0, 1, 2], by_round=True, orders=races, bonus=bonus)
    lds, with_table, _ = _given_lds(n)
    assert lds == with_table                                            # 54 556 bytes at 25 cars, 136 K at 32


@pytest.mark.parametrize('n', [9, 22])
def test_given_bonus_race_under_a_small_lds_budget(require_gpu, monkeypatch, n):
    """The same season with race 1, the bonus race, as the given one under MCGP_LDS_PER_BLOCK=16384: at 22 cars the
    table is counted by global atomics, at 9 cars it stays in LDS."""
    monkeypatch.setenv('MCGP_LDS_PER_BLOCK', '16384')
    plan, state, standings, bonus, races, _ = _bonus_season(n)
    _check_live(plan, state, BONUS_SIMS, 7, standings, [1], by_round=True, orders=races, bonus=bonus)
    lds, with_table, without = _given_lds(n)
    assert lds == (with_table if n == 9 else without) and (with_table <= 16384) == (n == 9)


# ---------------------------------------------------------------- 3. the tail bytes of champ_given's tile
TAIL_SIMS = [1, 255, 257, 258, 259]


@pytest.mark.parametrize('n', [1, 9, 23])
def test_tail_bytes_of_the_tile(require_gpu, monkeypatch, n):
    """The last tile's orders end 1, 2 and 3 bytes past a whole word: champ_given copies those bytes one by one.  Two
    races from the grid, the second the given one, under the device's LDS budget and under MCGP_LDS_PER_BLOCK=16384.
    At 23 cars the second budget moves the table to global atomics; at 1 and 9 cars tile and table (260 and 5 220 bytes)
    fit any budget the library accepts (16 384 at least), so both runs count in LDS."""
    assert {CC.tail_bytes(n, s) for s in TAIL_SIMS} == {1, 2, 3}
    case = RS.field_case(n)
    drivers = list(case['grid_probs'])
    plan = [(case, 11 + n, 32, F1, True), (case, 12 + n, 32, SPRINT, False)]
    standings = _field_standings(n, drivers)
    for n_sims in TAIL_SIMS:
        orders = None
        for budget in (None, 16384):
            if budget:
                monkeypatch.setenv('MCGP_LDS_PER_BLOCK', str(budget))
            else:
                monkeypatch.delenv('MCGP_LDS_PER_BLOCK', raising=False)
            _, orders = _check_live(plan, None, n_sims, 7, standings, [1], orders=orders)
            lds, with_table, without = _given_lds(n)
            assert lds == (without if budget and with_table > budget else with_table), (n_sims, budget)
    assert with_table > 16384 if n == 23 else with_table <= 16384


# ---------------------------------------------------------------- 4. full ties at the top
@pytest.mark.parametrize('n', [2, 10, 23])
def test_full_ties_go_to_the_lowest_index(require_gpu, n):
    """Two races that pay the winner one point and do not count back, no standings: whenever the wins are split, two
    drivers are level on the whole key, and champ_given's running maximum must name the one champ_rank puts first, the
    lower index.  Then a season that pays nothing: every key is equal and driver 0 is champion everywhere."""
    case = RS.field_case(n)
    n_sims = 300
    plan = [(case, 41 + n, 32, [1], False), (case, 82 + n, 32, [1], False)]
    orders = [O.Problem(c).run(n_sims, rng=O.RNG_PHILOX, seed=seed, sim_offset=7, want_orders=True)['orders']
              for c, seed, _, _, _ in plan]
    pts, cnt = CR.standings(orders, [[1], [1]], [0, 0])
    level = int(((pts == pts.max(axis=1)[:, None]).sum(axis=1) >= 2).sum())
    print(f'n = {n}: {level} of {n_sims} simulations with two drivers level on the top key')
    assert not cnt.any() and level >= 100
    res, _ = _check_live(plan, None, n_sims, 7, {}, [1], orders=orders)
    zero = [(c, seed, dev, [0], False) for c, seed, dev, _, _ in plan]
    res, _ = _check_live(zero, None, n_sims, 7, {}, [1], orders=orders)
    assert not res.title_given[:, :, 1:].any()
    assert np.array_equal(res.title_given[:, :, 0], CR.race_histogram(orders[1]))
