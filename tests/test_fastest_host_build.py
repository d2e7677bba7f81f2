"""race_fastest_kernel (csrc/fastest.hip.h) and champ_bonus (csrc/champ_bonus.hip.h) run from their source on the host
(tools/emu/emu_generic.cpp: emu_fastest_run; tools/emu/emu_champ.cpp: emu_champ_bonus_run) against
championship_bonus_ref, which shares no code with them: raw finishing orders and both byte rows equal the CPU oracle's
trace, and every field of every standing key, decoded with Python integers, equals the restated standings."""
import copy

import numpy as np
import pytest

import championship_bonus_ref as BR
import championship_cases as CC
import championship_ref as CR
import fastest_host_build as FH
import generic_cases as G
import oracle_py as O
import resume_ref as RS

GOLDEN = ['S60', 'S78', 'S50', 'EVT', 'HET', 'DMP', 'WET', 'N10']
SIMS = 48


def _compare_race(case, m, seed, sim_offset=0):
    ref = BR.race(case, m, seed, sim_offset)
    hist, orders, fl_driver, fl_pos = FH.fastest_run(case, m, seed, sim_offset)
    want_d, want_p = FH.bytes_of([ref])
    assert np.array_equal(orders, ref['orders'])
    assert np.array_equal(fl_driver, want_d[0]) and np.array_equal(fl_pos, want_p[0])
    assert np.array_equal(hist, CR.race_histogram(ref['orders']))
    return ref


@pytest.mark.parametrize('name', GOLDEN)
def test_golden_cases(name):
    ref = _compare_race(O.load_case(name), SIMS, seed=42, sim_offset=5)
    assert (ref['fl_driver'] != BR.NONE).all()


def test_fastest_laps_by_cars_that_retire_later():
    """EVT at seed 42: fastest laps by later-retired cars, classified inside and outside the top ten."""
    ref = _compare_race(O.load_case('EVT'), 256, seed=42)
    inside = int((ref['fl_retired'] & (ref['fl_pos'] < 10)).sum())
    outside = int((ref['fl_retired'] & (ref['fl_pos'] >= 10)).sum())
    assert (inside, outside) == (13, 18)


@pytest.mark.parametrize('n', [1, 2, 32])
def test_field_sizes(n):
    _compare_race(RS.field_case(n), SIMS, seed=7 + n)


@pytest.mark.parametrize('name', ['S60', 'N10'])
def test_a_race_of_one_lap_has_no_fastest_lap(name):
    case = copy.deepcopy(O.load_case(name))
    case['config']['total_laps'] = 1
    ref = _compare_race(case, SIMS, seed=3)
    assert (ref['fl_driver'] == BR.NONE).all() and (ref['fl_pos'] == BR.NONE).all()
    _, _, fl_driver, fl_pos = FH.fastest_run(case, SIMS, 3)
    assert (fl_driver == 0xFF).all() and (fl_pos == 0xFF).all()


def test_a_race_in_which_everybody_retires_on_lap_1():
    """No car completes a lap >= 2 although L > 1: none."""
    case = copy.deepcopy(RS.field_case(3))
    case['config']['dnf_rates'] = {k: 1.0 for k in case['config']['dnf_rates']}
    ref = _compare_race(case, 16, seed=1)
    assert (ref['fl_driver'] == BR.NONE).all()


def test_every_fuzz_configuration():
    """The generic family's inputs (8 golden, 84 fuzz, lap times near zero and at the overtake's floor, six field sizes):
    32 simulations each under the case's own seed, sim_offset 3.  Under a second for the hundred, references included."""
    done = 0
    for name, case, seed in G.run_inputs():
        _compare_race(case, 32, seed, sim_offset=3)
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ


def _last_of_equal_times_wins(ref):
    """The fastest-lap driver [m] under the WRONG tie rule, <= instead of <: of equal times the later lap, then the worse
    running position (-1 for none)."""
    tr, m, n = ref['trace'], *ref['orders'].shape
    rows = np.arange(m)
    slot = np.zeros((m, n), np.int64)
    slot[rows[:, None], ref['grids']] = np.arange(n)[None, :]
    best, driver = np.full(m, np.inf), np.full(m, BR.NONE, np.int64)
    for k in range(1, tr['cum'].shape[1]):
        order = np.lexsort((slot, tr['cum'][:, k, :]), axis=-1)
        t = np.where(np.take_along_axis(tr['dnf'][:, k, :], order, axis=1) == 0,
                     np.take_along_axis(tr['last'][:, k, :], order, axis=1), np.inf)
        j = n - 1 - np.argmin(t[:, ::-1], axis=1)                       # the last of equal times
        better = (t[rows, j] <= best) & np.isfinite(t[rows, j])
        best, driver = np.where(better, t[rows, j], best), np.where(better, order[rows, j], driver)
    return driver


def assert_ties_of_the_fastest_lap(case, m, seed, sim_offset):
    """From the oracle's trace alone: in at least 32 of X_no_noise's simulations two drivers share the race's fastest
    time, in at least one it is set on two laps, and in at least 32 the tie rule decides who has the fastest lap."""
    ref = RS.traced_run(case, m, seed, sim_offset)
    two_drivers, two_laps = G.fastest_lap_ties(ref)
    print(f'fastest-lap ties of {m} simulations: {two_drivers} between two drivers, {two_laps} across two laps')
    assert two_drivers >= 32 and two_laps >= 1
    first = BR.fastest_lap(ref)[0]
    differ = int((_last_of_equal_times_wins(ref) != first).sum())
    print(f'the fastest-lap driver under "last of equal times wins" differs in {differ} simulations')
    assert differ >= 32 and (first != BR.NONE).all()


def test_ties_of_the_fastest_lap():
    """X_no_noise (no lap-time noise: equal cars set equal times), 64 simulations: 63 have the fastest time shared by two
    drivers, 1 by two laps; an observer with <=, or one that walked the cars by index, gives another driver."""
    case = G.fuzz_cases()['X_no_noise']
    assert_ties_of_the_fastest_lap(case, 64, case['seed'], 3)
    _compare_race(case, 64, case['seed'], sim_offset=3)


# ---------------------------------------------------------------- champ_bonus behind champ_accumulate
def _perms(rng, sims, n):
    return rng.permuted(np.tile(np.arange(n, dtype=np.uint8), (sims, 1)), axis=1)


def _random_races(rng, R, sims, n, none_rate=0.1):
    """Race dicts as championship_bonus_ref.race gives them, from random orders and random fastest-lap drivers."""
    races = []
    for _ in range(R):
        orders = _perms(rng, sims, n)
        d = rng.integers(0, n, sims)
        d[rng.random(sims) < none_rate] = BR.NONE
        pos = np.where(d >= 0, (orders.astype(np.int64) == d[:, None]).argmax(axis=1), BR.NONE)
        races.append(dict(orders=orders, fl_driver=d, fl_pos=pos, fl_retired=np.zeros(sims, bool)))
    return races


def _compare_keys(races, tables, cb, team, T, bonus, within, ip=None, ic=None, **kw):
    n = races[0]['orders'].shape[1]
    sims = races[0]['orders'].shape[0]
    fd, fp = FH.bytes_of(races)
    out = FH.bonus_run([r['orders'] for r in races], tables, cb, team, T, bonus, within, fd, fp, ip, ic, **kw)
    ref = BR.season(races, tables, cb, team, T, bonus, within, ip, ic, by_round=False)
    cap = out['keys'].shape[2]
    last = sims - (sims - 1) // cap * cap                           # the simulations of the last chunk
    pts, cnt = FH.decode_keys(out['keys'][:, :, :last], n)
    want_pts, want_cnt = ref['final']
    assert np.array_equal(pts, want_pts[sims - last:]) and np.array_equal(cnt, want_cnt[sims - last:])
    assert np.array_equal(out['bonus_hist'], ref['bonus_hist']) and np.array_equal(out['fastest_hist'], ref['fastest_hist'])
    assert out['info']['gain_cols'] == ref['gain_hist'].shape[1]
    return out, ref


@pytest.mark.parametrize('n', [1, 2, 9, 10, 11, 12, 20, 22, 23, 24, 25, 32])
def test_every_key_field_at_the_layout_limits(n):
    """Every driver carries in 0x7FFF - (22 .. 39) points: the tables (15 at most) and race 0's bonus of 7 never reach
    bit 15 of the points field, race 2's bonus of 40 always carries across it; at n = 10, 11, 12 and 23, 24, 25 the
    field straddles a word and the carry leaves the word."""
    rng = np.random.default_rng(n)
    R, sims = 3, 300
    tables = [[5, 3, 1][:n]] * R
    bonus, within = [7, 0, 40], [max(1, n // 2), 1, n]
    ip = 0x7FFF - rng.integers(22, 40, n)
    ic = rng.integers(0, 31 - R + 1, (n, n))
    team = [i % min(n, 3) for i in range(n)]
    races = _random_races(rng, R, sims, n)
    out, ref = _compare_keys(races, tables, [1, 0, 1], team, min(n, 3), bonus, within, ip, ic, acc_grid=1)
    pts = ref['final'][0]
    took = np.zeros((sims, n), bool)
    hit = np.nonzero(races[2]['fl_driver'] >= 0)[0]
    took[hit, races[2]['fl_driver'][hit]] = True
    assert took.any() and not took.all() and np.array_equal(pts > 0x7FFF, took)
    assert (ref['bonus_hist'][1] == 0).all() and (ref['fastest_hist'][1] == 0).all()          # the race without a bonus
    if n > 1:
        assert (ref['bonus_hist'][0] < ref['fastest_hist'][0]).any()                           # some outside the limit
    assert np.array_equal(ref['bonus_hist'][2], ref['fastest_hist'][2])                        # within = n: all inside
    assert out['info']['words'] == (16 + 5 * n + 63) // 64


@pytest.mark.parametrize('n', CC.POINTS_STRADDLE)
def test_a_total_of_exactly_65535_and_one_point_more(n):
    rng = np.random.default_rng(40 + n)
    races = _random_races(rng, 2, 100, n, none_rate=0.0)
    for r in races:                                                 # driver 0 wins both races and sets both fastest laps
        r['orders'][:] = np.arange(n, dtype=np.uint8)
        r['fl_driver'][:] = 0
        r['fl_pos'][:] = 0
    tables, bonus = [[25, 18], [25, 18]], [1, 2]
    ip = np.zeros(n, np.int64)
    ip[0] = 65535 - 50 - 3
    out, ref = _compare_keys(races, tables, [1, 1], list(range(n)), n, bonus, [n, n], ip)
    assert (ref['final'][0][:, 0] == 65535).all()
    ip[0] += 1
    fd, fp = FH.bytes_of(races)
    rc, err = FH.bonus_run([r['orders'] for r in races], tables, [1, 1], list(range(n)), n, bonus, [n, n], fd, fp, ip,
                           expect_rc=-1)
    assert rc == -1 and '65535' in err


def test_grid_stride_chunks_and_accumulation():
    """700 simulations: 3 tiles on one block and on two; through a key buffer of 300 (three chunks, the last of 100);
    two runs into the same histograms."""
    n, R = 11, 4
    rng = np.random.default_rng(5)
    races = _random_races(rng, R, 700, n)
    args = ([[10, 6, 4, 3, 2, 1]] * R, [1, 1, 0, 1], [i // 2 for i in range(n)], 6, [1, 2, 0, 3], [3, 10, 5, 1])
    one, _ = _compare_keys(races, *args, acc_grid=1)
    two, _ = _compare_keys(races, *args, acc_grid=2)
    chunks, _ = _compare_keys(races, *args, cap=300)
    for k in ('bonus_hist', 'fastest_hist'):
        assert np.array_equal(one[k], two[k]) and np.array_equal(one[k], chunks[k])
    assert np.array_equal(one['keys'], two['keys'])
    fd, fp = FH.bytes_of(races)
    again = FH.bonus_run([r['orders'] for r in races], *args, fd, fp, into=one)
    assert np.array_equal(again['bonus_hist'], 2 * two['bonus_hist'])


def test_oracle_season_with_the_rule():
    """S60 under seeds 1, 2, 3, bonus 1 within 10 and within 3: the oracle's fastest laps through the kernels."""
    case = O.load_case('S60')
    races = [BR.race(case, 256, s) for s in (1, 2, 3)]
    team, T = CC.team_of(dict(case=case))
    F1 = [25, 18, 15, 12, 10, 8, 6, 4, 2, 1]
    for within in (10, 3):
        _, ref = _compare_keys(races, [F1] * 3, [1] * 3, team, T, [1] * 3, [within] * 3)
        outside = int((ref['fastest_hist'] - ref['bonus_hist']).sum())
        assert outside == (2 if within == 10 else 67)


def test_bad_bonus_arguments():
    n = 4
    rng = np.random.default_rng(1)
    races = _random_races(rng, 1, 10, n)
    fd, fp = FH.bytes_of(races)
    run = lambda b, w: FH.bonus_run([races[0]['orders']], [[3, 2, 1]], [1], [0, 0, 1, 1], 2, [b], [w], fd, fp, expect_rc=-1)
    assert 'bonus_points' in run(-1, 1)[1] and 'bonus_points' in run(65536, 1)[1]
    assert 'bonus_within' in run(1, 0)[1] and 'bonus_within' in run(1, n + 1)[1]
