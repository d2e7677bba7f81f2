"""champ_round run from its source on the host (tools/emu/emu_champ.cpp: blocks of 256 real threads, the library's own
key layout and remaining-points tables from csrc/champ_pack.h) behind champ_accumulate after every race, against
championship_rounds_ref: every count of every round equal."""
import numpy as np
import pytest

import champ_rounds_host_build as H
import championship_cases as CC
import championship_rounds_ref as RR

SHORT = CC.SHORT
ALL_N = list(range(1, 33))


def _perms(rng, sims, n):
    return rng.permuted(np.tile(np.arange(n, dtype=np.uint8), (sims, 1)), axis=1)


def _compare(orders, tables, cb, team, T, ip=None, ic=None, per=None, **kw):
    """The host build against the restatement; returns (the host build's output, the reference's per-simulation view).
    per: the reference's view of these very arguments, when the caller has it."""
    sims, n = orders[0].shape
    out = H.rounds_run(orders, tables, cb, team, T, ip, ic, **kw)
    per = per or RR.per_simulation(orders, tables, [int(c) for c in cb], team, T, ip, ic)
    ref = RR.rounds(orders, tables, cb, team, T, sims=per)
    M, B = RR.remaining(tables, n, team, T)
    assert np.array_equal(out['rem'][0], M) and np.array_equal(out['rem'][1], B)
    for k in RR.KEYS:
        if out[k] is None:
            assert k.startswith('team_') and kw.get('teams') is False
        else:
            assert np.array_equal(out[k], ref[k]), k
    if out['team_secure'] is not None:
        RR.assert_identities(out, sims)
    return out, per


def _season_args(season):
    team, T = CC.team_of(season)
    ip, ic = CC.standings_arrays(season)
    return [p[3] for p in season['plan']], [int(p[4]) for p in season['plan']], team, T, ip, ic


@pytest.mark.parametrize('n', ALL_N)
def test_tie_rich_seasons(n):
    """The oracle's orders of the tie-rich season: equal carried-in totals and a short table, so that the leader is
    found in every field of the key and many drivers sit on or next to the bound; 8 tiles on three blocks."""
    season = CC.tie_rich(n)
    _, per = _compare(CC.oracle_orders(season), *_season_args(season), acc_grid=1, round_grid=3)
    if n >= 4:
        e = RR.edges(per, 500)
        assert e['driver_on_bound'] > 0, e


@pytest.mark.parametrize('n', CC.POINTS_STRADDLE)
def test_random_permutations_at_the_straddling_sizes(n):
    """Uniformly random orders with the tie-rich standings where the points field is read in two pieces, carried-in
    totals spread so that drivers fall on both sides of the bound; 11 tiles on one block and on three."""
    rng = np.random.default_rng(200 + n)
    season = CC.tie_rich(n)
    tables, cb, team, T, ip, ic = _season_args(season)
    ip = ip - rng.integers(0, 12, n)
    orders = [_perms(rng, 700, n) for _ in season['plan']]
    low = CC.points_low_bits(n)
    one, per = _compare(orders, tables, cb, team, T, ip, ic, round_grid=1)
    lows = np.concatenate([s['pts'].reshape(-1) for s in per]) & ((1 << low) - 1)
    assert (lows < 8).any() and (lows > (1 << low) - 8).any()           # the lower piece just after and just before a carry
    assert 0 < per[1]['contend'].sum() < 700 * n                      # some in, some out
    three, _ = _compare(orders, tables, cb, team, T, ip, ic, acc_grid=2, round_grid=3)
    for k in RR.KEYS:
        assert np.array_equal(one[k], three[k])


@pytest.mark.parametrize('name', ['one_team_32', 'singletons_32', 'six_words', 'pairs_20', 'one_team_20', 'singletons_9'])
def test_wide_team_keys(name):
    """One team of all n (T = 1: it is secure from row 0), T = n, and the six-word layout, whose team points field
    lies above 320 bits of counts."""
    season, words = CC.team_seasons()[name]
    args = _season_args(season)
    out, _ = _compare(CC.oracle_orders(season), *args, round_grid=2)
    assert out['info']['team_words'] == words
    if args[3] == 1:
        assert (out['team_secure'] == season['n_sims']).all() and (out['team_contend'] == season['n_sims']).all()
    rng = np.random.default_rng(len(name))
    _compare([_perms(rng, 200, len(args[2])) for _ in season['plan']], *args)


@pytest.mark.parametrize('tail', [1, 6, 63])
@pytest.mark.parametrize('n', [3, 12, 23])
def test_last_tile(n, tail):
    """A last tile of 1, 6 and 63 simulations behind a full one, and alone."""
    rng = np.random.default_rng(n + tail)
    args = _season_args(CC.tie_rich(n))
    for sims in (64 + tail, tail):
        _compare([_perms(rng, sims, n) for _ in range(5)], *args)


@pytest.mark.parametrize('grid', [1, 2, 3])
def test_grid_stride_and_histogram_reuse(grid):
    """9 tiles (540 simulations) on grids of 1, 2 and 3 blocks, through a key buffer of 300: two chunks."""
    n = 11
    rng = np.random.default_rng(77)
    tables, cb, team, T, ip, ic = _season_args(CC.tie_rich(n))
    ip = ip - rng.integers(0, 9, n)
    orders = [_perms(rng, 540, n) for _ in range(5)]
    whole, _ = _compare(orders, tables, cb, team, T, ip, ic)
    parts, _ = _compare(orders, tables, cb, team, T, ip, ic, round_grid=grid, cap=300)
    for k in RR.KEYS:
        assert np.array_equal(whole[k], parts[k])


def test_two_runs_accumulate_and_drivers_only():
    n = 7
    rng = np.random.default_rng(3)
    tables, cb, team, T, ip, ic = _season_args(CC.tie_rich(n))
    orders = [_perms(rng, 150, n) for _ in range(5)]
    a, _ = _compare(orders, tables, cb, team, T, ip, ic)
    b = H.rounds_run(orders, tables, cb, team, T, ip, ic, into=a)
    for k in RR.KEYS:
        assert np.array_equal(b[k], 2 * a[k])
    c, _ = _compare(orders, tables, cb, team, T, ip, ic, teams=False)
    assert c['team_round_hist'] is None and np.array_equal(c['secure'], a['secure'])


@pytest.mark.parametrize('n', [1, 2, 10, 32])
def test_one_race(n):
    """R = 1: the only row is the last one, where only the leader is in contention."""
    rng = np.random.default_rng(n)
    team = [i % 3 for i in range(n)]
    out, _ = _compare([_perms(rng, 100, n)], [SHORT], [1], team, min(n, 3), rng.integers(0, 3, n), None)
    assert out['secure'].sum() == 100 and np.array_equal(out['secure'], out['contend'])


def test_one_driver_is_secure_from_row_0():
    orders = [np.zeros((70, 1), np.uint8)] * 4
    out, _ = _compare(orders, [SHORT] * 4, [1, 1, 0, 1], [0], 1)
    for k in ('contend', 'secure', 'team_contend', 'team_secure'):
        assert (out[k] == 70).all() and out[k].shape == (4, 1)


def test_initial_standings_that_already_secure_the_title():
    """Driver 2 carries in 13 points more than anybody can still take after race 0 (4 races x 3 = 12 remain), so the
    title is secure in row 0 whatever happens; with 12 it is not (the bound is inclusive)."""
    n = 5
    rng = np.random.default_rng(9)
    orders = [_perms(rng, 200, n) for _ in range(5)]
    orders[0][:, :] = [0, 1, 3, 4, 2]                                   # driver 2 scores nothing in race 0, driver 0 wins it
    team = [0, 0, 1, 1, 2]
    out, _ = _compare(orders, [SHORT] * 5, [1] * 5, team, 3, [0, 0, 3 + 13, 0, 0], None)
    assert (out['secure'][:, 2] == 200).all() and out['secure'].sum() == 5 * 200
    assert (out['contend'][:, [0, 1, 3, 4]] == 0).all()
    out, _ = _compare(orders, [SHORT] * 5, [1] * 5, team, 3, [0, 0, 3 + 12, 0, 0], None)
    assert out['secure'][0].sum() == 0 and out['contend'][0, 0] == 200 and out['contend'][0, 1] == 0


def known_decisive_season():
    """6 drivers, 7 races, 400 simulations: orders drawn without replacement with weights 6:3:2:1:1:1, five short Grands
    Prix, a two-place sprint, a last Grand Prix; three teams of two; driver 0 carries in 4 points, driver 3 two."""
    rng = np.random.default_rng(5)
    w = np.array([6, 3, 2, 1, 1, 1], np.float64)
    w /= w.sum()
    orders = [np.array([rng.choice(6, 6, replace=False, p=w) for _ in range(400)], np.uint8) for _ in range(7)]
    return orders, [[3, 2, 1]] * 5 + [[2, 1]] + [[3, 2, 1]], [1] * 5 + [0, 1], [0, 1, 0, 1, 2, 2], 3, [4, 0, 0, 2, 0, 0]


def test_decisive_season():
    """A season that is decided at different rounds: the reference alone proves that it has partly decided rounds,
    non-leaders exactly on the bound (so that <= is told from <) among drivers and teams, final ties on points, and a
    sprint with a shorter table."""
    orders, tables, cb, team, T, ip = known_decisive_season()
    per = RR.per_simulation(orders, tables, cb, team, T, ip)
    e = RR.assert_decisive(per, 400, tables, cb)
    assert (e['driver_on_bound'], e['team_on_bound'], e['final_points_ties']) == (525, 129, 5)
    assert [int(s['secure'].sum()) for s in per] == [0, 0, 0, 57, 233, 326, 400]
    _compare(orders, tables, cb, team, T, ip, None, round_grid=2)


# ---------------------------------------------------------------- the limit seasons of championship_cases.py, by round
# (what tests/test_gpu_championship_rounds_limits.py runs on the device: the same seasons, after the same proofs)
def _limit_season(season, per):
    """The season on the oracle's orders on one block and on three; the restated LDS size is the kernel's."""
    args = CC.season_args(season)
    outs = [_compare(CC.oracle_orders(season), *args, per=per, round_grid=g)[0] for g in (1, 3)]
    n, T = len(args[2]), args[3]
    assert outs[0]['info']['lds_bytes'] == CC.round_lds_bytes(n, T, outs[0]['info']['team_words'])
    assert outs[0]['info']['team_words'] == CC.team_layout(season)[1]
    return outs[0]


def test_uneven_team_bounds():
    """Teams of 3, 2, 1 and 1: every team is tested against its own B_r(e), where the leader's, the largest and the
    smallest bound of the round each decide hundreds of cells differently."""
    season = CC.uneven_teams()
    per = CC.reference_rounds(season)
    CC.assert_uneven_team_edges(per)
    out = _limit_season(season, per)
    assert [list(b) for b in out['rem'][1][[0, 4]]] == [[43, 35, 22, 22], [3, 3, 2, 2]]


@pytest.mark.parametrize('n', [20, 32])
def test_procession_duel_at_the_points_limit(n):
    """A leader that ends on 65 535 points and a rival exactly on the bound in row 20, out in row 21: lead - points
    between two points fields with bit 15 set."""
    season = CC.procession_duel(n)
    per = CC.reference_rounds(season)
    CC.assert_duel_edges(per)
    out = _limit_season(season, per)
    assert (out['contend'][:21, 1] >= 100).all() and (out['contend'][21:, 1] <= 100).all()


def test_calendar_of_64_races_by_round():
    """64 launches and 64 rows of every output, 31 races that count back."""
    season = CC.long_calendar()
    per = CC.reference_rounds(season)
    CC.assert_long_calendar_rounds(per, season['n_sims'])
    out = _limit_season(season, per)
    assert out['round_hist'].shape[0] == 64 and (np.diff(out['secure'], axis=0) >= 0).all()


@pytest.mark.parametrize('name', ['pairs_32', 'uneven_pairs_20', 'quads_27'])
def test_team_points_field_by_round(name):
    """The team seasons that test_wide_team_keys leaves out, each after the by-round proof: the leading team's total
    needs the top bit of a 17- or 18-bit points field that starts above 120 to 192 bits of counts."""
    season, _ = CC.team_seasons()[name]
    per = CC.reference_rounds(season)
    CC.assert_team_round_edges(name, season, per)
    _limit_season(season, per)


def test_team_points_borrow_across_bit_16_and_a_word():
    """Rival teams just below 2^16 under a leader just above it, within the bound: lead - points borrows across bit 16
    of the team points field and across the word boundary inside it.  A field read with 16 bits, or from its lower
    word alone, gives another difference here and in no other season."""
    season = CC.team_points_borrow()
    per = CC.reference_rounds(season)
    CC.assert_team_borrow_edges(season, per)
    _limit_season(season, per)
