"""champ_accumulate and champ_rank run from their source on the host (tools/emu/emu_champ.cpp: blocks of 256 real
threads, the library's own key layout from csrc/champ_pack.h) against championship_ref, on finishing orders made for
the purpose: every histogram equal count for count, and every field of every final driver key, decoded here with Python
integers, equal to the restated points and counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import championship_cases as CC
import championship_ref as CR
import kernel_host_build as K

F1, SHORT = CC.F1, CC.SHORT
ALL_N = list(range(1, 33))


def _perms(rng, sims, n):
    return rng.permuted(np.tile(np.arange(n, dtype=np.uint8), (sims, 1)), axis=1)


def _decode(keys, n, sims):
    """(points [s][n], counts [s][n][n]) of the kernel's key buffer [words][n][stride], by the documented layout."""
    pts, cnt = np.zeros((sims, n), np.int64), np.zeros((sims, n, n), np.int64)
    for s in range(sims):
        for d in range(n):
            k = sum(int(keys[w, d, s]) << (64 * w) for w in range(keys.shape[0]))
            assert k >> (5 * n + 16) == 0
            pts[s, d] = k >> (5 * n)
            for p in range(n):
                cnt[s, d, p] = (k >> (5 * (n - 1 - p))) & 31
    return pts, cnt


def _compare(orders, tables, cb, team, T, ip=None, ic=None, keys=True, **kw):
    """The host build against the restatement; returns the host build's output."""
    sims, n = orders[0].shape
    out = K.champ_run(orders, tables, cb, team, T, ip, ic, want_keys=keys, **kw)
    champ, teams, gain, _ = CR.championship(orders, tables, [int(c) for c in cb], team, T, init_points=ip, init_counts=ic,
                                            grouped='lexsort')
    assert np.array_equal(out['champ'], champ)
    assert np.array_equal(out['team'], teams)
    assert np.array_equal(out['gain'], gain)
    if keys:
        pts, cnt = CR.standings(orders, tables, cb, ip, ic)
        kp, kc = _decode(out['keys'], n, sims)
        assert np.array_equal(kp, pts) and np.array_equal(kc, cnt)
    return out


def _season_args(season):
    team, T = CC.team_of(season)
    ip, ic = CC.standings_arrays(season)
    return [p[3] for p in season['plan']], [int(p[4]) for p in season['plan']], team, T, ip, ic


@pytest.mark.parametrize('n', ALL_N)
def test_tie_rich_seasons(n):
    """The oracle's orders of the tie-rich season (its edges: test_championship_host.py): carries out of both straddling
    count fields and out of the points field's lower piece, rankings decided in every field; 2 accumulate tiles on one
    block, 8 rank tiles on three."""
    season = CC.tie_rich(n)
    _compare(CC.oracle_orders(season), *_season_args(season), acc_grid=1, rank_grid=3)


@pytest.mark.parametrize('n', ALL_N)
def test_constructed_extremes(n):
    """One driver first in all 31 races from 65 535 - 775 points (a count of 31, a total of 65 535); every driver in
    the same position every race (every count field that is used full, its neighbours empty); a season nobody can tell
    apart (zero tables, no countback: the index decides)."""
    rng = np.random.default_rng(n)
    sims = 70
    team = [i % 10 for i in range(n)]
    T = min(n, 10)
    # sim 0: the same order in every race; the others: driver 0 first, the rest at random
    orders = []
    for _ in range(31):
        o = np.zeros((sims, n), np.uint8)
        o[:, 1:] = 1 + _perms(rng, sims, n - 1)
        o[0] = np.arange(n)
        orders.append(o)
    ip = np.full(n, CC.MAX_POINTS - 31 * 25, np.int64)
    out = _compare(orders, [F1] * 31, [1] * 31, team, T, ip, None)
    pts, cnt = _decode(out['keys'], n, sims)
    assert (cnt[:, 0, 0] == 31).all() and (pts[:, 0] == 65535).all()
    assert np.array_equal(cnt[0], 31 * np.eye(n, dtype=np.int64))
    # nothing to tell anyone apart
    out = _compare([_perms(rng, sims, n) for _ in range(3)], [[0]] * 3, [0] * 3, team, T, np.full(n, 77), np.full((n, n), 5))
    assert np.array_equal(out['champ'], sims * np.eye(n, dtype=np.int64))
    assert np.array_equal(out['team'], sims * np.eye(T, dtype=np.int64))


@pytest.mark.parametrize('n', ALL_N)
def test_random_permutations_with_tie_rich_standings(n):
    """Uniformly random orders, the tie-rich season's standings and tables, 700 seasons: 3 accumulate tiles and 11 rank
    tiles, once on a grid of one block (the LDS histograms live through every tile) and once on three."""
    rng = np.random.default_rng(100 + n)
    season = CC.tie_rich(n)
    args = _season_args(season)
    orders = [_perms(rng, 700, n) for _ in season['plan']]
    pts, cnt = CR.standings(orders, args[0], args[1], args[4], args[5])
    if n >= 13:
        assert (cnt[:, :, n - 13] >= 16).sum() >= 100
    if n >= 26:
        assert (cnt[:, :, n - 26] >= 8).sum() >= 100
    one = _compare(orders, *args, acc_grid=1, rank_grid=1)
    three = _compare(orders, *args, acc_grid=2, rank_grid=3, keys=False)
    for k in ('champ', 'team', 'gain'):
        assert np.array_equal(one[k], three[k])


@pytest.mark.parametrize('name', list(CC.team_seasons()))
def test_team_layouts(name):
    """The team seasons (one team, singletons, pairs, fours, 30 + 1 + 1; 1, 3, 4, 5 and 6 team words): the library's
    layout is the documented rule's, and the team standings equal the restatement on the oracle's orders (whose team
    edges test_championship_host.py proves) and on random ones."""
    season, words = CC.team_seasons()[name]
    args = _season_args(season)
    out = _compare(CC.oracle_orders(season), *args, keys=False, rank_grid=2)
    cbits, tw = CC.team_layout(season)
    assert (out['info']['team_cbits'], out['info']['team_words']) == (cbits, tw) and tw == words
    rng = np.random.default_rng(len(name))
    _compare([_perms(rng, 300, len(args[2])) for _ in season['plan']], *args, keys=False)


@pytest.mark.parametrize('seed', list(range(24)))
def test_random_standings_near_the_bounds(seed):
    """Random field size, teams, calendar, tables and carried-in standings within a few units of what the call's
    limits allow: every field of every key is the restated value (a field one bit too narrow, a carry into a
    neighbour, would show), and team totals that differ in their leading bits rank as the restatement ranks them."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 33))
    T = int(rng.integers(1, n + 1))
    team = rng.integers(0, T, n)
    team[rng.permutation(n)[:T]] = np.arange(T)            # every team has a driver
    R = int(rng.integers(1, 7))
    cb = rng.integers(0, 2, R)
    tables = [sorted((int(x) for x in rng.integers(0, 400, int(rng.integers(1, n + 1)))), reverse=True) for _ in range(R)]
    G = sum(max(t) for t in tables)
    ip = CC.MAX_POINTS - G - rng.integers(0, 3000, n)
    ic = CC.MAX_COUNT - int(cb.sum()) - rng.integers(0, 3, (n, n))
    sims = 130
    out = _compare([_perms(rng, sims, n) for _ in range(R)], tables, cb, team, T, ip, ic)
    pts, cnt = _decode(out['keys'], n, sims)
    assert pts.max() > 60000 and cnt.max() >= 29


@pytest.mark.parametrize('n', [1, 2, 5, 23, 32])
def test_both_gain_paths(n):
    """The same seasons with the gain histogram in LDS and by global atomics; gains of 0 and of G occur.  Then a
    five-figure win, which the library's rule sends to global atomics under any LDS budget."""
    rng = np.random.default_rng(n)
    team = [i % 10 for i in range(n)]
    orders = [_perms(rng, 400, n) for _ in range(2)]
    orders[0][:60] = orders[1][:60] = np.arange(n)           # driver 0 wins both, the last driver scores nothing
    tables, ip = [SHORT, [5, 1]], rng.integers(0, 50, n)
    for path in (0, 1):
        out = _compare(orders, tables, [1, 0], team, min(n, 10), ip, None, gain_in_lds=path, rank_grid=2)
        assert out['info']['gain_in_lds'] == path and out['gain'][0, 8] >= 60 and (n < 3 or out['gain'][n - 1, 0] >= 60)
    wide = [[20000, 2, 1], [20000, 2, 1]]
    for budget in (64 * 1024, 160 * 1024):
        out = _compare(orders, wide, [1, 1], team, min(n, 10), ip + 20000, None, lds_per_block=budget, keys=False)
        assert out['info']['gain_in_lds'] == 0
        assert out['gain'][0, 40000] >= 60
    # the library's rule, restated: in LDS when the block then takes no more than half the budget
    for budget in (64 * 1024, 160 * 1024):
        out = _compare(orders, tables, [1, 0], team, min(n, 10), ip, None, lds_per_block=budget, keys=False)
        need = CC.rank_lds_bytes(n, min(n, 10), out['info']['team_words'], 9, True)
        assert out['info']['gain_in_lds'] == int(need <= budget // 2) and (n > 5 or out['info']['gain_in_lds'] == 1)
        assert out['info']['lds_bytes'] == CC.rank_lds_bytes(n, min(n, 10), out['info']['team_words'], 9,
                                                             bool(out['info']['gain_in_lds']))


def test_chunks_start_from_the_initial_keys_again():
    """517 seasons through a key buffer of 200: three chunks, each starting from the carried-in standings in a buffer
    the chunk before has written (`first` set), the last with fewer simulations than the buffer's stride."""
    n = 23
    rng = np.random.default_rng(5)
    season = CC.tie_rich(n)
    args = _season_args(season)
    orders = [_perms(rng, 517, n) for _ in season['plan']]
    whole = _compare(orders, *args, keys=False)
    parts = _compare(orders, *args, keys=False, cap=200, rank_grid=2)
    for k in ('champ', 'team', 'gain'):
        assert np.array_equal(whole[k], parts[k])
    # the last chunk's keys: simulations 400..516
    out = K.champ_run(orders, *args, cap=200, want_keys=True)
    pts, cnt = CR.standings([o[400:] for o in orders], args[0], args[1], args[4], args[5])
    kp, kc = _decode(out['keys'], n, 117)
    assert np.array_equal(kp, pts) and np.array_equal(kc, cnt)


@pytest.mark.parametrize('n', [9, 23, 31, 32])
def test_byte_tail_of_the_staged_orders(n):
    """Last tiles of 1 to 4 simulations, alone and after a full tile: for an odd n their orders end 1, 2 and 3 bytes
    past a whole word (and on a whole word for n = 32).  Every position scores, so a wrong byte moves points."""
    rng = np.random.default_rng(n)
    team = [i % 10 for i in range(n)]
    table = list(range(n, 0, -1))
    tails = set()
    for sims in (1, 2, 3, 4, 257, 258, 259, 260):
        tails.add(CC.tail_bytes(n, sims))
        _compare([_perms(rng, sims, n) for _ in range(3)], [table] * 3, [1, 1, 0], team, min(n, 10), rng.integers(0, 9, n),
                 None)
    assert tails == ({0, 1, 2, 3} if n % 2 else {0})


UBSAN_CHILD = """
import sys
sys.path[:0] = [{tests!r}, {root!r}]
import numpy as np
import championship_cases as CC
import kernel_host_build as K
import test_champ_host_build as T
rng = np.random.default_rng(8)
for name in ('six_words', 'one_team_32', 'pairs_20', 'singletons_9'):
    season, _ = CC.team_seasons()[name]
    args = T._season_args(season)
    T._compare([T._perms(rng, 150, len(args[2])) for _ in season['plan']], *args, variant='ubsan', rank_grid=2)
for n in (1, 12, 13, 25, 26):
    args = T._season_args(CC.tie_rich(n))
    T._compare([T._perms(rng, 150, n) for _ in range(5)], *args, variant='ubsan', gain_in_lds=n % 2)
print('ran')
"""


def test_the_undefined_behaviour_sanitizer_is_silent():
    """The same comparisons in a build with the host's undefined-behaviour sanitizer (a child process: its reports go
    to stderr): the shifts of champ_piece and champ_field at every kind of layout, with nothing to report."""
    K.build_champ('ubsan')
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, '-c', UBSAN_CHILD.format(tests=here, root=os.path.dirname(here))],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip() == 'ran', r.stderr[-2000:]
    assert 'runtime error' not in r.stderr, r.stderr[-2000:]
