"""The fastest-lap bonus of mcgp_run_championship_bonus (include/mcgp.h) restated in numpy on top of championship_ref and
championship_rounds_ref, from the CPU oracle's per-lap trace (resume_ref.traced_run).  No packed keys, no code shared
with the kernels.

TEST INFRASTRUCTURE.  fastest_lap(ref) gives, per simulation, the fastest-lap driver and that driver's position in the
oracle's finishing order; season() turns R races' orders and fastest laps into every count the entry point returns.

Fastest lap: the smallest last lap time of a car running after lap k, over laps 2..L; strict <, laps in order, cars in
running order (cumulative time, grid slot), so ties go to the earlier lap, then to the better running position.  A race
without a completed lap >= 2 has none (-1).
"""
import numpy as np

import championship_ref as CR
import championship_rounds_ref as RR
import resume_ref as RS

NONE = -1


def fastest_lap_loop(ref):
    """(driver [m], classified position [m] 0-based, retired_later [m] bool) of a traced oracle run; -1 / -1 / False for
    a simulation without a fastest lap.  A plain loop over simulations, laps and running order: the definition, slow."""
    tr, grids, orders = ref['trace'], ref['grids'], ref['orders']
    m, L, n = tr['cum'].shape
    driver = np.full(m, NONE, np.int64)
    pos = np.full(m, NONE, np.int64)
    retired = np.zeros(m, bool)
    for i in range(m):
        slot = np.empty(n, np.int64)
        slot[grids[i]] = np.arange(n)
        best, best_d = np.inf, NONE
        for k in range(1, L):                                   # after lap k + 1 = 2 .. L
            running = [d for d in range(n) if tr['dnf'][i, k, d] == 0]
            running.sort(key=lambda d: (tr['cum'][i, k, d], slot[d]))
            for d in running:
                t = tr['last'][i, k, d]
                if t < best:
                    best, best_d = t, d
        if best_d != NONE:
            driver[i] = best_d
            pos[i] = int(np.nonzero(orders[i] == best_d)[0][0])
            retired[i] = tr['dnf'][i, L - 1, best_d] != 0
    return driver, pos, retired


def fastest_lap(ref):
    """fastest_lap_loop's result, a lap at a time over all simulations (tests/test_championship_bonus_ref.py holds the two
    together)."""
    tr, grids, orders = ref['trace'], ref['grids'], ref['orders']
    m, L, n = tr['cum'].shape
    rows = np.arange(m)
    slot = np.zeros((m, n), np.int64)
    slot[rows[:, None], grids] = np.arange(n)[None, :]
    best = np.full(m, np.inf)
    driver = np.full(m, NONE, np.int64)
    for k in range(1, L):
        order = np.lexsort((slot, tr['cum'][:, k, :]), axis=-1)         # running order: (cumulative time, grid slot)
        t = np.where(np.take_along_axis(tr['dnf'][:, k, :], order, axis=1) == 0,
                     np.take_along_axis(tr['last'][:, k, :], order, axis=1), np.inf)
        j = np.argmin(t, axis=1)                                        # the first of equal times: the better position
        better = t[rows, j] < best
        best = np.where(better, t[rows, j], best)
        driver = np.where(better, order[rows, j], driver)
    has = driver != NONE
    pos = np.where(has, (orders.astype(np.int64) == driver[:, None]).argmax(axis=1), NONE)
    retired = has & (tr['dnf'][rows, L - 1, np.where(has, driver, 0)] != 0)
    return driver, pos, retired


def race(case, m, seed, sim_offset=0):
    """dict(orders [m][n] u8, fl_driver [m], fl_pos [m], fl_retired [m]) of the oracle's simulations of a case."""
    ref = RS.traced_run(case, m, seed, sim_offset)
    d, p, ret = fastest_lap(ref)
    return dict(orders=ref['orders'], fl_driver=d, fl_pos=p, fl_retired=ret)


def takes_bonus(r, points, within):
    """[m] bool: the simulations in which race dict r's fastest-lap driver takes a bonus of `points` within `within`."""
    if points <= 0:
        return np.zeros(len(r['fl_driver']), bool)
    return (r['fl_driver'] != NONE) & (r['fl_pos'] < within)


def bonus_matrix(races, bonus_points, bonus_within):
    """[R][m][n] int64: the bonus points every driver takes in every race and simulation."""
    m, n = races[0]['orders'].shape
    out = np.zeros((len(races), m, n), np.int64)
    for q, r in enumerate(races):
        hit = np.nonzero(takes_bonus(r, bonus_points[q], bonus_within[q]))[0]
        out[q, hit, r['fl_driver'][hit]] = bonus_points[q]
    return out


def standings_after(races, upto, points_list, countback, bonus, init_points, init_counts):
    """Points [m][n] and counts [m][n][n] after races 0..upto: championship_ref's, plus the bonuses (points only)."""
    pts, cnt = CR.standings([r['orders'] for r in races[:upto + 1]], points_list[:upto + 1], countback[:upto + 1],
                            init_points, init_counts)
    return pts + bonus[:upto + 1].sum(axis=0), cnt


def remaining(points_list, n, team, n_teams, bonus_points):
    """(M [R], B [R][T]) with the bonuses still to come: each adds the sum over q > r of bonus_points[q] (at most one car
    of a team takes a race's bonus; a team without drivers can take nothing)."""
    M, B = RR.remaining(points_list, n, team, n_teams)
    size = np.bincount(np.asarray(team, np.int64), minlength=n_teams)
    later = np.array([sum(int(b) for b in bonus_points[r + 1:]) for r in range(len(points_list))], np.int64)
    return M + later, B + later[:, None] * (size > 0)[None, :]


def season(races, points_list, countback, team, n_teams, bonus_points, bonus_within, init_points=None, init_counts=None,
           by_round=True):
    """Every count of mcgp_run_championship_bonus: champ_hist, team_hist, gain_hist, race_hist, bonus_hist [R][n],
    fastest_hist [R][n] (rows of races without a bonus zero) and, by round, championship_rounds_ref's six arrays;
    'per' = the per-round per-simulation views (championship_rounds_ref.per_simulation's keys), 'final' = (pts, cnt)."""
    R = len(races)
    m, n = races[0]['orders'].shape
    bonus = bonus_matrix(races, bonus_points, bonus_within)
    pts, cnt = standings_after(races, R - 1, points_list, countback, bonus, init_points, init_counts)
    tp, tc = CR.team_standings(pts, cnt, team, n_teams)
    out = dict(champ_hist=CR.histogram(CR.rank_lexsort(pts, cnt), n), team_hist=CR.histogram(CR.rank_lexsort(tp, tc), n_teams))
    G = sum(max([int(x) for x in t[:n]] + [0]) for t in points_list) + sum(int(b) for b in bonus_points)
    gain = pts - (np.asarray(init_points, np.int64)[None, :] if init_points is not None else 0)
    assert gain.min() >= 0 and gain.max() <= G
    out['gain_hist'] = np.array([np.bincount(gain[:, d], minlength=G + 1) for d in range(n)], np.int64)
    out['race_hist'] = np.array([CR.race_histogram(r['orders']) for r in races])
    out['bonus_hist'] = np.zeros((R, n), np.int64)
    out['fastest_hist'] = np.zeros((R, n), np.int64)
    for q, r in enumerate(races):
        if bonus_points[q] > 0:
            d = r['fl_driver']
            out['fastest_hist'][q] = np.bincount(d[d != NONE], minlength=n)
            out['bonus_hist'][q] = (bonus[q] > 0).sum(axis=0)
    out['final'] = (pts, cnt)
    if by_round:
        M, B = remaining(points_list, n, team, n_teams, bonus_points)
        per = []
        for r in range(R):
            p, c = standings_after(races, r, points_list, countback, bonus, init_points, init_counts)
            tpr, tcr = CR.team_standings(p, c, team, n_teams)
            pos, con, sec = RR._round(p, c, M[r], r == R - 1)
            tpos, tcon, tsec = RR._round(tpr, tcr, B[r], r == R - 1)
            per.append(dict(pts=p, cnt=c, tp=tpr, tc=tcr, pos=pos, contend=con, secure=sec, tpos=tpos, tcontend=tcon,
                            tsecure=tsec, M=int(M[r]), B=B[r]))
        out.update(RR.rounds([r['orders'] for r in races], points_list, countback, team, n_teams, sims=per))
        out['per'] = per
    return out


SEASON_KEYS = ('champ_hist', 'team_hist', 'gain_hist', 'race_hist')
BONUS_KEYS = ('bonus_hist', 'fastest_hist')


def changed_by_the_bonus(races, points_list, countback, team, n_teams, bonus_points, bonus_within, init_points=None,
                        init_counts=None):
    """dict(champions, standings, champ_cells): simulations whose champion changes with the bonus, simulations in which
    some standings position changes, cells of champ_hist that change."""
    with_b = season(races, points_list, countback, team, n_teams, bonus_points, bonus_within, init_points, init_counts, False)
    zero = season(races, points_list, countback, team, n_teams, [0] * len(races), bonus_within, init_points, init_counts, False)
    pa, pb = CR.rank_lexsort(*with_b['final']), CR.rank_lexsort(*zero['final'])
    return dict(champions=int(((pa == 0) != (pb == 0)).any(axis=1).sum()), standings=int((pa != pb).any(axis=1).sum()),
                champ_cells=int((with_b['champ_hist'] != zero['champ_hist']).sum()))
