"""Championship semantics restated in numpy / Python, independently of the device's packed standing keys.

TEST INFRASTRUCTURE.  Input: R finishing-order arrays ([sims][n], driver index classified p-th), one points table per
race (positions past the table score 0), countback flags (1 = Grand Prix, 0 = sprint: scores, no tie-break), initial
standings (points [n], countback counts [n][n]) and a team index per driver.  Ranking: the Python sort key
(-points, -count of P1, ..., -count of Pn, index).
"""
import numpy as np


def standings(orders_list, points_list, countback, init_points=None, init_counts=None):
    """Per simulation: points [sims][n] and countback counts [sims][n][n] after the races."""
    sims, n = orders_list[0].shape
    pts = np.zeros((sims, n), np.int64)
    cnt = np.zeros((sims, n, n), np.int64)
    if init_points is not None:
        pts += np.asarray(init_points, np.int64)[None, :]
    if init_counts is not None:
        cnt += np.asarray(init_counts, np.int64)[None, :, :]
    rows = np.arange(sims)
    for orders, table, cb in zip(orders_list, points_list, countback):
        orders = np.asarray(orders).astype(np.int64)
        assert orders.shape == (sims, n)
        for p in range(n):
            d = orders[:, p]
            if p < len(table):
                pts[rows, d] += int(table[p])
            if cb:
                cnt[rows, d, p] += 1
    return pts, cnt


def team_standings(pts, cnt, team, n_teams):
    """Team points [sims][T] and counts [sims][T][n]: sums over the team's drivers."""
    sims, n = pts.shape
    tp = np.zeros((sims, n_teams), np.int64)
    tc = np.zeros((sims, n_teams, n), np.int64)
    for d in range(n):
        tp[:, team[d]] += pts[:, d]
        tc[:, team[d], :] += cnt[:, d, :]
    return tp, tc


def _key(p, c, i):
    return (-int(p),) + tuple(-int(x) for x in c) + (i,)


def rank_one(p, c):
    """Positions (0-based) of one simulation's entrants: sorted by the Python key."""
    m = len(p)
    order = sorted(range(m), key=lambda i: _key(p[i], c[i], i))
    pos = np.empty(m, np.int64)
    pos[order] = np.arange(m)
    return pos


def rank(pts, cnt):
    """Positions [sims][m] of every simulation: one Python sort per simulation."""
    return np.array([rank_one(pts[s], cnt[s]) for s in range(pts.shape[0])], np.int64).reshape(pts.shape)


def rank_grouped(pts, cnt, block=1 << 15):
    """Same positions as rank(), for many simulations: the distinct (points, counts) vectors of a block are ordered by
    the same Python key (without the index), then a simulation's entrants are placed by that order and, on equal
    vectors, by index."""
    sims, m = pts.shape
    out = np.empty((sims, m), np.int64)
    for s0 in range(0, sims, block):
        p, c = pts[s0:s0 + block], cnt[s0:s0 + block]
        rows = np.concatenate([p[:, :, None], c], axis=2).reshape(-1, 1 + c.shape[2])
        uniq, inv = np.unique(rows, axis=0, return_inverse=True)
        order = sorted(range(len(uniq)), key=lambda i: tuple(-int(x) for x in uniq[i]))
        g = np.empty(len(uniq), np.int64)
        g[order] = np.arange(len(uniq))
        gs = g[inv.reshape(-1)].reshape(p.shape[0], m)                  # smaller = better
        better = gs[:, None, :] < gs[:, :, None]                        # [s][d][e]: e ranks above d
        tie_lower = (gs[:, None, :] == gs[:, :, None]) & np.tri(m, m, -1, bool)[None]
        out[s0:s0 + block] = better.sum(axis=2) + tie_lower.sum(axis=2)
    return out


def rank_lexsort(pts, cnt):
    """Same positions as rank(), for many simulations at wide fields: one numpy lexsort of the unpacked fields (the
    simulation, then fewer points, fewer P1s, ..., then the index)."""
    sims, m = pts.shape
    keys = [np.tile(np.arange(m), sims)]
    keys += [-cnt[:, :, p].reshape(-1) for p in range(cnt.shape[2] - 1, -1, -1)]
    keys += [-pts.reshape(-1), np.repeat(np.arange(sims), m)]
    order = np.lexsort(keys)                                            # the last key is the primary one
    pos = np.empty(sims * m, np.int64)
    pos[order] = np.tile(np.arange(m), sims)
    return pos.reshape(sims, m)


def histogram(pos, m):
    """counts[entrant][position] of positions [sims][m]."""
    h = np.zeros((m, m), np.int64)
    for d in range(m):
        h[d] = np.bincount(pos[:, d], minlength=m)[:m]
    return h


def race_histogram(orders):
    sims, n = orders.shape
    h = np.zeros((n, n), np.int64)
    for p in range(n):
        h[:, p] = np.bincount(orders[:, p].astype(np.int64), minlength=n)[:n]
    return h


def championship(orders_list, points_list, countback, team, n_teams, init_points=None, init_counts=None, grouped=False):
    """champ_hist [n][n], team_hist [T][T], gain_hist [n][G + 1], race_hist [R][n][n] of the races' orders."""
    n = orders_list[0].shape[1]
    pts, cnt = standings(orders_list, points_list, countback, init_points, init_counts)
    tp, tc = team_standings(pts, cnt, team, n_teams)
    rk = {False: rank, True: rank_grouped, 'lexsort': rank_lexsort}[grouped]
    champ = histogram(rk(pts, cnt), n)
    teams = histogram(rk(tp, tc), n_teams)
    G = sum(max([int(x) for x in t[:n]] + [0]) for t in points_list)
    gain = pts - (np.asarray(init_points, np.int64)[None, :] if init_points is not None else 0)
    gain_hist = np.zeros((n, G + 1), np.int64)
    for d in range(n):
        gain_hist[d] = np.bincount(gain[:, d], minlength=G + 1)[:G + 1]
    races = np.array([race_histogram(o) for o in orders_list])
    return champ, teams, gain_hist, races


def decision_depth(pts, cnt, pos=None):
    """How deep the ranking had to look: depth[k] = the number of pairs of entrants adjacent in the final ranking (over
    all simulations) that are first told apart at field k, where field 0 is the points, field 1 + p the count of
    position p + 1, and field 1 + (number of count fields) the index (every field equal).  Length 2 + cnt.shape[2]."""
    sims, m = pts.shape
    if pos is None:
        pos = rank(pts, cnt)
    fields = np.concatenate([pts[:, :, None], cnt], axis=2)              # [s][entrant][field]
    order = np.argsort(pos, axis=1)                                     # [s][rank] = entrant
    ranked = np.take_along_axis(fields, order[:, :, None], axis=1)
    diff = ranked[:, :-1, :] != ranked[:, 1:, :]                        # [s][pair][field]
    first = np.where(diff.any(axis=2), diff.argmax(axis=2), fields.shape[2])
    return np.bincount(first.reshape(-1), minlength=fields.shape[2] + 1)
