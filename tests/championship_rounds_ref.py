"""The standings after every race of a season (mcgp_run_championship_rounds, include/mcgp.h) restated in numpy on top
of championship_ref: positions, contention and secure titles per round, with no packed keys.

TEST INFRASTRUCTURE.  Inputs as championship_ref takes them: R finishing-order arrays [sims][n], a points table per race
(positions past the table score 0), countback flags, initial standings, a team index per driver.

"After race r" is the initial standings plus races 0..r.  The leader is the entrant in position 0 of the ranking
(points, countback, lower index).  A driver is in contention after race r when it leads or, for r < R - 1, when
lead - points <= M_r, the most a driver can still take; a team when lead - points <= B_r(team), the most its drivers can
still take together.  After the last race only the leader is in contention.  An entrant is secure when it is the only
one in contention.
"""
import numpy as np

import championship_ref as CR


def padded_tables(points_list, n):
    """[R][n]: the tables cut or padded with zeros to n positions."""
    out = np.zeros((len(points_list), n), np.int64)
    for r, t in enumerate(points_list):
        t = [int(x) for x in t][:n]
        out[r, :len(t)] = t
    return out


def remaining(points_list, n, team, n_teams):
    """(M [R], B [R][T]): the points a driver, and each team, can still take after race r."""
    tables = padded_tables(points_list, n)
    R = len(tables)
    size = np.bincount(np.asarray(team, np.int64), minlength=n_teams)
    M, B = np.zeros(R, np.int64), np.zeros((R, n_teams), np.int64)
    for r in range(R):
        for q in range(r + 1, R):
            top = np.sort(tables[q])[::-1]
            M[r] += top[0]
            for e in range(n_teams):
                B[r, e] += top[:size[e]].sum()
    return M, B


def _round(pts, cnt, bound, last):
    """One round of one kind of entrant: (positions [s][m], in contention [s][m] bool, secure [s][m] bool).
    bound: scalar or [m]."""
    pos = CR.rank_lexsort(pts, cnt)
    leader = pos == 0
    lead = (pts * leader).sum(axis=1)
    assert (lead == pts.max(axis=1)).all()                      # the leader has the most points
    inside = leader.copy()
    if not last:
        inside |= (lead[:, None] - pts) <= np.broadcast_to(np.asarray(bound, np.int64), pts.shape[1:])[None, :]
    alone = inside.sum(axis=1) == 1
    return pos, inside, leader & alone[:, None]


def per_simulation(orders_list, points_list, countback, team, n_teams, init_points=None, init_counts=None):
    """Per round r, a dict of per-simulation arrays: pts, cnt, tp, tc (the standings), pos, contend, secure and their
    team counterparts tpos, tcontend, tsecure; M and B (the bounds of the round)."""
    R, n = len(orders_list), orders_list[0].shape[1]
    M, B = remaining(points_list, n, team, n_teams)
    out = []
    for r in range(R):
        pts, cnt = CR.standings(orders_list[:r + 1], points_list[:r + 1], countback[:r + 1], init_points, init_counts)
        tp, tc = CR.team_standings(pts, cnt, team, n_teams)
        pos, con, sec = _round(pts, cnt, M[r], r == R - 1)
        tpos, tcon, tsec = _round(tp, tc, B[r], r == R - 1)
        out.append(dict(pts=pts, cnt=cnt, tp=tp, tc=tc, pos=pos, contend=con, secure=sec, tpos=tpos, tcontend=tcon,
                        tsecure=tsec, M=int(M[r]), B=B[r]))
    return out


def rounds(orders_list, points_list, countback, team, n_teams, init_points=None, init_counts=None, sims=None):
    """dict(round_hist [R][n][n], contend [R][n], secure [R][n], team_round_hist [R][T][T], team_contend [R][T],
    team_secure [R][T]) of the races' orders.  sims: per_simulation's result, when the caller has it."""
    n = orders_list[0].shape[1]
    sims = sims or per_simulation(orders_list, points_list, countback, team, n_teams, init_points, init_counts)
    return dict(round_hist=np.array([CR.histogram(s['pos'], n) for s in sims]),
                contend=np.array([s['contend'].sum(axis=0) for s in sims], np.int64),
                secure=np.array([s['secure'].sum(axis=0) for s in sims], np.int64),
                team_round_hist=np.array([CR.histogram(s['tpos'], n_teams) for s in sims]),
                team_contend=np.array([s['tcontend'].sum(axis=0) for s in sims], np.int64),
                team_secure=np.array([s['tsecure'].sum(axis=0) for s in sims], np.int64))


KEYS = ('round_hist', 'contend', 'secure', 'team_round_hist', 'team_contend', 'team_secure')


def assert_identities(out, n_sims, champ_hist=None, team_hist=None):
    """What holds for the counts of any season (include/mcgp.h)."""
    for pre, hist in (('', champ_hist), ('team_', team_hist)):
        rh, con, sec = out[pre + 'round_hist'], out[pre + ('contend')], out[pre + 'secure']
        assert (rh.sum(axis=2) == n_sims).all() and (rh.sum(axis=1) == n_sims).all()
        if hist is not None:
            assert np.array_equal(rh[-1], hist)
        assert np.array_equal(sec[-1], rh[-1][:, 0]) and np.array_equal(con[-1], rh[-1][:, 0])
        assert (np.diff(sec, axis=0) >= 0).all()
        assert (con >= rh[:, :, 0]).all() and (sec <= rh[:, :, 0]).all()
        assert (sec.sum(axis=1) <= n_sims).all()


def edges(sims, n_sims):
    """What a decisive season must reach, from per_simulation's result: the rounds at which some but not all titles are
    secure; the driver and team non-leaders exactly on the bound (before the last round); the simulations whose top two
    drivers end level on points."""
    partial = [r for r, s in enumerate(sims) if 0 < s['secure'].sum() < n_sims]
    eq_d = eq_t = 0
    for s in sims[:-1]:
        lead = s['pts'].max(axis=1)
        eq_d += int((((lead[:, None] - s['pts']) == s['M']) & (s['pos'] != 0)).sum())
        tlead = s['tp'].max(axis=1)
        eq_t += int((((tlead[:, None] - s['tp']) == s['B'][None, :]) & (s['tpos'] != 0)).sum())
    top = np.sort(sims[-1]['pts'], axis=1)
    final_ties = int((top[:, -1] == top[:, -2]).sum()) if top.shape[1] > 1 else 0
    return dict(partial_rounds=partial, driver_on_bound=eq_d, team_on_bound=eq_t, final_points_ties=final_ties)


def assert_decisive(sims, n_sims, points_list, countback):
    """The four conditions of a decisive season."""
    e = edges(sims, n_sims)
    assert len(e['partial_rounds']) >= 3, e
    assert e['driver_on_bound'] > 0 and e['team_on_bound'] > 0, e
    assert e['final_points_ties'] > 0, e
    longest = max(len(t) for t in points_list)
    assert any(not cb and len(t) < longest for t, cb in zip(points_list, countback)), 'a sprint with a shorter table'
    return e
