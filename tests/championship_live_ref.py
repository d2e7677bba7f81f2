"""Title odds by finishing position restated in numpy / Python, independently of the device's packed standing keys.

TEST INFRASTRUCTURE.  The joint table of mcgp_run_championship_live: given[d][p][e] = simulations in which driver d is
classified p + 1-th in race `given_race` and driver e is champion.  The standings and the ranking are championship_ref's
(points, then countback, then the lower index); the champion is the entrant at position 0.
"""
import numpy as np

import championship_ref as CR


def champions(orders_list, points_list, countback, init_points=None, init_counts=None, bonus=None, rank=CR.rank):
    """[sims] the champion of every simulation.  bonus: None or [R][sims][n] bonus points per race, simulation and driver
    (championship_bonus_ref.bonus_matrix); they add to the points only."""
    pts, cnt = CR.standings(orders_list, points_list, countback, init_points, init_counts)
    if bonus is not None:
        pts = pts + np.asarray(bonus, np.int64).sum(axis=0)
    pos = rank(pts, cnt)
    champ = np.argmin(pos, axis=1)
    assert (pos[np.arange(len(champ)), champ] == 0).all()
    return champ


def title_given(orders_list, points_list, countback, given_race, init_points=None, init_counts=None, bonus=None,
                rank=CR.rank):
    """given [n][n][n] int64 = [driver][position in race given_race][champion]."""
    orders = np.asarray(orders_list[given_race]).astype(np.int64)
    sims, n = orders.shape
    champ = champions(orders_list, points_list, countback, init_points, init_counts, bonus, rank)
    out = np.zeros((n, n, n), np.int64)
    for p in range(n):
        np.add.at(out, (orders[:, p], p, champ), 1)
    return out


def title_given_of(orders, champ):
    """title_given's table from one race's orders [sims][n] and the champions [sims] the caller already has, by bincount:
    for millions of simulations (tests/test_championship_live_host.py holds the two together)."""
    orders = np.asarray(orders).astype(np.int64)
    sims, n = orders.shape
    cell = (orders * n + np.arange(n)[None, :]) * n + np.asarray(champ, np.int64)[:, None]
    return np.bincount(cell.reshape(-1), minlength=n ** 3).reshape(n, n, n)


def check_invariants(given, race_hist, champ_hist):
    """The two invariants of the table against the given race's position histogram and the season's champ_hist."""
    given = np.asarray(given, np.int64)
    n = given.shape[0]
    assert np.array_equal(given.sum(axis=2), np.asarray(race_hist, np.int64))
    assert np.array_equal(given.sum(axis=0), np.tile(np.asarray(champ_hist, np.int64)[:, 0][None, :], (n, 1)))
