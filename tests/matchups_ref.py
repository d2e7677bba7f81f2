"""Head-to-head and podium counts restated in numpy, independently of the device's mask-and-ballot method.

TEST INFRASTRUCTURE.  Input: finishing orders [sims][n] (driver index classified p-th).  Positions come from inverting
each order; driver i is ahead of driver j when its position is smaller; the podium cell is the first three entries.
"""
import numpy as np


def positions(orders):
    """[sims][n]: the classified position (0-based) of driver d in each simulation."""
    orders = np.asarray(orders).astype(np.int64)
    sims, n = orders.shape
    pos = np.empty((sims, n), np.int8)                  # n <= 32
    rows = np.arange(sims)
    for p in range(n):
        pos[rows, orders[:, p]] = p
    return pos


def hist(orders):
    """[n][n] counts of [driver][position]."""
    orders = np.asarray(orders).astype(np.int64)
    n = orders.shape[1]
    h = np.zeros((n, n), np.int64)
    for p in range(n):
        h[:, p] = np.bincount(orders[:, p], minlength=n)
    return h


def ahead(orders):
    """[n][n]: ahead[i][j] = simulations in which driver i is classified ahead of driver j."""
    pos = positions(orders)
    n = pos.shape[1]
    a = np.zeros((n, n), np.int64)
    for i in range(n):
        a[i] = (pos[:, i:i + 1] < pos).sum(axis=0)
    return a


def podium(orders):
    """[n][n][n]: simulations whose first three classified cars are a, b, c in that order."""
    orders = np.asarray(orders).astype(np.int64)
    n = orders.shape[1]
    cell = (orders[:, 0] * n + orders[:, 1]) * n + orders[:, 2]
    return np.bincount(cell, minlength=n ** 3).reshape(n, n, n).astype(np.int64)


def matchups(orders, podiums=True):
    """(hist, ahead, podium or None): what mcgp_run_matchups counts for these orders."""
    orders = np.asarray(orders)
    want = podiums and orders.shape[1] >= 3
    return hist(orders), ahead(orders), podium(orders) if want else None


def ahead_by_loop(orders):
    """ahead() once more with a plain loop over simulations and pairs (small inputs only)."""
    orders = np.asarray(orders)
    n = orders.shape[1]
    a = np.zeros((n, n), np.int64)
    for row in orders:
        row = [int(x) for x in row]
        for p, i in enumerate(row):
            for j in row[p + 1:]:
                a[i, j] += 1
    return a
