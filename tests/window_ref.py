"""numpy restatement of mcgp_run_pit_windows's counts (include/mcgp.h, csrc/pit_window.hip.h) from per-lap times: the CPU
oracle's trace of the same simulations (resume_ref.traced_run: cum, dnf, grids), or, for many simulations from one
state, gaps_ref.restated_times.  Also the C-ABI call for the tests.  Nothing here shares code with the kernel, which
walks the running order once and keeps the last car seen ahead: here the hypothetical rejoin key (t*, slot of a) is put
among the other running cars' keys as one more entry, numpy's lexsort orders them, and the entry's place in that order
is the rejoin position, its neighbours the cars ahead and behind; a bin is numpy's searchsorted."""
import ctypes as C

import numpy as np

import gaps_ref as GR
import oracle_py as O
import resume_ref as RR
from monte_carlo_gp_amd import _native as N

DEFAULT_EDGES = GR.DEFAULT_EDGES
KEYS = ('hist', 'rejoin', 'lost', 'ahead', 'gap_ahead', 'gap_behind')
ROWS = KEYS[1:]                         # the staged rows of a window, in the staging's order


def widths(n, n_edges):
    """The width of each row's value range, by name."""
    B = n_edges + 1
    return dict(rejoin=n + 1, lost=n + 1, ahead=n + 2, gap_ahead=B + 1, gap_behind=B + 1)


def empty(n, L, n_edges, n_windows):
    out = {k: np.zeros((L, n_windows, w), np.int64) for k, w in widths(n, n_edges).items()}
    out['hist'] = np.zeros((n, n), np.int64)
    return out


def values_from_times(cum, dnf, slot, windows, edges=DEFAULT_EDGES):
    """[m][L][W][5]: per simulation, lap and window the five staged values (rejoin, lost, ahead, gap_ahead, gap_behind)
    from cum, dnf [m][L][n] (after every lap) and slot [m][n] (each driver's grid slot); windows = [(driver index,
    loss), ...]."""
    m, L, n = cum.shape
    B, W = len(edges) + 1, len(windows)
    a = np.array([w[0] for w in windows], np.int64)
    loss = np.array([w[1] for w in windows], np.float64)
    vals = np.zeros((m, L, W, 5), np.int64)
    mi = np.arange(m)[:, None]
    slot_all = np.concatenate([np.broadcast_to(slot[:, None, :], (m, W, n)), slot[:, a][:, :, None]], axis=2)
    for k in range(L):                                        # after lap k + 1
        t = cum[:, k, :]
        running = dnf[:, k, :] == 0
        # a's own running position: its place among all cars by (time, slot), the retired ones behind every runner
        order = np.lexsort((slot, np.where(running, t, np.inf)), axis=-1)
        pos = np.empty((m, n), np.int64)
        pos[mi, order] = np.arange(n)[None, :]
        ts = t[:, a] + loss[None, :]                          # [m][W]: one addition
        a_runs = running[:, a]
        others = running[:, None, :] & (np.arange(n)[None, None, :] != a[None, :, None])          # [m][W][n]
        # the other running cars' keys and, as entry n, the rejoin key (t*, slot of a); whoever is not in it goes last
        t_all = np.concatenate([np.where(others, t[:, None, :], np.inf), ts[:, :, None]], axis=2)
        srt = np.lexsort((slot_all, t_all), axis=-1)          # [m][W][n + 1]
        rank = np.argmax(srt == n, axis=-1)                   # entries before the rejoin key: the cars ahead
        count = others.sum(axis=-1)
        prev = np.take_along_axis(srt, np.maximum(rank - 1, 0)[..., None], axis=-1)[..., 0]
        nxt = np.take_along_axis(srt, np.minimum(rank + 1, n)[..., None], axis=-1)[..., 0]
        has_prev, has_next = rank > 0, rank < count
        t_prev = t[mi, np.where(has_prev, prev, 0)]
        t_next = t[mi, np.where(has_next, nxt, 0)]
        gap_a = np.where(has_prev, ts - t_prev, 0.0)
        gap_b = np.where(has_next, t_next - ts, 0.0)
        assert (gap_a >= 0).all() and (gap_b >= 0).all()
        vals[:, k, :, 0] = np.where(a_runs, rank, n)
        vals[:, k, :, 1] = np.where(a_runs, rank - pos[:, a], n)
        vals[:, k, :, 2] = np.where(a_runs, np.where(has_prev, prev, n), n + 1)
        vals[:, k, :, 3] = np.where(a_runs & has_prev, GR.bin_of(gap_a, edges), B)
        vals[:, k, :, 4] = np.where(a_runs & has_next, GR.bin_of(gap_b, edges), B)
    return vals


def counts_from_values(vals, n, n_edges, lap0=0):
    """rejoin, lost, ahead, gap_ahead and gap_behind from values [m][L][W][5]; the rows of laps 1 .. lap0 stay zero."""
    m, L, W, _ = vals.shape
    out = empty(n, L, n_edges, W)
    v = np.asarray(vals, np.int64)[:, lap0:]
    cell = np.arange((L - lap0) * W).reshape(1, L - lap0, W)
    for r, key in enumerate(ROWS):
        width = out[key].shape[2]
        x = v[..., r]
        assert x.size == 0 or (0 <= x.min() and x.max() < width), key
        count = np.bincount((cell * width + x).ravel(), minlength=(L - lap0) * W * width)
        out[key][lap0:] = count.reshape(L - lap0, W, width)
    return out


def window_counts(case, m, seed, sim_offset=0, windows=(), edges=DEFAULT_EDGES, ref=None, vals=None):
    """The counts (and the histogram) of simulations sim_offset .. sim_offset + m - 1 from the grid, from the oracle."""
    ref = ref or RR.traced_run(case, m, seed, sim_offset)
    tr = ref['trace']
    if vals is None:
        vals = values_from_times(tr['cum'], tr['dnf'], GR.slots_of(ref['grids']), windows, edges)
    out = counts_from_values(vals, tr['cum'].shape[2], len(edges))
    out['hist'] = ref['hist'].astype(np.int64)
    return out


def continued_counts(ref, sims, k, windows, edges=DEFAULT_EDGES, vals=None):
    """The counts of the traced simulations `sims`, each resumed after lap k as itself: the oracle trace's laps k + 1 ..
    L of those simulations.  hist = their finishing orders' counts."""
    tr = ref['trace']
    sims = np.asarray(sims)
    if vals is None:
        vals = values_from_times(tr['cum'], tr['dnf'], GR.slots_of(ref['grids']), windows, edges)
    out = counts_from_values(vals[sims], tr['cum'].shape[2], len(edges), lap0=k)
    out['hist'] = RR.counts(ref['orders'][sims], ref['grids'].shape[1])
    return out


def restated_counts(case, m, seed, sim_offset=0, state=None, windows=(), edges=DEFAULT_EDGES):
    """The counts of m simulations from the grid or from one state (arrays, lap, drs_disabled_until), from
    gaps_ref.restated_times."""
    cum, dnf, slot, orders = GR.restated_times(case, m, seed, sim_offset, state)
    lap0 = 0 if state is None else state[1]
    out = counts_from_values(values_from_times(cum, dnf, slot, windows, edges), cum.shape[2], len(edges), lap0)
    out['hist'] = RR.counts(orders, cum.shape[2])
    return out


def tie_cells(cum, dnf, loss, drivers=None):
    """The number of ordered pairs (a, d), a in `drivers` (None: all), of running cars in one (simulation, lap) with
    Cum(d) == Cum(a) + loss: the cells whose side of the rejoin the grid slots decide."""
    n = cum.shape[2]
    cells = 0
    for a in (range(n) if drivers is None else drivers):
        ts = cum[:, :, a] + np.float64(loss)
        hit = (cum == ts[:, :, None]) & (dnf == 0) & (dnf[:, :, a] == 0)[:, :, None]
        hit[:, :, a] = False
        cells += int(hit.sum())
    return cells


def own_losses(cum, dnf, most=3, tried=12):
    """Losses taken from the run's own commonest positive time differences Cum(d) - Cum(a) between two running cars of
    one (simulation, lap): of the `tried` most frequent, those at which the rejoin time Cum(a) + loss -- the addition,
    not the difference it came from -- equals a running car's time somewhere, the most tie cells first, at most `most`."""
    run = dnf == 0
    diff = cum[:, :, :, None] - cum[:, :, None, :]
    both = run[:, :, :, None] & run[:, :, None, :]
    v, c = np.unique(diff[both & (diff > 0)], return_counts=True)
    cells = {float(v[i]): tie_cells(cum, dnf, float(v[i])) for i in np.argsort(-c, kind='stable')[:tried]}
    return [x for x in sorted(cells, key=lambda x: -cells[x]) if cells[x] > 0][:most]


def every_driver(n, losses):
    """Windows (driver, loss) of every driver at each of `losses`, driver-major, at most 64."""
    return [(d, float(x)) for d in range(n) for x in losses][:64]


def run_c(case, n_sims, seed, sim_offset=0, windows=(), edges=DEFAULT_EDGES, state=None, device=0, prob=None, into=None,
          null=()):
    """mcgp_run_pit_windows on a case -> (rc, counts dict as window_counts returns).  windows = [(driver index, loss)];
    state = (mcgp_race_state arrays, lap, drs_disabled_until) or None (from the grid).  into: a dict of uint64 arrays to
    accumulate into.  null: names of arguments passed as NULL ('edges', 'window_drivers', 'window_losses', or an output)."""
    prob = prob or RR.problem(case)
    n, L = prob.n, case['config']['total_laps']
    g = np.ascontiguousarray(O.Problem(case).grid_probs, np.float64) if state is None else None
    cs = RR.c_state(*state) if state is not None else None
    e = np.ascontiguousarray(edges, np.float64)
    wd = np.ascontiguousarray([w[0] for w in windows], np.uint8)
    wl = np.ascontiguousarray([w[1] for w in windows], np.float64)
    out = into if into is not None else {k: v.astype(np.uint64) for k, v in empty(n, L, len(e), len(wd)).items()}
    u64 = lambda k: None if k in null else out[k].ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_pit_windows(
        C.byref(prob.cfg), C.byref(prob.drv), g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None,
        C.byref(cs) if cs is not None else None, n, len(e),
        None if 'edges' in null else e.ctypes.data_as(C.POINTER(C.c_double)), len(wd),
        None if 'window_drivers' in null else wd.ctypes.data_as(C.POINTER(C.c_uint8)),
        None if 'window_losses' in null else wl.ctypes.data_as(C.POINTER(C.c_double)), int(n_sims), int(sim_offset),
        int(seed), device, *[u64(k) for k in KEYS])
    return rc, {k: v.astype(np.int64) for k, v in out.items()}


def budget_sims(L_rec, n_windows, cap=0xFFFFFE00):
    """The staging budget of mcgp_run_pit_windows: 1 GiB / (recorded laps x 5 W) simulations, at most the launch cap, in
    multiples of 256 when it can."""
    c = min(cap, max(1, (1024 << 20) // (L_rec * 5 * n_windows)))
    return c // 256 * 256 if c >= 256 else c


def chunk_sims(L_rec, n_windows, device_round):
    """The documented chunk rule: the budget, rounded down to whole rounds of the device."""
    c = budget_sims(L_rec, n_windows)
    return c // device_round * device_round if c >= device_round else c
