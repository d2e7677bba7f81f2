"""numpy restatement of mcgp_run_gaps's counts (include/mcgp.h, csrc/gaps.hip.h) from per-lap times: the CPU oracle's
trace of the same simulations (resume_ref.traced_run: cum, dnf, grids), or, for many simulations from one state -- for
which the oracle has no entry point --, the Python restatement strategy_ref._Race with update_positions wrapped to
record (cum, dnf) per lap.  Also the C-ABI call for the tests.  Nothing here shares code with the kernel: the bin of a
value is numpy's searchsorted, the running order numpy's lexsort."""
import ctypes as C

import numpy as np

import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
from monte_carlo_gp_amd import _native as N

DEFAULT_EDGES = (0.5, 1, 2, 3, 5, 7.5, 10, 15, 20, 30, 45, 60, 90, 120)


def bin_of(x, edges):
    """The number of edges <= x: edges[b - 1] <= x < edges[b], a value equal to an edge goes up."""
    return np.searchsorted(np.asarray(edges, np.float64), x, side='right')


def empty(n, L, n_edges, n_pairs):
    B = n_edges + 1
    return dict(hist=np.zeros((n, n), np.int64), lap_gap=np.zeros((L, n, B + 1), np.int64),
                lead=np.zeros((L, B + 1), np.int64), pair=np.zeros((L, n_pairs, 2 * B + 1), np.int64))


def values_from_times(cum, dnf, slot, edges=DEFAULT_EDGES, pairs=()):
    """[m][L][n + 1 + P]: per simulation and lap the value of every row of the call -- driver d's bin or B = retired; the
    lead's bin or B = fewer than two running; pair p's column -- from cum, dnf [m][L][n] (after every lap) and slot
    [m][n] (each driver's grid slot)."""
    m, L, n = cum.shape
    B = len(edges) + 1
    vals = np.zeros((m, L, n + 1 + len(pairs)), np.int64)
    rows = np.arange(m)[:, None]
    pa, pb = (np.array(pairs, np.int64).reshape(-1, 2).T if len(pairs) else (None, None))
    for k in range(L):                                        # after lap k + 1
        t = cum[:, k, :]
        running = dnf[:, k, :] == 0
        order = np.lexsort((slot, t), axis=-1)                # (cumulative time, grid slot)
        run_sorted = running[rows, order]
        rank = np.cumsum(run_sorted, axis=1) - 1
        pos = np.empty((m, n), np.int64)
        pos[rows, order] = np.where(run_sorted, rank, n)      # running position, n = retired
        leader = np.where(pos == 0, t, 0.0).sum(axis=1)       # (one car at most is in position 0)
        second = np.where(pos == 1, t, 0.0).sum(axis=1)
        vals[:, k, :n] = np.where(running, bin_of(t - leader[:, None], edges), B)
        vals[:, k, n] = np.where(running.sum(axis=1) >= 2, bin_of(second - leader, edges), B)
        if len(pairs):                                        # all pairs at once: [m][P]
            both = running[:, pa] & running[:, pb]
            a_ahead = pos[:, pa] < pos[:, pb]
            v = np.where(a_ahead, bin_of(t[:, pb] - t[:, pa], edges), B + bin_of(t[:, pa] - t[:, pb], edges))
            vals[:, k, n + 1:] = np.where(both, v, 2 * B)
    return vals


def counts_from_values(vals, n, n_edges, n_pairs, lap0=0):
    """lap_gap, lead and pair from values [m][L][n + 1 + P]; the rows of laps 1 .. lap0 stay zero."""
    L, B = vals.shape[1], n_edges + 1
    out = empty(n, L, n_edges, n_pairs)
    v = np.asarray(vals, np.int64)[:, lap0:, :]
    for key, cols, width in (('lap_gap', slice(0, n), B + 1), ('lead', slice(n, n + 1), B + 1),
                             ('pair', slice(n + 1, n + 1 + n_pairs), 2 * B + 1)):
        x = v[:, :, cols]
        assert x.size == 0 or (0 <= x.min() and x.max() < width)
        cell = np.arange(x.shape[1] * x.shape[2]).reshape(1, x.shape[1], x.shape[2])      # (lap, row) of every value
        count = np.bincount((cell * width + x).ravel(), minlength=x.shape[1] * x.shape[2] * width)
        out[key][lap0:] = count.reshape((L - lap0,) + out[key].shape[1:])
    return out


def counts_from_times(cum, dnf, slot, edges=DEFAULT_EDGES, pairs=(), lap0=0):
    """lap_gap, lead and pair of m simulations from their times; the rows of laps 1 .. lap0 stay zero."""
    return counts_from_values(values_from_times(cum, dnf, slot, edges, pairs), cum.shape[2], len(edges), len(pairs), lap0)


def slots_of(grids):
    m, n = grids.shape
    slot = np.zeros((m, n), np.int64)
    slot[np.arange(m)[:, None], grids] = np.arange(n)[None, :]
    return slot


def gap_counts(case, m, seed, sim_offset=0, edges=DEFAULT_EDGES, pairs=(), ref=None, vals=None):
    """The counts (and the histogram) of simulations sim_offset .. sim_offset + m - 1 from the grid, from the oracle.
    vals: values_from_times of ref with these edges and pairs, where the caller has them already."""
    ref = ref or RR.traced_run(case, m, seed, sim_offset)
    tr = ref['trace']
    if vals is None:
        vals = values_from_times(tr['cum'], tr['dnf'], slots_of(ref['grids']), edges, pairs)
    out = counts_from_values(vals, tr['cum'].shape[2], len(edges), len(pairs))
    out['hist'] = ref['hist'].astype(np.int64)
    return out


def continued_counts(ref, sims, k, edges=DEFAULT_EDGES, pairs=(), vals=None):
    """The counts of the traced simulations `sims`, each resumed after lap k as itself: the oracle trace's laps k + 1 ..
    L of those simulations.  hist = their finishing orders' counts.  vals: values_from_times of the whole traced run with
    these edges and pairs, where a caller continues many states of one run."""
    tr = ref['trace']
    sims = np.asarray(sims)
    if vals is None:
        out = counts_from_times(tr['cum'][sims], tr['dnf'][sims], slots_of(ref['grids'][sims]), edges, pairs, lap0=k)
    else:
        out = counts_from_values(vals[sims], tr['cum'].shape[2], len(edges), len(pairs), lap0=k)
    out['hist'] = RR.counts(ref['orders'][sims], ref['grids'].shape[1])
    return out


def own_edges(cum, dnf, most=63):
    """Edges that are values the oracle itself shows: of the distinct positive gaps to the leader, cum[d] - cum[leader]
    over the running cars of every simulation and lap (the subtraction of values_from_times: the leader's time is the
    smallest of the running cars'), min(most, their number) at evenly spaced ranks; None when no gap is positive.  Each
    edge e then decides a cell of the reference by e <= e, and the next double above it by the opposite."""
    running = dnf == 0
    leader = np.where(running, cum, np.inf).min(axis=2, keepdims=True)
    gaps = (cum - np.where(np.isfinite(leader), leader, 0.0))[running]
    v = np.unique(gaps[gaps > 0])
    if v.size == 0:
        return None
    ranks = np.round(np.linspace(0, v.size - 1, min(most, v.size))).astype(np.int64)
    assert (np.diff(ranks) > 0).all()
    return tuple(float(x) for x in v[ranks])


def tied_pairs(cum, dnf, most=64):
    """(pairs, cells): the driver pairs (a, b) that some (simulation, lap) shows both running with EQUAL cumulative
    times -- where the pair's column is decided by the grid slots alone --, the most often tied first, each in both
    orientations, at most `most`; and the number of such (simulation, lap, pair a < b) cells."""
    n = cum.shape[2]
    times = np.zeros((n, n), np.int64)
    for t, x in zip(cum, dnf):                                # one simulation: [L][n]
        run = x == 0
        times += ((t[:, :, None] == t[:, None, :]) & run[:, :, None] & run[:, None, :]).sum(axis=0)
    times = np.triu(times, 1)
    a, b = np.nonzero(times)
    first = np.argsort(-times[a, b], kind='stable')
    pairs = [p for i in first for p in ((int(a[i]), int(b[i])), (int(b[i]), int(a[i])))]
    return pairs[:most], int(times.sum())


def pairs_then(first, more, most=64):
    """`first`, then those of `more` not yet listed, at most `most`."""
    out = list(first)
    for p in more:
        if p not in out:
            out.append(p)
    return out[:most]


def restated_times(case, m, seed, sim_offset=0, state=None, grids=None):
    """(cum, dnf [m][L][n], slot [m][n], orders [m][n]) of strategy_ref._Race (no plans), update_positions wrapped to record
    the times after every lap it runs (laps before a state's stay zero).  state = (arrays, lap, drs_disabled_until)."""
    M = SR.Model(case)
    n, L = M.n, M.L
    cum, dnf = np.zeros((m, L, n), np.float64), np.zeros((m, L, n), np.int64)
    slot, orders = np.zeros((m, n), np.int64), np.zeros((m, n), np.uint8)
    if state is None and grids is None:
        grids = RR.traced_run(case, m, seed, sim_offset)['grids']
    for i in range(m):
        r = SR._Race(M, seed, sim_offset + i)
        inner, rec = r.update_positions, []

        def wrapped(drs_allowed, inner=inner, r=r, rec=rec):
            inner(drs_allowed)
            rec.append((list(r.cum), list(r.dnf)))
        r.update_positions = wrapped
        first, dd = r.start_grid(grids[i], {}) if state is None else r.start_state(*state)
        if state is not None:
            rec.clear()                     # (start_state's update_positions restates the end of lap k: not recorded)
        r.laps(first, dd, {})
        lap_a = 0 if state is None else state[1]
        assert len(rec) == L - lap_a
        for j, (c, x) in enumerate(rec):
            cum[i, lap_a + j], dnf[i, lap_a + j] = c, x
        slot[i], orders[i] = r.gpos, r.classify()
    return cum, dnf, slot, orders


def restated_counts(case, m, seed, sim_offset=0, state=None, edges=DEFAULT_EDGES, pairs=()):
    """The counts of m simulations from the grid or from one state, from the wrapped restatement."""
    cum, dnf, slot, orders = restated_times(case, m, seed, sim_offset, state)
    out = counts_from_times(cum, dnf, slot, edges, pairs, lap0=0 if state is None else state[1])
    out['hist'] = RR.counts(orders, cum.shape[2])
    return out


def few_pairs(n):
    """A few pairs in both orientations; none for a field of one."""
    if n < 2:
        return []
    return [(0, 1), (1, 0), (n - 1, 0), (n // 2, n - 1)] if n > 2 else [(0, 1), (1, 0)]


def own_call(ref, most_pairs=64, more_pairs=None):
    """The edges and pairs of a call that the traced run `ref` itself decides: dict(edges = own_edges or, without a
    positive gap, the default ones; up = the next doubles above them; own = whether the edges are the run's; pairs =
    tied_pairs, then more_pairs (few_pairs unless given); cells = the run's tie cells)."""
    tr = ref['trace']
    n = tr['cum'].shape[2]
    edges = own_edges(tr['cum'], tr['dnf'])
    pairs, cells = tied_pairs(tr['cum'], tr['dnf'], most_pairs)
    use = edges if edges is not None else tuple(float(e) for e in DEFAULT_EDGES)
    return dict(edges=use, up=tuple(float(x) for x in np.nextafter(np.asarray(use, np.float64), np.inf)),
                own=edges is not None, cells=cells,
                pairs=pairs_then(pairs, few_pairs(n) if more_pairs is None else more_pairs, most_pairs))


def c_pairs(pairs):
    return np.ascontiguousarray(np.asarray(list(pairs), np.uint8).reshape(-1, 2))


def run_c(case, n_sims, seed, sim_offset=0, edges=DEFAULT_EDGES, pairs=(), state=None, device=0, prob=None, lead=True,
          into=None):
    """mcgp_run_gaps on a case -> (rc, counts dict as gap_counts returns).  state = (mcgp_race_state arrays, lap,
    drs_disabled_until) or None (from the grid).  into: a dict of uint64 arrays to accumulate into."""
    prob = prob or RR.problem(case)
    n, L = prob.n, case['config']['total_laps']
    g = np.ascontiguousarray(O.Problem(case).grid_probs, np.float64) if state is None else None
    cs = RR.c_state(*state) if state is not None else None
    e = np.ascontiguousarray(edges, np.float64)
    pr = c_pairs(pairs)
    out = into if into is not None else {k: v.astype(np.uint64) for k, v in empty(n, L, len(e), len(pr)).items()}
    u64 = lambda k: out[k].ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_gaps(C.byref(prob.cfg), C.byref(prob.drv),
                               g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None,
                               C.byref(cs) if cs is not None else None, n, len(e), e.ctypes.data_as(C.POINTER(C.c_double)),
                               len(pr), pr.ctypes.data_as(C.POINTER(C.c_uint8)) if len(pr) else None, int(n_sims),
                               int(sim_offset), int(seed), device, u64('hist'), u64('lap_gap'), u64('lead') if lead else None,
                               u64('pair') if len(pr) else None)
    return rc, {k: v.astype(np.int64) for k, v in out.items()}


def budget_sims(n, L_rec, n_pairs, cap=0xFFFFFE00):
    """The staging budget of mcgp_run_gaps: 512 MiB / (recorded laps x (n + 1 + n_pairs)) simulations, at most the launch
    cap, in multiples of 256 when it can."""
    c = min(cap, max(1, (512 << 20) // (L_rec * (n + 1 + n_pairs))))
    return c // 256 * 256 if c >= 256 else c


def chunk_sims(n, L_rec, n_pairs, device_round):
    """The documented chunk rule: the budget, rounded down to whole rounds of the device (device_round = grid_blocks x
    block_threads of a full launch, mcgp_last_launch_info)."""
    c = budget_sims(n, L_rec, n_pairs)
    return c // device_round * device_round if c >= device_round else c
