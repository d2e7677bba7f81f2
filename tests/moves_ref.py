"""numpy restatement of mcgp_run_moves's counts (include/mcgp.h, csrc/moves.hip.h) from per-lap data: the CPU oracle's
trace of the same simulations (resume_ref.traced_run: cum, dnf, age, grids, orders), or, for many simulations from one
state -- for which the oracle has no entry point --, the Python restatement strategy_ref._Race with update_positions
wrapped to record (cum, dnf, age) per lap.  Also the C-ABI call for the tests.  Nothing here shares code with the
kernel: positions come from numpy's lexsort of (cumulative time, grid slot), passes from comparing every ordered pair of
cars' positions on two consecutive laps."""
import copy
import ctypes as C

import numpy as np

import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
from monte_carlo_gp_amd import _native as N

DRIVER_CAP, RACE_CAP = 127, 1023
KEYS = ('hist', 'grid_fin', 'start_gain', 'passes', 'race_passes', 'lap_passes', 'pair_passes')
OPTIONAL = KEYS[2:]


def empty(n, L):
    z = lambda *shape: np.zeros(shape, np.int64)
    return dict(hist=z(n, n), grid_fin=z(n, n, n), start_gain=z(n, 2 * n), passes=z(n, 4, DRIVER_CAP + 1),
                race_passes=z(RACE_CAP + 1), lap_passes=z(L + 1, 2), pair_passes=z(n, n))


def slots_of(grids):
    """[m][n]: every driver's grid slot from the sampled grids (grids[i][slot] = driver)."""
    m, n = grids.shape
    slot = np.zeros((m, n), np.int64)
    slot[np.arange(m)[:, None], grids] = np.arange(n)[None, :]
    return slot


def positions_of(orders):
    m, n = orders.shape
    pos = np.zeros((m, n), np.int64)
    pos[np.arange(m)[:, None], orders] = np.arange(n)[None, :]
    return pos


def running_positions(cum, dnf, slot):
    """pos [m][n] after one lap: the rank among the running cars by (cumulative time, grid slot), n for a retired car."""
    m, n = cum.shape
    rows = np.arange(m)[:, None]
    running = dnf == 0
    order = np.lexsort((slot, cum), axis=-1)
    run_sorted = running[rows, order]
    pos = np.empty((m, n), np.int64)
    pos[rows, order] = np.where(run_sorted, np.cumsum(run_sorted, axis=1) - 1, n)
    return pos


def tallies(cum, dnf, age, slot, lap0):
    """Per simulation, over the laps lap0 + 1 .. L with the baseline after lap lap0 (>= 1), from cum, dnf, age [m][L][n]
    after every lap and slot [m][n]: dict(kinds [m][n][4] a car's passes by kind, uncapped; race [m] on-track passes;
    lap [m][L + 1][2]; pair [m][n][n] on track; pos1 [m][n] the positions after lap 1)."""
    m, L, n = cum.shape
    kinds = np.zeros((m, n, 4), np.int64)
    lap = np.zeros((m, L + 1, 2), np.int64)
    pair = np.zeros((m, n, n), np.int64)
    prev = running_positions(cum[:, lap0 - 1], dnf[:, lap0 - 1], slot)
    for k in range(lap0 + 1, L + 1):
        cur = running_positions(cum[:, k - 1], dnf[:, k - 1], slot)
        both = (prev < n) & (cur < n)
        pit = (cur < n) & (age[:, k - 1] == 0) & (k >= 2)
        # took[i][a][b]: a took a place from b on lap k
        took = (both[:, :, None] & both[:, None, :] & (prev[:, :, None] > prev[:, None, :]) &
                (cur[:, :, None] < cur[:, None, :]))
        pits = took & (pit[:, :, None] | pit[:, None, :])
        track = took & ~pits
        kinds[:, :, 0] += track.sum(axis=2)
        kinds[:, :, 1] += track.sum(axis=1)
        kinds[:, :, 2] += pits.sum(axis=2)
        kinds[:, :, 3] += pits.sum(axis=1)
        lap[:, k, 0] = track.sum(axis=(1, 2))
        lap[:, k, 1] = pits.sum(axis=(1, 2))
        pair += track
        prev = cur
    return dict(kinds=kinds, race=lap[:, :, 0].sum(axis=1), lap=lap, pair=pair,
                pos1=running_positions(cum[:, 0], dnf[:, 0], slot))


def counts_from_tallies(t, slot, positions, L, from_grid):
    """Every output but hist from tallies(), slot [m][n] and positions [m][n] (classified, 0-based)."""
    m, n = slot.shape
    out = empty(n, L)
    for d in range(n):
        np.add.at(out['grid_fin'][d], (slot[:, d], positions[:, d]), 1)
        if from_grid:
            p1 = t['pos1'][:, d]
            out['start_gain'][d] = np.bincount(np.where(p1 < n, slot[:, d] - p1 + n - 1, 2 * n - 1), minlength=2 * n)
        for kind in range(4):
            out['passes'][d, kind] = np.bincount(np.minimum(t['kinds'][:, d, kind], DRIVER_CAP), minlength=DRIVER_CAP + 1)
    out['race_passes'] = np.bincount(np.minimum(t['race'], RACE_CAP), minlength=RACE_CAP + 1)
    out['lap_passes'] = t['lap'].sum(axis=0)
    out['pair_passes'] = t['pair'].sum(axis=0)
    return out


def move_counts(case, m, seed, sim_offset=0, ref=None, with_tallies=False):
    """The counts (and the histogram) of simulations sim_offset .. sim_offset + m - 1 from the grid, from the oracle."""
    ref = ref or RR.traced_run(case, m, seed, sim_offset)
    tr = ref['trace']
    L = tr['cum'].shape[1]
    slot = slots_of(ref['grids'])
    t = tallies(tr['cum'], tr['dnf'], tr['age'], slot, 1)
    out = counts_from_tallies(t, slot, positions_of(ref['orders']), L, True)
    out['hist'] = ref['hist'].astype(np.int64)
    return (out, t) if with_tallies else out


def continued_counts(ref, sims, k):
    """The counts of the traced simulations `sims` (indices into ref), each resumed after lap k as itself: the oracle
    trace's laps k + 1 .. L of those simulations with the baseline after lap k.  hist = their finishing orders' counts."""
    tr = ref['trace']
    sims = np.asarray(sims)
    L, n = tr['cum'].shape[1], tr['cum'].shape[2]
    slot = slots_of(ref['grids'][sims])
    t = tallies(tr['cum'][sims], tr['dnf'][sims], tr['age'][sims], slot, k)
    out = counts_from_tallies(t, slot, positions_of(ref['orders'][sims]), L, False)
    out['hist'] = RR.counts(ref['orders'][sims], n)
    return out


def restated_counts(case, m, seed, sim_offset=0, state=None):
    """The counts of m simulations from the grid or from one state = (arrays, lap, drs_disabled_until), from
    strategy_ref._Race (no plans) with update_positions wrapped to record the field after every lap it runs -- and, from
    a state, after the start's own update_positions, which is the baseline."""
    M = SR.Model(case)
    n, L = M.n, M.L
    cum = np.zeros((m, L, n), np.float64)
    dnf, age = np.zeros((m, L, n), np.int64), np.zeros((m, L, n), np.int64)
    slot, orders = np.zeros((m, n), np.int64), np.zeros((m, n), np.int64)
    grids = RR.traced_run(case, m, seed, sim_offset)['grids'] if state is None else None
    lap_a = 1 if state is None else int(state[1])
    for i in range(m):
        r = SR._Race(M, seed, sim_offset + i)
        inner, rec = r.update_positions, []

        def wrapped(drs_allowed, inner=inner, r=r, rec=rec):
            inner(drs_allowed)
            rec.append((list(r.cum), list(r.dnf), list(r.age)))
        r.update_positions = wrapped
        first, dd = r.start_grid(grids[i], {}) if state is None else r.start_state(*state)
        r.laps(first, dd, {})
        assert len(rec) == L - lap_a + 1                    # the start's (lap 1, or the state's lap), then every lap run
        for j, (c, x, a) in enumerate(rec):
            cum[i, lap_a - 1 + j], dnf[i, lap_a - 1 + j], age[i, lap_a - 1 + j] = c, x, a
        slot[i] = r.gpos
        orders[i] = r.classify()
    t = tallies(cum, dnf, age, slot, lap_a)
    out = counts_from_tallies(t, slot, positions_of(orders), L, state is None)
    out['hist'] = RR.counts(orders, n)
    return out


def cap_case():
    """S78 over 400 laps: more than 127 on-track passes by one driver and more than 1023 in one race."""
    case = copy.deepcopy(O.load_case('S78'))
    case['config']['total_laps'] = 400
    return case


def run_c(case, n_sims, seed, sim_offset=0, state=None, device=0, prob=None, skip=(), into=None):
    """mcgp_run_moves on a case -> (rc, counts dict as move_counts returns).  state = (mcgp_race_state arrays, lap,
    drs_disabled_until) or None (from the grid).  into: a dict of uint64 arrays to accumulate into.  skip: the outputs
    passed as NULL (from a state start_gain always is)."""
    prob = prob or RR.problem(case)
    n, L = prob.n, case['config']['total_laps']
    g = np.ascontiguousarray(O.Problem(case).grid_probs, np.float64) if state is None else None
    cs = RR.c_state(*state) if state is not None else None
    out = into if into is not None else {k: v.astype(np.uint64) for k, v in empty(n, L).items()}
    skip = set(skip) | ({'start_gain'} if state is not None else set())
    u64 = lambda k: None if k in skip else out[k].ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_moves(C.byref(prob.cfg), C.byref(prob.drv),
                                g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None,
                                C.byref(cs) if cs is not None else None, n, int(n_sims), int(sim_offset), int(seed),
                                device, *[u64(k) for k in KEYS])
    return rc, {k: v.astype(np.int64) for k, v in out.items()}


def budget_sims(n, L, cap=0xFFFFFE00):
    """The staging budget of mcgp_run_moves: 512 MiB / ((L + 2) n) simulations, at most the launch cap, in multiples of
    256 when it can."""
    c = min(cap, max(1, (512 << 20) // ((L + 2) * n)))
    return c // 256 * 256 if c >= 256 else c


def chunk_sims(n, L, device_round):
    """The documented chunk rule: the budget, rounded down to whole rounds of the device (device_round = grid_blocks x
    block_threads of a full launch, mcgp_last_launch_info)."""
    c = budget_sims(n, L)
    return c // device_round * device_round if c >= device_round else c
