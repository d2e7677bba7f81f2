"""numpy restatement of mcgp_run_stints's counts (include/mcgp.h, csrc/stints.hip.h) from per-lap tyre data: the CPU
oracle's trace of the same simulations (resume_ref.traced_run: age, comp, dnf) with the red flags restated from the
event draws (trace_ref.lap_event_kind), or, for many simulations from one state -- for which the oracle has no entry
point --, the Python restatement strategy_ref._Race with update_positions wrapped to record (age, comp, dnf) per lap.
Also the C-ABI call for the tests.  Nothing here shares code with the kernel."""
import copy
import ctypes as C

import numpy as np

import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
import trace_ref as TR
from monte_carlo_gp_amd import _native as N

STOPS, SEQ, CODES = 4, 4, 1296
KEYS = ('hist', 'stop_lap', 'stops_pos', 'seq')


def empty(n, L):
    return dict(hist=np.zeros((n, n), np.int64), stop_lap=np.zeros((n, STOPS, L + 1), np.int64),
                stops_pos=np.zeros((n, STOPS + 1, n), np.int64), seq=np.zeros((n, CODES), np.int64))


def red_flags(case, seed, sims, L):
    """[len(sims)][L] bool: lap k + 1 of that simulation drew a red flag (lap 1 draws no event)."""
    red = np.zeros((len(sims), L), bool)
    for j, sim in enumerate(sims):
        for lap in range(2, L + 1):
            red[j, lap - 1] = TR.lap_event_kind(case, seed, int(sim), lap) == TR.RED
    return red


def start_compounds(case, grids):
    """[m][n]: the compound _initialize_cars gives every driver on the sampled grids (wet: WET, damp: INTERMEDIATE, dry:
    SOFT on slots 1-10, MEDIUM behind)."""
    m, n = grids.shape
    track = O.TRACK_ID[case.get('track_condition', 'dry')]
    by_slot = np.full(n, 4 if track == 2 else 3, np.int64) if track else np.where(np.arange(n) < 10, 0, 1)
    comp0 = np.zeros((m, n), np.int64)
    comp0[np.arange(m)[:, None], grids] = by_slot[None, :]
    return comp0


def tallies(age, comp, dnf, red, comp0, lap0):
    """Per (simulation, car) over the recorded laps lap0 + 1 .. L, from age, comp, dnf [m][L][n] (after every lap), red
    [m][L] and the compounds of stint 0 [m][n]: dict(stops [m][n], stints [m][n], code [m][n] (0 = more than 4 stints),
    laps [m][n][4] (0 = no such stop), both = the (simulation, lap, car) cells with a stop under a red flag)."""
    m, L, n = age.shape
    stops, stints = np.zeros((m, n), np.int64), np.ones((m, n), np.int64)
    code = np.asarray(comp0, np.int64) + 1
    laps = np.zeros((m, n, STOPS), np.int64)
    both = 0
    for lap in range(lap0 + 1, L + 1):
        run = dnf[:, lap - 1, :] == 0
        stop = run & (age[:, lap - 1, :] == 0)
        change = run & red[:, lap - 1, None]
        new = stop | change
        both += int((stop & change).sum())
        code = code + np.where(new & (stints < SEQ), (comp[:, lap - 1, :].astype(np.int64) + 1) * 6 ** np.minimum(stints, SEQ), 0)
        stints = stints + new
        for k in range(STOPS):
            laps[:, :, k] = np.where(stop & (stops == k), lap, laps[:, :, k])
        stops = stops + stop
    return dict(stops=stops, stints=stints, code=np.where(stints > SEQ, 0, code), laps=laps, both=both)


def counts_from_tallies(t, positions, L):
    """stop_lap, stops_pos and seq from tallies() and positions [m][n] (each driver's classified position, 0-based)."""
    m, n = t['stops'].shape
    out = empty(n, L)
    for d in range(n):
        for k in range(STOPS):
            out['stop_lap'][d, k] = np.bincount(t['laps'][:, d, k], minlength=L + 1)
        np.add.at(out['stops_pos'][d], (np.minimum(t['stops'][:, d], STOPS), positions[:, d]), 1)
        out['seq'][d] = np.bincount(t['code'][:, d], minlength=CODES)
    return out


def positions_of(orders):
    m, n = orders.shape
    pos = np.zeros((m, n), np.int64)
    pos[np.arange(m)[:, None], orders] = np.arange(n)[None, :]
    return pos


def stint_counts(case, m, seed, sim_offset=0, ref=None, with_tallies=False):
    """The counts (and the histogram) of simulations sim_offset .. sim_offset + m - 1 from the grid, from the oracle."""
    ref = ref or RR.traced_run(case, m, seed, sim_offset)
    tr = ref['trace']
    L = tr['age'].shape[1]
    comp0 = start_compounds(case, ref['grids'])
    assert np.array_equal(comp0, tr['comp'][:, 0, :])            # (lap 1 changes no tyre: the trace shows the start's)
    t = tallies(tr['age'], tr['comp'], tr['dnf'], red_flags(case, seed, sim_offset + np.arange(m), L), comp0, 1)
    out = counts_from_tallies(t, positions_of(ref['orders']), L)
    out['hist'] = ref['hist'].astype(np.int64)
    return (out, t) if with_tallies else out


def continued_counts(ref, sims, k, case, seed, sim_offset=0):
    """The counts of the traced simulations `sims` (indices into ref, ids sim_offset + index), each resumed after lap k
    as itself: the oracle trace's laps k + 1 .. L of those simulations, stint 0 on the compound after lap k.  hist = their
    finishing orders' counts."""
    tr = ref['trace']
    sims = np.asarray(sims)
    L, n = tr['age'].shape[1], tr['age'].shape[2]
    t = tallies(tr['age'][sims], tr['comp'][sims], tr['dnf'][sims], red_flags(case, seed, sim_offset + sims, L),
                tr['comp'][sims, k - 1, :], k)
    out = counts_from_tallies(t, positions_of(ref['orders'][sims]), L)
    out['hist'] = RR.counts(ref['orders'][sims], n)
    return out


def restated_counts(case, m, seed, sim_offset=0, state=None):
    """The counts of m simulations from the grid or from one state = (arrays, lap, drs_disabled_until), from
    strategy_ref._Race (no plans) with update_positions wrapped to record the tyres after every lap it runs."""
    M = SR.Model(case)
    n, L = M.n, M.L
    age, comp, dnf = (np.zeros((m, L, n), np.int64) for _ in range(3))
    comp0, orders = np.zeros((m, n), np.int64), np.zeros((m, n), np.int64)
    grids = RR.traced_run(case, m, seed, sim_offset)['grids'] if state is None else None
    lap_a = 0 if state is None else int(state[1])
    for i in range(m):
        r = SR._Race(M, seed, sim_offset + i)
        inner, rec = r.update_positions, []

        def wrapped(drs_allowed, inner=inner, r=r, rec=rec):
            inner(drs_allowed)
            rec.append((list(r.age), list(r.comp), list(r.dnf)))
        r.update_positions = wrapped
        first, dd = r.start_grid(grids[i], {}) if state is None else r.start_state(*state)
        if state is not None:
            rec.clear()                     # (start_state's update_positions restates the end of lap k: not recorded)
            comp0[i] = r.comp
        r.laps(first, dd, {})
        assert len(rec) == L - lap_a
        for j, (a, c, x) in enumerate(rec):
            age[i, lap_a + j], comp[i, lap_a + j], dnf[i, lap_a + j] = a, c, x
        if state is None:
            comp0[i] = comp[i, 0]
        orders[i] = r.classify()
    t = tallies(age, comp, dnf, red_flags(case, seed, sim_offset + np.arange(m), L), comp0, max(lap_a, 1))
    out = counts_from_tallies(t, positions_of(orders), L)
    out['hist'] = RR.counts(orders, n)
    return out


def cap_case():
    """S60 over 12 laps with a red flag every other lap and tyres that are worn out at once: five and more stops, stops
    under a red flag, up to 12 stints."""
    case = copy.deepcopy(O.load_case('S60'))
    case['config']['total_laps'] = 12
    case['config']['red_flag_probability'] = 0.5
    case['config']['tire_compounds'] = {c: dict(v, optimal_laps=0) for c, v in case['config']['tire_compounds'].items()}
    return case


def run_c(case, n_sims, seed, sim_offset=0, state=None, device=0, prob=None, optional=True, into=None):
    """mcgp_run_stints on a case -> (rc, counts dict as stint_counts returns).  state = (mcgp_race_state arrays, lap,
    drs_disabled_until) or None (from the grid).  into: a dict of uint64 arrays to accumulate into.  optional False:
    stops_pos_out and seq_out NULL."""
    prob = prob or RR.problem(case)
    n, L = prob.n, case['config']['total_laps']
    g = np.ascontiguousarray(O.Problem(case).grid_probs, np.float64) if state is None else None
    cs = RR.c_state(*state) if state is not None else None
    out = into if into is not None else {k: v.astype(np.uint64) for k, v in empty(n, L).items()}
    u64 = lambda k: out[k].ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_stints(C.byref(prob.cfg), C.byref(prob.drv),
                                 g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None,
                                 C.byref(cs) if cs is not None else None, n, int(n_sims), int(sim_offset), int(seed),
                                 device, u64('hist'), u64('stop_lap'), u64('stops_pos') if optional else None,
                                 u64('seq') if optional else None)
    return rc, {k: v.astype(np.int64) for k, v in out.items()}


def budget_sims(n, cap=0xFFFFFE00):
    """The staging budget of mcgp_run_stints: 256 MiB / (9 n) simulations, at most the launch cap, in multiples of 256
    when it can."""
    c = min(cap, max(1, (256 << 20) // (9 * n)))
    return c // 256 * 256 if c >= 256 else c


def chunk_sims(n, device_round):
    """The documented chunk rule: the budget, rounded down to whole rounds of the device (device_round = grid_blocks x
    block_threads of a full launch, mcgp_last_launch_info)."""
    c = budget_sims(n)
    return c // device_round * device_round if c >= device_round else c
