"""numpy restatement of mcgp_run_conditions (include/mcgp.h, csrc/conditions.hip.h): the nine facts of every simulation from
the CPU oracle's run of the same simulations (resume_ref.traced_run: positions from `orders`, slots from `grids`,
retirement laps from the trace's dnf / dnf_lap after the last lap, events from trace_ref.lap_event_kind), the masks and
the counts from those facts.  For many simulations from one state -- for which the oracle has no entry point -- the facts
come from the Python restatement strategy_ref._Race, as gaps_ref.restated_* do.  Also the C-ABI call for the tests, and
the choice of the conditions a test compares: candidates are generated from a seed and kept only if the REFERENCE shows
them met by at least one and by fewer than all simulations, so no comparison is between two constant columns.  Nothing
here shares code with the kernel or with the product's parser: a condition is a list of (fact, a, b, lo, hi, negate)."""
import ctypes as C

import numpy as np

import gaps_ref as GR
import generic_cases as G
import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
import trace_ref as TR
from monte_carlo_gp_amd import _native as N

POSITION, GRID, RETIRED_LAP, AHEAD_BY, GAINED, FINISHERS, RED_FLAGS, SAFETY_CARS, VSCS = range(9)
FACT_NAMES = ('position', 'grid', 'retired_lap', 'ahead_by', 'gained', 'finishers', 'red_flags', 'safety_cars', 'vscs')
LO, HI = -2 ** 31, 2 ** 31 - 1
ALWAYS = [(FINISHERS, 0, 0, 0, HI, 0)]                   # finishers >= 0
NEVER = [(FINISHERS, 0, 0, LO, -1, 0)]                   # finishers < 0
EMPTY = []                                               # no atom: always holds


# ---------------------------------------------------------------- facts
def event_counts(case, seed, sims, first_lap=2):
    """[m][3]: red flags, safety cars, VSCs of laps first_lap .. L of the simulation ids `sims`."""
    L = case['config']['total_laps']
    out = np.zeros((len(sims), 3), np.int64)
    for i, sim in enumerate(sims):
        for lap in range(first_lap, L + 1):
            kind = TR.lap_event_kind(case, seed, int(sim), lap)
            if kind is not None:
                out[i, kind] += 1
    return out


def facts_of(orders, slot, retired, events):
    """The facts of m simulations: orders [m][n] (driver classified p-th), slot [m][n] (0-based grid slot by driver),
    retired [m][n] (lap of retirement or 0), events [m][3]."""
    orders = np.asarray(orders).astype(np.int64)
    m, n = orders.shape
    pos = np.zeros((m, n), np.int64)
    pos[np.arange(m)[:, None], orders] = np.arange(1, n + 1)[None, :]
    retired = np.asarray(retired, np.int64)
    return dict(pos=pos, grid=np.asarray(slot, np.int64) + 1, out=retired, finishers=(retired == 0).sum(axis=1),
                events=np.asarray(events, np.int64), orders=orders)


def oracle_facts(case, m, seed, sim_offset=0, ref=None, sims=None, lap0=0):
    """The facts of the oracle's simulations sim_offset + [0, m) (or of the traced simulations `sims` of `ref`); lap0 > 0:
    as resumed after lap lap0 as themselves -- the same race, events counted from lap lap0 + 1."""
    ref = ref or RR.traced_run(case, m, seed, sim_offset)
    idx = np.arange(m) if sims is None else np.asarray(sims)
    tr = ref['trace']
    L = case['config']['total_laps']
    retired = np.where(tr['dnf'][idx, L - 1] != 0, tr['dnf_lap'][idx, L - 1], 0)
    ev = event_counts(case, seed, sim_offset + idx, first_lap=max(2, lap0 + 1))
    return facts_of(ref['orders'][idx], GR.slots_of(ref['grids'][idx]), retired, ev)


def restated_facts(case, m, seed, sim_offset=0, state=None, grids=None):
    """The facts of m simulations from the grid or from state = (arrays, lap, drs_disabled_until), from strategy_ref._Race."""
    M = SR.Model(case)
    n = M.n
    if state is None and grids is None:
        grids = RR.traced_run(case, m, seed, sim_offset)['grids']
    orders, slot, retired = np.zeros((m, n), np.int64), np.zeros((m, n), np.int64), np.zeros((m, n), np.int64)
    for i in range(m):
        r = SR._Race(M, seed, sim_offset + i)
        first, dd = r.start_grid(grids[i], {}) if state is None else r.start_state(*state)
        r.laps(first, dd, {})
        orders[i], slot[i], retired[i] = r.classify(), r.gpos, r.dnf
    ev = event_counts(case, seed, sim_offset + np.arange(m), first_lap=2 if state is None else int(state[1]) + 1)
    return facts_of(orders, slot, retired, ev)


# ---------------------------------------------------------------- evaluation
def value(facts, fact, a, b):
    if fact == POSITION:
        return facts['pos'][:, a]
    if fact == GRID:
        return facts['grid'][:, a]
    if fact == RETIRED_LAP:
        return facts['out'][:, a]
    if fact == AHEAD_BY:
        return facts['pos'][:, b] - facts['pos'][:, a]
    if fact == GAINED:
        return facts['grid'][:, a] - facts['pos'][:, a]
    if fact == FINISHERS:
        return facts['finishers']
    return facts['events'][:, fact - RED_FLAGS]


def holds(facts, cond):
    """bool [m]: the conjunction of the atoms (fact, a, b, lo, hi, negate)."""
    ok = np.ones(len(facts['pos']), bool)
    for fact, a, b, lo, hi, negate in cond:
        v = value(facts, fact, a, b)
        ok &= ((lo <= v) & (v <= hi)) != bool(negate)
    return ok


def met(facts, conds):
    """bool [m][C]."""
    return np.stack([holds(facts, c) for c in conds], axis=1)


def masks(facts, conds):
    """u64 [m]: bit c = condition c holds."""
    out = np.zeros(len(facts['pos']), np.uint64)
    for c, cond in enumerate(conds):
        out |= holds(facts, cond).astype(np.uint64) << np.uint64(c)
    return out


def counts(facts, conds):
    """dict(hist [n][n], count [C], cond_hist [C][n][n]) of the simulations."""
    orders = facts['orders']
    n = orders.shape[1]
    out = dict(hist=RR.counts(orders, n), count=np.zeros(len(conds), np.int64),
               cond_hist=np.zeros((len(conds), n, n), np.int64))
    for c, cond in enumerate(conds):
        h = holds(facts, cond)
        out['count'][c] = h.sum()
        out['cond_hist'][c] = RR.counts(orders[h], n)
    return out


def counts_each(facts, conds):
    """masks() and counts() of every simulation on its own, for runs of one simulation each: dict(masks [m], hist
    [m][n][n], count [m][C], cond_hist [m][C][n][n])."""
    orders = facts['orders']
    m, n = orders.shape
    hist = np.zeros((m, n, n), np.int64)
    hist[np.arange(m)[:, None], orders, np.arange(n)[None, :]] = 1
    count = met(facts, conds).astype(np.int64)
    return dict(masks=masks(facts, conds), hist=hist, count=count, cond_hist=count[:, :, None, None] * hist[:, None, :, :])


def informative(facts, conds):
    """bool [C]: met by at least one and by fewer than all simulations."""
    k = met(facts, conds).sum(axis=0)
    return (k >= 1) & (k < len(facts['pos']))


def assert_informative(facts, conds, constant=()):
    """Every condition is met by some and not by all simulations of the reference, except those at the indices `constant`
    (the deliberate always / never cases), which must be constant."""
    inf = informative(facts, conds)
    for c in range(len(conds)):
        assert inf[c] != (c in constant), (c, conds[c], int(holds(facts, conds[c]).sum()), len(facts['pos']))


# ---------------------------------------------------------------- the conditions a test compares
def simple_candidates(n, L):
    """One- to three-atom conditions over every fact, for a field of n."""
    ds = sorted({0, 1 % n, n // 2, n - 1})
    out = []
    for d in ds:
        out += [[(POSITION, d, 0, 1, 1, 0)], [(POSITION, d, 0, 1, 3, 0)], [(POSITION, d, 0, 1, 10, 0)],
                [(POSITION, d, 0, 1, max(1, n // 2), 1)], [(GRID, d, 0, 1, 1, 0)], [(GRID, d, 0, 1, max(1, n // 2), 0)],
                [(RETIRED_LAP, d, 0, 1, HI, 0)], [(RETIRED_LAP, d, 0, 0, 0, 0)], [(RETIRED_LAP, d, 0, 1, 1, 0)],
                [(RETIRED_LAP, d, 0, 2, max(2, L // 2), 0)], [(GAINED, d, 0, 1, HI, 0)], [(GAINED, d, 0, 3, HI, 0)],
                [(GAINED, d, 0, LO, -1, 0)], [(GAINED, d, 0, 0, 0, 1)]]
        for e in ds:
            if e != d:
                out += [[(AHEAD_BY, d, e, 1, HI, 0)], [(AHEAD_BY, d, e, -2, 2, 0)],
                        [(POSITION, d, 0, 1, 1, 0), (POSITION, e, 0, 1, 3, 0)],
                        [(RETIRED_LAP, d, 0, 0, 0, 0), (RETIRED_LAP, e, 0, 0, 0, 0), (AHEAD_BY, e, d, 1, HI, 0)]]
    for k in (n, n - 1, n - 2, n - 4):
        out += [[(FINISHERS, 0, 0, LO, k, 0)], [(FINISHERS, 0, 0, k, k, 0)]]
    for f in (RED_FLAGS, SAFETY_CARS, VSCS):
        out += [[(f, 0, 0, 1, HI, 0)], [(f, 0, 0, 0, 0, 0)], [(f, 0, 0, 1, 1, 0)], [(f, 0, 0, 2, HI, 0)],
                [(f, 0, 0, 1, HI, 0), (POSITION, 0, 0, 1, max(1, n // 2), 0)]]
    out += [[(SAFETY_CARS, 0, 0, 1, HI, 0), (VSCS, 0, 0, 1, HI, 1), (FINISHERS, 0, 0, LO, n - 1, 0)]]
    return out


def wide_candidates(n, L, rng, count, n_atoms=8):
    """`count` conditions of n_atoms atoms each with wide ranges, so that a conjunction of eight is still met sometimes;
    generated one by one as they are asked for, so that pick() pays only for the candidates it looks at."""
    for _ in range(count):
        cond = []
        for _ in range(n_atoms):
            f = int(rng.integers(0, 9))
            a = int(rng.integers(0, n))
            b = int((a + 1 + rng.integers(0, max(1, n - 1))) % n) if n > 1 else 0
            if f == AHEAD_BY and n == 1:
                f = POSITION
            if f in (POSITION, GRID):
                cut = int(rng.integers(1, n + 1))
                lo, hi = (1, cut) if rng.random() < 0.5 else (cut, n)
                if rng.random() < 0.7:                      # widen: most simulations pass
                    lo, hi = (1, max(hi, (3 * n + 3) // 4)) if lo == 1 else (min(lo, (n + 3) // 4), n)
            elif f == RETIRED_LAP:
                lo, hi = ((0, 0), (0, int(rng.integers(1, L + 1))), (int(rng.integers(1, L + 1)), HI))[int(rng.integers(0, 3))]
            elif f == AHEAD_BY:
                lo, hi = ((1, HI), (LO, -1), (-(n // 2) - 1, n))[int(rng.integers(0, 3))]
            elif f == GAINED:
                lo, hi = ((-(n // 2), n), (0, HI), (LO, 0), (-2, 2))[int(rng.integers(0, 4))]
            elif f == FINISHERS:
                lo, hi = ((n - int(rng.integers(0, 5)), HI), (LO, n - int(rng.integers(0, 3))))[int(rng.integers(0, 2))]
            else:
                lo, hi = ((0, 0), (0, 1), (1, HI), (0, 3))[int(rng.integers(0, 4))]
            negate = int(rng.random() < 0.15)
            cond.append((f, a, b if f == AHEAD_BY else 0, int(lo), int(hi), negate))
        yield cond


def pick(facts, candidates, most=64):
    """The informative candidates, in order, at most `most`, duplicates (same truth column) dropped."""
    keep, seen = [], set()
    for cond in candidates:
        h = holds(facts, cond)
        if 1 <= h.sum() < len(h) and h.tobytes() not in seen:
            seen.add(h.tobytes())
            keep.append(cond)
            if len(keep) == most:
                break
    return keep


def choose(facts, n, L, seed, most=61, wide=600):
    """(conditions, indices of the constant ones): informative simple and eight-atom conditions chosen on the reference's
    facts (`wide` eight-atom candidates from default_rng(seed)), then the empty condition, an always-true and an
    always-false bound."""
    rng = np.random.default_rng(seed)
    simple = pick(facts, simple_candidates(n, L), most // 2)
    conds = simple + pick(facts, wide_candidates(n, L, rng, wide), most - len(simple))
    k = len(conds)
    return conds + [EMPTY, ALWAYS, NEVER], (k, k + 1, k + 2)


def state_runs(case, seed, ref, sims, base):
    """[(i, k, state)]: the traced simulations `sims` of ref (simulation ids base + i) after every lap of
    generic_cases.resume_laps, as (mcgp_race_state arrays, lap, drs_disabled_until)."""
    return [(i, k, (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k)))
            for i in sims for k in G.resume_laps(case, seed, base + i)]


def concat(parts):
    """The facts of several runs as one."""
    return {key: np.concatenate([p[key] for p in parts], axis=0) for key in parts[0]}


def facts_used(conds):
    return {FACT_NAMES[a[0]] for c in conds for a in c}


# ---------------------------------------------------------------- the C ABI
def c_conditions(conds):
    arr = (N.McgpCondition * max(len(conds), 1))()
    for c, cond in enumerate(conds):
        arr[c].n_atoms = len(cond)
        for k, at in enumerate(cond[:N.MAX_CONDITION_ATOMS]):
            arr[c].atom[k] = N.McgpConditionAtom(*[int(x) for x in at])
    return arr


def empty(n, C_):
    return dict(hist=np.zeros((n, n), np.int64), count=np.zeros(C_, np.int64), cond_hist=np.zeros((C_, n, n), np.int64))


def run_c(case, conds, n_sims, seed, sim_offset=0, state=None, device=0, prob=None, cond_hist=True, into=None,
          table=None):
    """mcgp_run_conditions on a case -> (rc, counts dict as counts() returns; cond_hist stays as passed when cond_hist is
    False).  state = (mcgp_race_state arrays, lap, drs_disabled_until) or None (from the grid).  into: a dict of uint64
    arrays to accumulate into.  table: c_conditions(conds), where a caller makes many calls with the same conditions."""
    prob = prob or RR.problem(case)
    n = prob.n
    g = np.ascontiguousarray(O.Problem(case).grid_probs, np.float64) if state is None else None
    cs = RR.c_state(*state) if state is not None else None
    table = table if table is not None else c_conditions(conds)
    out = into if into is not None else {k: v.astype(np.uint64) for k, v in empty(n, len(conds)).items()}
    u64 = lambda k: out[k].ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_conditions(C.byref(prob.cfg), C.byref(prob.drv),
                                     g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None,
                                     C.byref(cs) if cs is not None else None, n, len(conds), table,
                                     int(n_sims), int(sim_offset), int(seed), device, u64('hist'), u64('count'),
                                     u64('cond_hist') if cond_hist else None)
    return rc, {k: v.astype(np.int64) for k, v in out.items()}


def budget_sims(n, cap=0xFFFFFE00):
    """The staging budget of mcgp_run_conditions: 256 MiB / (n + 8) simulations, at most the launch cap, in multiples of
    256 when it can."""
    c = min(cap, max(1, (256 << 20) // (n + 8)))
    return c // 256 * 256 if c >= 256 else c


def chunk_sims(n, device_round):
    """The documented chunk rule: the budget, rounded down to whole rounds of the device (device_round = grid_blocks x
    block_threads of a full launch, mcgp_last_launch_info)."""
    c = budget_sims(n)
    return c // device_round * device_round if c >= device_round else c
