"""Penalty scenarios and trace references shared by the tests of mcgp_run_penalties on the host build
(test_penalties_host_build.py) and on the device (test_gpu_penalties_fuzz.py) over the inputs of generic_cases.py.

scenarios(): a deterministic generator of [(penalties, plans)] scaled to a case's field size n, lap count L and the first
lap with a pit step (2 from the grid, k + 1 from a state after lap k), seeded from the case's name by CRC-32 (not
Python's hash, which changes from process to process).

Two references that share no code with the kernels or with penalties_ref, both read from the CPU oracle's per-lap trace
(resume_ref.traced_run) of a race from the grid:

  trace_fates   nothing a penalty does changes when a car stops or retires (the rule stop depends on tyre age, laps
                remaining and events; retirement laps are shared by all scenarios), so the fate of a SERVE_AT_STOP
                penalty is a function of the trace: served if the car runs with age 0 after a lap >= max(pending, 2) --
                for a planned car, if it runs after a planned stop lap >= pending --, else retired or at the flag;
  flag_orders   the finishing orders of a scenario with AT_FLAG penalties only and no plans: the oracle's order with its
                running prefix sorted again by (time after lap L + seconds, grid slot), the retired tail as it is.

flag_tie(): the AT_FLAG penalty that puts the oracle's winner at exactly the time of its runner-up.

Nothing here looks at what the code under test returns."""
import zlib

import numpy as np

import generic_cases as G
import moves_ref as MR

SERVE, FLAG, LAP = 0, 1, 2                                          # MCGP_PEN_*
FATE_NONE, FATE_SERVED, FATE_FLAG, FATE_RETIRED = 0, 1, 2, 3
SECONDS = (0.5, 5.0, 10.0, 20.0)
# Inputs of generic_cases.run_inputs() on which no penalised scenario of scenarios() changes any of the first 8 finishing
# orders from the grid (simulations 3 .. 10, the host build's; at most 12 may be listed).  Over the first 16, which the
# device test runs, F09 leaves the list.
NO_BITE = {
    'F09': 'a three-car race over 22 laps, D00 at p = 0.2 a lap: the two survivors finish far apart',
    'F19': 'a five-car race over 78 laps: the cars finish minutes apart, no addition of seconds reorders them',
    'F27': 'a two-car wet race over 78 laps: the cars finish minutes apart or one retires',
    'F29': 'a three-car wet race over 57 laps, mostly decided by retirements (D01: p = 0.2 a lap)',
    'F52': 'a two-car race over 66 laps: the cars finish minutes apart, no addition of seconds reorders them',
    'F63': 'a five-car race over 44 laps with three cars at p = 0.03 a lap: the survivors finish minutes apart',
    'X_all_out_lap1': 'every car retires on lap 1: nobody runs where time is added',
    'n1': 'one car',
}


def _rng(name, first):
    return np.random.default_rng(zlib.crc32(f'penalties/{name}/{first}'.encode()))


def _shuffled(rng, pens):
    return [pens[j] for j in rng.permutation(len(pens))]


def flag_only(rng, n, dense):
    """AT_FLAG penalties: on about n / 3 drivers, or on every driver with seconds distinct per driver."""
    if dense:
        return _shuffled(rng, [(d, FLAG, 0, float(rng.choice(SECONDS)) + 0.125 * d) for d in range(n)])
    who = rng.choice(n, size=max(1, round(n / 3)), replace=False)
    return [(int(d), FLAG, 0, float(rng.choice(SECONDS))) for d in who]


def sparse(rng, n, L, first):
    """About n / 3 drivers, a random kind each, a random lap in [first, L], seconds from SECONDS."""
    who = rng.choice(n, size=max(1, round(n / 3)), replace=False)
    out = []
    for d in who:
        kind = int(rng.integers(3))
        out.append((int(d), kind, 0 if kind == FLAG else int(rng.integers(first, L + 1)), float(rng.choice(SECONDS))))
    return out


def dense(rng, n, L, first, pending=None):
    """Every driver: a serve penalty from a random lap in [first, L] (or pending[d]), a flag penalty, a lap addition on
    lap `first` and, if L > first, one on lap L -- all n drivers in one lap mask, every seconds value distinct."""
    pending = pending or {}
    out = []
    for d in range(n):
        out.append((d, SERVE, int(pending.get(d, rng.integers(first, L + 1))), 5.0 + 0.25 * d))
        out.append((d, FLAG, 0, 1.0 + 0.125 * ((5 * d + 3) % 32)))         # (odd factors: distinct for d < 32)
        out.append((d, LAP, first, 0.5 + 0.0625 * ((3 * d + 1) % 32)))
        if L > first:
            out.append((d, LAP, L, 2.0 + 0.03125 * ((7 * d + 2) % 32)))
    return _shuffled(rng, out)


def grid_plans(n, L):
    """Plans from generic_cases.grid_scenarios for the dense scenario from the grid, L >= 8: driver 0 stops once on lap
    max(2, L // 4); driver n - 1 (n >= 2) starts on aged HARD and stops once on lap L // 2; driver 1 (n >= 3) stops on
    laps L // 3 and L - 1.  -> (plans, pending): driver 0's penalty is pending from exactly its stop lap, driver
    n - 1's from the lap after its only stop."""
    scen = G.grid_scenarios(n, L)
    plans, pending = dict(scen[1]), {0: scen[1][0][2][0][0]}
    if n >= 3:
        plans.update(scen[2])
    if n >= 2:
        plans.update(scen[3])
        pending[n - 1] = scen[3][n - 1][2][0][0] + 1
    return plans, pending


def scenarios(name, n, L, first, from_state=False):
    """[(penalties, plans)] for a case called `name` of n cars and L laps whose first lap with a pit step is `first`:
    2 from the grid, k + 1 from a state after lap k (from_state).  first > L (a one-lap race from the grid, a state
    after lap L): empty, sparse flag, dense flag.  Else: empty, sparse, dense; and, where L >= 8, the dense scenario with
    plans -- from the grid grid_plans(), from a state after k with k + 2 < L generic_cases.state_scenarios' plans on the
    first and the last driver."""
    assert from_state or first == 2
    rng = _rng(name, f'{first}/{int(from_state)}')
    if first > L:
        return [([], {}), (flag_only(rng, n, False), {}), (flag_only(rng, n, True), {})]
    out = [([], {}), (sparse(rng, n, L, first), {}), (dense(rng, n, L, first), {})]
    if L >= G.MIN_STRATEGY_LAPS:
        if not from_state:
            plans, pending = grid_plans(n, L)
            out.append((dense(rng, n, L, first, pending), plans))
        elif first + 1 < L:
            out.append((dense(rng, n, L, first), G.state_scenarios(n, L, first - 1)[1]))
    return out


def flag_scenario(name, n):
    """AT_FLAG penalties on every driver, for a case whose scenarios() hold no flag-only scenario (first <= L)."""
    return flag_only(_rng(name, 0), n, True)


def sub_ref(ref, sims):
    """The oracle's traced run restricted to the simulations `sims` (a slice or an index array)."""
    return dict(trace={key: v[sims] for key, v in ref['trace'].items()}, orders=ref['orders'][sims],
                grids=ref['grids'][sims])


# ---------------------------------------------------------------- reference 1: fates from the oracle's trace
def trace_fates(ref, penalties, plans=None):
    """fates [m][n] of a scenario from the grid, from the oracle's trace of the same simulations alone."""
    plans = plans or {}
    tr = ref['trace']
    run, age = tr['dnf'] == 0, tr['age']
    m, L, n = age.shape
    fates = np.zeros((m, n), np.uint8)
    for d, kind, p, _ in penalties:
        if kind != SERVE:
            continue
        if d in plans:
            served = np.zeros(m, bool)
            for lap, _ in plans[d][2]:
                if lap >= p:
                    served |= run[:, lap - 1, d]
        else:
            lo = max(p, 2)
            served = (run[:, lo - 1:, d] & (age[:, lo - 1:, d] == 0)).any(axis=1)
        fates[:, d] = np.where(served, FATE_SERVED, np.where(run[:, L - 1, d], FATE_FLAG, FATE_RETIRED))
    return fates


# ---------------------------------------------------------------- reference 2: orders under flag penalties only
def flag_seconds(penalties, n):
    sec = np.zeros(n)
    for d, kind, _, s in penalties:
        assert kind == FLAG
        sec[d] = s
    return sec


def flag_orders(ref, sec):
    """Finishing orders [..., m][n] under AT_FLAG seconds sec [..., n] (0: none) and no plans, from the oracle's trace."""
    sec = np.asarray(sec, np.float64)
    tr, orders = ref['trace'], ref['orders'].astype(np.int64)
    m, n = orders.shape
    cum, run = tr['cum'][:, -1, :], tr['dnf'][:, -1, :] == 0
    slot = MR.slots_of(ref['grids'])
    rows = np.arange(m)[:, None]
    run_o, slot_o = run[rows, orders], slot[rows, orders]           # in the oracle's finishing order
    k = run.sum(axis=1)
    assert (run_o == (np.arange(n)[None, :] < k[:, None])).all()    # the running cars are its prefix
    t = cum + sec[..., None, :]                                     # [..., m][n] by driver
    t_o = np.take_along_axis(t, np.broadcast_to(orders, t.shape), axis=-1)
    primary = np.where(run_o, t_o, np.inf)
    secondary = np.broadcast_to(np.where(run_o, slot_o, np.arange(n)[None, :]), t.shape)
    perm = np.lexsort((secondary, primary), axis=-1)
    return np.take_along_axis(np.broadcast_to(orders, t.shape), perm, axis=-1).astype(np.uint8)


# ---------------------------------------------------------------- what a run from the grid must give, and what it shows
def grid_expectation(name, case, seed, ref, m, offset):
    """The scenarios of a case from the grid with the restatement's orders and fates of simulations offset .. offset +
    m - 1 (ref: the oracle's traced run of the same), checked here against both trace references, and what they show:
    dict(scen, orders [S][m][n], fates [S][m][n], bites, fates_seen {fate}, on_lap, early, red).
      bites    a penalised scenario changes a finishing order;
      on_lap   a penalty is served at a planned stop on exactly its pending lap (driver 0 of the planned scenario);
      early    a penalty stays unserved by a running car whose only planned stop was the lap before (driver n - 1);
      red      in the dense scenario a car that never stops runs through a red flag on a lap >= its pending lap, and its
               penalty is not served."""
    import penalties_ref as PR
    import stints_ref as ST
    n, L = len(case['grid_probs']), case['config']['total_laps']
    scen = scenarios(name, n, L, 2)
    tr = ref['trace']
    run = tr['dnf'] == 0
    orders, fates = [ref['orders'][:m]], [np.zeros((m, n), np.uint8)]
    for pens, plans in scen[1:]:
        o, f = PR.orders(case, m, seed, offset, plans=plans, penalties=pens, grids=ref['grids'])
        assert np.array_equal(f, trace_fates(ref, pens, plans)), name                   # reference 1
        if not plans and all(kind == FLAG for _, kind, _, _ in pens):
            assert np.array_equal(o, flag_orders(ref, flag_seconds(pens, n))), name     # reference 2
        orders.append(o)
        fates.append(f)
    orders, fates = np.stack(orders), np.stack(fates)
    out = dict(scen=scen, orders=orders, fates=fates, bites=bool((orders[1:] != orders[0]).any()),
               fates_seen={int(x) for x in np.unique(fates)} - {FATE_NONE}, on_lap=False, early=False, red=False)
    if len(scen) == 4 and scen[3][1]:
        pens, plans = scen[3]
        out['on_lap'] = bool((fates[3][:, 0] == FATE_SERVED).any())
        if n >= 2:
            stop = plans[n - 1][2][0][0]
            pending = [lap for d, kind, lap, _ in pens if d == n - 1 and kind == SERVE][0]
            assert pending == stop + 1 and len(plans[n - 1][2]) == 1
            out['early'] = bool((run[:, stop - 1, n - 1] & (fates[3][:, n - 1] != FATE_SERVED)).any())
    if L >= 2:
        red = ST.red_flags(case, seed, offset + np.arange(m), L)                        # [m][L], lap k + 1 at k
        stopped = (run[:, 1:, :] & (tr['age'][:, 1:, :] == 0)).any(axis=1)              # [m][n]
        for d, kind, p, _ in scen[2][0]:
            if kind == SERVE:
                through = (red[:, p - 1:] & run[:, p - 1:, d]).any(axis=1)
                out['red'] |= bool((through & ~stopped[:, d] & (fates[2][:, d] != FATE_SERVED)).any())
    return out


# ---------------------------------------------------------------- the tie at the flag
def flag_tie(ref, i):
    """Traced simulation i's (a, b, delta, flips) or None: a and b the oracle's first and second, both running, with
    final times t_a < t_b and delta = t_b - t_a exact, so that t_a + delta == t_b bit for bit (asserted): an AT_FLAG
    penalty of delta on a ties them, and b wins exactly when its grid slot is the better one (flips)."""
    tr, o = ref['trace'], ref['orders'][i]
    if len(o) < 2:
        return None
    a, b = int(o[0]), int(o[1])
    if tr['dnf'][i, -1, a] or tr['dnf'][i, -1, b]:
        return None
    ta, tb = float(tr['cum'][i, -1, a]), float(tr['cum'][i, -1, b])
    delta = tb - ta
    if not 0.0 < delta <= 1e6:
        return None
    assert ta + delta == tb, (i, ta, tb)
    slot = MR.slots_of(ref['grids'][i:i + 1])[0]
    return a, b, delta, bool(slot[b] < slot[a])


def flag_ties(case, seed, m, offset):
    """([(i, penalties, order)], flips, keeps): for every simulation offset + i, i < m, that flag_tie can use, the one
    AT_FLAG penalty that ties its first two and the finishing order under it -- the restatement's, which must be
    flag_orders' and must have the tied pair in grid-slot order in front; and how many of them swap the pair."""
    import penalties_ref as PR
    import resume_ref as RR
    ref = RR.traced_run(case, m, seed, offset)
    n = len(case['grid_probs'])
    out, flips = [], 0
    for i in range(m):
        tie = flag_tie(ref, i)
        if tie is None:
            continue
        a, b, delta, flip = tie
        pens = [(a, FLAG, 0, delta)]
        want, _ = PR.orders(case, 1, seed, offset + i, penalties=pens, grids=ref['grids'][i:i + 1])
        assert np.array_equal(want, flag_orders(sub_ref(ref, slice(i, i + 1)), flag_seconds(pens, n))), i
        assert tuple(want[0][:2]) == ((b, a) if flip else (a, b)), i
        out.append((i, pens, want[0]))
        flips += flip
    return out, flips, len(out) - flips
