"""Calls for the tests of mcgp_run_weather at its limits, generated from a case's shape and seeded through
weather_cases.scenarios by CRC-32 of the case's name: nothing here looks at what the code under test returns (the
*_wanted functions hand the calls and the restatement's results to the caller's comparison and read their counts from the
restatement alone).  A call is (table, [(changes, plans)]) as weather_ref takes it.

  tables   on the 8 golden inputs and the 12 X_ fuzz cases, from the grid: the planned and the cross-back scenario of
           weather_cases.scenarios under the 15 tables with one non-zero cell each, a checkerboard table and a
           table holding 60.0 and 5e-324 (WeatherPace::base reads one `live` bit per compound);
  limits   64 scenarios of 64 single-lap changes each on 32 cars over 70 laps (the conditions cycle DAMP, DRY, WET, every
           scenario starts the cycle on another lap, the odd ones carry plans of 8 stops on all 32 drivers); a 1000-lap race
           on 3 cars that cannot retire, one of them planned onto WET without a stop on a dry track, one under the rule,
           under 64 changes spread over the race; a one-lap race with every driver started on intermediates; X_all_out_lap1
           with every driver started on intermediates; a damp race that is wet on every later lap under 24 single-lap
           changes, with every driver planned onto dry tyres without a stop;
  states   on the same 20 inputs from the oracle's state after laps 1, L - 1 and L: the scenarios of
           weather_cases.scenarios(name, case, first=k + 1), which after lap L is the empty list;
  F33      a copy of F33 under 64 scenarios for the counting kernel's loops: the even ones put every driver under a plan,
           so that the laps on the wrong tyres have a closed form from the oracle's trace (trace_wrong_laps); the odd ones
           run under the rule;
  budget   64 scenarios on 32 cars over 3 laps for the call just past its staging budget."""
import copy
import functools

import numpy as np

import generic_cases as G
import oracle_py as O
import resume_ref as RR
import weather_cases as WC
import weather_ref as WR

DRY, DAMP, WET_TRACK = WR.DRY, WR.DAMP, WR.WET_TRACK
FUZZ_SIMS, FUZZ_OFFSET = WC.FUZZ_SIMS, WC.FUZZ_OFFSET
MAX_SCENARIOS, MAX_CHANGES = 64, 64
FULL = WC.FULL_TABLE

ONE_CELL = [[[FULL[c][k] if (c, k) == (cc, kk) else 0.0 for k in range(5)] for c in range(3)]
            for cc in range(3) for kk in range(5)]
CHECKER = [[FULL[c][k] if (c + k) % 2 == 0 else 0.0 for k in range(5)] for c in range(3)]
EXTREME = [[60.0 if (c + k) % 2 else 5e-324 for k in range(5)] for c in range(3)]
TABLES = ONE_CELL + [CHECKER, EXTREME]
assert len(TABLES) == 17 and all(sum(x != 0.0 for row in t for x in row) == 1 for t in ONE_CELL)


@functools.lru_cache(maxsize=None)
def corners():
    """[((name, case, seed), the oracle's traced run)] of the golden and the X_ inputs."""
    inputs, refs = WC.fuzz_inputs()
    names = set(G.GOLDEN) | {name for name in G.fuzz_cases() if name.startswith('X_')}
    picked = [(inp, ref) for inp, ref in zip(inputs, refs) if inp[0] in names]
    assert len(picked) == 20
    return picked


def restate(case, seed, table, scen, m, offset, **kw):
    want = [WR.orders(case, m, seed, offset, plans=pl, changes=ch, table=table, **kw) for ch, pl in scen]
    return np.stack([w[0] for w in want]), np.stack([w[1] for w in want])


# ---------------------------------------------------------------- tables
TABLE_PARTS = 10
# Inputs (of 20) on which, by weather_ref alone, a table with one non-zero cell moved a finishing order against the zero
# table's.  Measured with weather_ref on the CPU; the floor is about a tenth below.
TABLES_MEASURED, TABLES_FLOOR = 19, 17


def _restate_under_tables(case, seed, scen, grids):
    """[(orders [S][m][n], wrong laps [S][m][n])] under the zero table and then TABLES.  The restatement reads a table
    only in the rows of the conditions a scenario's laps have, so a scenario is run once for every distinct content of
    those rows (under a one-cell table of another condition it is the zero table's run, addition for addition)."""
    track = {'dry': DRY, 'damp': DAMP, 'wet': WET_TRACK}[case.get('track_condition', 'dry')]
    L = case['config']['total_laps']
    done, out = {}, []
    for table in [WR.ZERO_TABLE] + TABLES:
        runs = []
        for s, (ch, pl) in enumerate(scen):
            key = (s,) + tuple((c, tuple(table[c])) for c in sorted(set(WR.conditions(track, ch, L)[1:])))
            if key not in done:
                done[key] = WR.orders(case, FUZZ_SIMS, seed, FUZZ_OFFSET, plans=pl, changes=ch, table=table, grids=grids)
            runs.append(done[key])
        out.append((np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs])))
    return out


@functools.lru_cache(maxsize=None)
def table_wanted(part):
    """[(name, case, seed, [(table, scen, orders, wrong laps)])] of slice `part` and the inputs on which a one-cell table
    moved an order."""
    out, moved = [], 0
    for (name, case, seed), ref in corners()[part::TABLE_PARTS]:
        sets = WC.scenarios(name, case)
        scen = sets[1][1][1:] if len(sets) > 1 else sets[0][1]      # planned, cross-back; a one-lap race: the empty one
        (base, _), *wants = _restate_under_tables(case, seed, scen, ref['grids'])
        calls = [(table, scen, want_o, want_w) for table, (want_o, want_w) in zip(TABLES, wants)]
        out.append((name, case, seed, calls))
        moved += any(not np.array_equal(want_o, base) for _, _, want_o, _ in calls[:len(ONE_CELL)])
    return out, moved


def tables_moved():
    return sum(table_wanted(p)[1] for p in range(TABLE_PARTS))


# ---------------------------------------------------------------- limits
def _field(n, laps, no_retirements=False):
    case = RR.field_case(n)
    case['config'] = dict(case['config'], total_laps=laps)
    if no_retirements:
        case['config'] = dict(case['config'], red_flag_probability=0.0, dnf_rates={t: 0.0 for t in case['config']['dnf_rates']})
        case['driver_dnf_rates'] = {d: 0.0 for d in case['driver_dnf_rates']}
    return case


def scenario_limit():
    n, L = 32, 70
    scen = []
    for s in range(MAX_SCENARIOS):
        changes = [(2 + (s + j) % (L - 1),) * 2 + ((DAMP, DRY, WET_TRACK)[j % 3],) for j in range(MAX_CHANGES)]
        plans = {}
        if s % 2:
            plans = {d: ((d + s) % 5, 0, [(2 + (d + s) % 5 + 8 * j, (d + s + j) % 5) for j in range(8)]) for d in range(n)}
        scen.append((changes, plans))
    assert all(len({a for a, _, _ in ch}) == MAX_CHANGES and max(b for _, b, _ in ch) <= L for ch, _ in scen)
    assert all(len(p[2]) == 8 and p[2][-1][0] <= L for _, pl in scen for p in pl.values())
    return 'sixty-four scenarios of sixty-four changes', _field(n, L), 13, FULL, scen, 2, 3


def thousand_laps():
    """Driver 0 on WET without a stop, driver 1 under the rule, driver 2 on a plan of dry tyres.  Scenario 1's 64 changes
    all name DRY (legal, and they change nothing): driver 0 is on the wrong tyres on every one of the 1000 laps.  Scenario
    2's alternate DAMP and WET_TRACK on single laps spread over the race."""
    L = 1000
    laps = [2 + 15 * j for j in range(MAX_CHANGES)]
    assert laps[-1] <= L
    plans = {0: (WR.WET, 0, []), 2: (WR.MEDIUM, 0, [(400, WR.HARD), (800, WR.SOFT)])}
    scen = [([], {}), ([(lap, lap, DRY) for lap in laps], plans),
            ([(lap, lap, (DAMP, WET_TRACK)[j % 2]) for j, lap in enumerate(laps)], plans)]
    return 'a thousand laps', _field(3, L, no_retirements=True), 47, FULL, scen, FUZZ_SIMS, 1


def one_lap(n):
    plans = {d: (WR.INTER, 0, []) for d in range(n)}
    return f'one lap, {n} cars', _field(n, 1), 5, FULL, [([], {}), ([], plans)], 40, 5


def all_out_lap1():
    case = copy.deepcopy(G.fuzz_cases()['X_all_out_lap1'])
    n, L = len(case['grid_probs']), case['config']['total_laps']
    plans = {d: (WR.INTER, 0, []) for d in range(n)}
    return 'all out on lap 1', case, case['seed'], FULL, [([], {}), ([], plans), ([(2, L, DAMP)], plans)], FUZZ_SIMS, FUZZ_OFFSET


def wrong_class_every_lap(n):
    """A damp race of 25 laps, wet from lap 2 under 24 single-lap changes that alternate WET_TRACK and DAMP, with every
    driver planned onto dry tyres without a stop: a car that sees the flag without a red flag was on the wrong tyres on all
    L laps, lap 1 included, which is the only way into column L."""
    case = _field(n, 25)
    case['track_condition'] = 'damp'
    L = 25
    changes = [(lap, lap, (WET_TRACK, DAMP)[lap % 2]) for lap in range(2, L + 1)]
    plans = {d: (d % 3, 0, []) for d in range(n)}
    return f'the wrong class on every lap, {n} cars', case, 5, FULL, [([], {}), (changes, plans), (changes, {})], FUZZ_SIMS, FUZZ_OFFSET


LIMITS = (scenario_limit, thousand_laps, lambda: one_lap(3), lambda: one_lap(32), all_out_lap1,
          lambda: wrong_class_every_lap(3), lambda: wrong_class_every_lap(32))
# Cells (scenario, simulation, driver) of the limit calls whose car was on the wrong tyres on all L laps (column L of
# wrong_laps), by weather_ref alone.  Measured with weather_ref on the CPU; the floor is about a tenth below.
COLUMN_L_MEASURED, COLUMN_L_FLOOR = 1612, 1450


@functools.lru_cache(maxsize=None)
def limit_wanted(k):
    """(label, case, seed, table, scen, m, offset, orders, wrong laps) of limit call k."""
    label, case, seed, table, scen, m, offset = LIMITS[k]()
    want_o, want_w = restate(case, seed, table, scen, m, offset)
    return label, case, seed, table, scen, m, offset, want_o, want_w


def column_l_cells():
    return sum(int((limit_wanted(k)[8] == limit_wanted(k)[1]['config']['total_laps']).sum()) for k in range(len(LIMITS)))


# ---------------------------------------------------------------- states after the first and the last laps
STATE_PARTS = 5


@functools.lru_cache(maxsize=None)
def state_wanted(part):
    """[(name, case, seed, k, state, [(table, scen, orders, wrong laps)])] of slice `part`: the state of simulation
    FUZZ_OFFSET after k in {1, L - 1, L} (less max(1, L // 2), which weather_cases.state_wanted has), continued as
    simulations 0 .. FUZZ_SIMS - 1."""
    out = []
    for (name, case, seed), ref in corners()[part::STATE_PARTS]:
        L = case['config']['total_laps']
        for k in sorted({1, max(1, L - 1), L} - {max(1, L // 2)}):
            state = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, FUZZ_OFFSET, k))
            sets = WC.scenarios(name, case, first=k + 1)
            assert k < L or sets == [(None, [([], {})])]
            calls = [(table, scen) + restate(case, seed, table, scen, FUZZ_SIMS, 0, state=state) for table, scen in sets]
            out.append((name, case, seed, k, state, calls))
    return out


# ---------------------------------------------------------------- F33 under 64 scenarios, for the counting loops
def f33():
    case = copy.deepcopy(G.fuzz_cases()['F33'])
    case['config']['red_flag_probability'] = 0.0            # no free tyre change: a planned car's compounds are its plan's
    assert (len(case['grid_probs']), case['config']['total_laps'], case.get('track_condition', 'dry')) == (20, 9, 'dry')
    return case, case['seed']


def f33_scenarios(n=20, L=9):
    """Even: every driver under a plan (a start compound and 0, 1 or 2 stops, all varying with the scenario) and one
    change; odd: nobody planned, one change for the rule to react to."""
    scen = []
    for s in range(MAX_SCENARIOS):
        h = s // 2
        a = 2 + h % 4
        change = [(a, min(L, a + s % 5), (DAMP, WET_TRACK)[h % 2])]
        plans = {}
        if s % 2 == 0:
            for d in range(n):
                first = 2 + (d + s) % 4
                stops = [(first, (d + h + 1) % 5), (first + 1 + d % 3, (d + h + 3) % 5)][:(d + h) % 3]
                plans[d] = ((d + h) % 5, 0, stops)
        scen.append((change if s else [], plans))
    return scen


def trace_wrong_laps(ref, scen, track, L):
    """Laps on the wrong tyres [S][m][n] of scenarios that plan every driver, in a race without red flags, from the
    oracle's trace of the same simulations alone: the compound on every lap is the plan's, retirement laps are shared by
    all scenarios, so the count is the sum of wrong(c_k, compound before lap k's stop) over lap 1 to the car's last
    timed lap."""
    tr = ref['trace']
    out_lap = np.where(tr['dnf'][:, L - 1, :] != 0, tr['dnf_lap'][:, L - 1, :], 0)         # [m][n], 0: runs to the flag
    last = np.where(out_lap != 0, out_lap - 1, L)
    m, n = last.shape
    out = np.zeros((len(scen), m, n), np.int64)
    for s, (changes, plans) in enumerate(scen):
        cond = WR.conditions(track, changes, L)
        assert len(plans) == n
        for d, (comp, _, stops) in plans.items():
            stop = dict(stops)
            upto = [0]                                      # upto[k]: wrong laps among laps 1 .. k
            for lap in range(1, L + 1):
                upto.append(upto[-1] + WR.wrong(cond[lap], comp))
                comp = stop.get(lap, comp)
            out[s, :, d] = np.asarray(upto)[last[:, d]]
    return out


# ---------------------------------------------------------------- the call just past its staging budget
def budget_call():
    """(case, seed, table, 64 scenarios) on 32 cars over 3 laps: a change on lap 2, lap 3 or both (in every eighth to
    DRY, which changes nothing), and in every fourth scenario all drivers started on tyres that vary with the driver, so
    that some are on the wrong tyres on all three laps."""
    n, L = 32, 3
    scen = [([], {})]
    for s in range(1, MAX_SCENARIOS):
        a = 2 + s % 2
        plans = {d: ((d + s) % 5, 0, [(3, (d + 1) % 5)] if d % 2 else []) for d in range(n)} if s % 4 == 0 else {}
        scen.append(([(a, L if s % 3 else a, DRY if s % 8 == 0 else 1 + (s // 2) % 2)], plans))
    return _field(n, L), 9, FULL, scen
