"""Scenario sets for the tests of mcgp_run_weather, generated from a case's shape (field size, laps, first lap a change
may name, track condition) and seeded by CRC-32 of the case's name: the generator looks at nothing the code under test
returns (grid_wanted and state_wanted, below, hand the sets and the restatement's results to the caller's comparison and
read their three counts from the restatement alone).  scenarios() gives the calls of one input, [(table, [(changes,
plans)])] as weather_ref takes them; `other` is the condition of the other class (DAMP on a dry track, DRY on a damp or
wet one):

  call 0, a zero table (so scenario 0 is mcgp_run's race):
    the empty scenario; a change to the case's own condition over every lap; `other` to the flag from the lap with
    remaining == 6 and, in another scenario, from the lap with remaining == 5 (the two sides of the rule's guard); a single
    changed lap; DAMP and then WET_TRACK (one class); `other` for a while and then the case's condition again (the
    cross-back: on a dry track the rule's two-compound choice after the rain, with either side of remaining > 20 over the
    inputs); driver 0 planned to stop for the right tyres on the lap the condition changes, beside the last driver under a
    plan without stops, who stays out to the flag or to its retirement;
  call 1, a table with a different non-zero entry in every cell:
    the empty scenario; the planned scenario; the cross-back.

A scenario whose laps the race does not have (L < first, or L - 6 < first) is left out."""
import functools
import zlib

import numpy as np

import generic_cases as G
import paces_cases as PC
import resume_ref as RR
import strategy_ref as SR
import weather_ref as WR

FULL_TABLE = [[round(0.21 + 0.9 * c + 0.17 * k + 0.013 * c * k, 3) for k in range(5)] for c in range(3)]
assert len({x for row in FULL_TABLE for x in row}) == 15 and min(min(row) for row in FULL_TABLE) > 0


def scenarios(name, case, first=2):
    n, L = len(case['grid_probs']), case['config']['total_laps']
    track = {'dry': WR.DRY, 'damp': WR.DAMP, 'wet': WR.WET_TRACK}[case.get('track_condition', 'dry')]
    if first > L:
        return [(None, [([], {})])]
    rng = np.random.default_rng(zlib.crc32(name.encode()) + first)
    lap = lambda lo=first, hi=L: int(rng.integers(lo, hi + 1))
    other = WR.DAMP if track == WR.DRY else WR.DRY
    zero = [([], {}), ([(first, L, track)], {})]
    for remaining in (6, 5):
        if L - remaining >= first:
            zero.append(([(L - remaining, L, other)], {}))
    one = lap()
    zero.append(([(one, one, other)], {}))
    p = lap()
    q = lap(p)
    zero.append(([(p, q, WR.DAMP)] + ([(q + 1, L, WR.WET_TRACK)] if q < L else []), {}))
    p = lap(first, max(first, (first + L) // 2))
    cross = ([(p, min(L, p + lap(0, max(L // 4, 1))), other)], {})
    zero.append(cross)
    p = lap()
    plans = {0: (-1, 0, [(p, WR.INTER if other != WR.DRY else WR.MEDIUM)])}
    if n > 1:
        plans[n - 1] = (-1, 0, [])
    planned = ([(p, L, other)], plans)
    zero.append(planned)
    return [(None, zero), (FULL_TABLE, [([], {}), planned, cross])]


# ---------------------------------------------------------------- the sweep over every input, for the tests
FUZZ_SIMS, FUZZ_OFFSET = PC.FUZZ_SIMS, PC.FUZZ_OFFSET
GRID_PARTS, STATE_PARTS = 8, 4      # the inputs are dealt into this many slices, one per case of a parametrised test
# Inputs (of 100 from the grid, of 94 from a state) on which, by weather_ref alone: a car under the rule stopped only
# because it was on the wrong tyres; a red flag fell on a lap whose condition is not the case's; a finishing order moved.
# Measured with weather_ref on the CPU: GRID_MEASURED and STATE_MEASURED; the floors are a little below.
GRID_MEASURED, STATE_MEASURED = (87, 33, 89), (69, 26, 79)
GRID_FLOORS, STATE_FLOORS = (80, 28, 82), (62, 21, 72)


def _wanted(case, seed, sets, sim_offset, **kw):
    """[(table, scen, orders [S][m][n], laps on the wrong tyres [S][m][n])] and (crossed, red on a changed lap, moved)."""
    out, crossed, red_changed, moved = [], 0, 0, False
    for table, scen in sets:
        want = [WR.orders(case, FUZZ_SIMS, seed, sim_offset, plans=pl, changes=ch, table=table, want_marks=True, **kw)
                for ch, pl in scen]
        want_o, want_w = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        crossed += sum(w[2][0] for w in want)
        red_changed += sum(w[2][1] for w in want)
        moved |= any(not np.array_equal(want_o[s], want_o[0]) for s in range(1, len(scen)))
        out.append((table, scen, want_o, want_w))
    return out, (crossed > 0, red_changed > 0, moved)


@functools.lru_cache(maxsize=None)
def fuzz_inputs():
    return PC.fuzz_inputs()


@functools.lru_cache(maxsize=None)
def grid_wanted(part):
    """The restatement on slice `part` (of GRID_PARTS) of the inputs from the grid, computed once:
    [(name, case, seed, calls)] and the three counts."""
    inputs, refs = fuzz_inputs()
    assert len(inputs) == 100
    out, marks = [], np.zeros(3, np.int64)
    for (name, case, seed), ref in list(zip(inputs, refs))[part::GRID_PARTS]:
        calls, m = _wanted(case, seed, scenarios(name, case), FUZZ_OFFSET, grids=ref['grids'])
        assert np.array_equal(calls[0][2][0], ref['orders']), name          # the empty scenario is the oracle's race
        out.append((name, case, seed, calls))
        marks += m
    return out, marks


@functools.lru_cache(maxsize=None)
def state_wanted(part):
    """The same from states: on slice `part` (of STATE_PARTS) of the inputs of generic_cases.resume_inputs() the oracle's
    state of simulation FUZZ_OFFSET after k = max(1, L // 2), continued as simulations 0 .. FUZZ_SIMS - 1 under
    scenarios(name, case, first=k + 1): [(name, case, seed, state, calls)] and the three counts."""
    inputs, refs = fuzz_inputs()
    resume = {name for name, _, _ in G.resume_inputs()}
    picked = [(inp, ref) for inp, ref in zip(inputs, refs) if inp[0] in resume]
    assert len(picked) == 94
    out, marks = [], np.zeros(3, np.int64)
    for (name, case, seed), ref in picked[part::STATE_PARTS]:
        k = max(1, case['config']['total_laps'] // 2)
        state = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, FUZZ_OFFSET, k))
        calls, m = _wanted(case, seed, scenarios(name, case, first=k + 1), 0, state=state)
        out.append((name, case, seed, state, calls))
        marks += m
    return out, marks


def grid_marks():
    """(crossed, red flag on a changed lap, moved) over all inputs from the grid (the slices are computed once)."""
    return tuple(int(x) for x in sum(grid_wanted(p)[1] for p in range(GRID_PARTS)))


def state_marks():
    return tuple(int(x) for x in sum(state_wanted(p)[1] for p in range(STATE_PARTS)))


def check_floors(marks, floors):
    assert all(m >= f for m, f in zip(marks, floors)), (marks, floors)


def check_against(got, case, want_o, want_w, m):
    """The outputs of the code under test (orders, hist, delta, wrong-lap counts) against the restatement's."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    for s in range(want_o.shape[0]):
        bad = [i for i in range(m) if not np.array_equal(got['orders'][s, i], want_o[s, i])]
        assert not bad, f'scenario {s}: {len(bad)} of {m} orders differ, first sim {bad[0]}'
    assert np.array_equal(got['hist'], WR.hist_counts(want_o, n))
    assert np.array_equal(got['delta'], SR.delta_counts(want_o, n))
    assert np.array_equal(got['wrong_laps'], WR.wrong_counts(want_w, L))
