"""Scenario sets for the tests of mcgp_run_grids, generated from a case's shape (field size, laps, track condition) and
from the oracle's drawn grid of the input's first simulation, and seeded by CRC-32 of the case's name: the generator looks
at nothing the code under test returns (wanted(), below, hands the sets and the restatement's results to the caller's
comparison and reads its three counts from the restatement alone).  scenarios() gives one call per input, [(edits,
plans)] as grids_ref takes them; `pole`, `second` and so on are the drivers the oracle drew on those slots in the first
simulation (in the other seven another driver may stand there, which is part of the sweep):

  the empty scenario (so scenario 0 is mcgp_run's race); a one-place drop of the driver drawn on pole (its key ties with
  the second car's, which stays behind it: nobody moves); a drop of exactly n - 1 places of the pole driver; a drop of 255
  of a random driver; two dropped drivers whose keys tie on the slot of an undropped third (n >= 3); on a dry track with
  n >= 11, a two-place drop from slot 10, which crosses the tyre boundary behind slot 10, and a pin of the pole driver on
  slot 11; a pin on slot 1 with a pin on slot n; all n drivers pinned on a random permutation; one pit-lane car; two
  pit-lane cars; a pit-lane car with a start-tyre plan (and a stop where the race has the laps); a pin on the last slot in
  front of a pit-lane car; driver n - 1 (index 31 at n = 32) dropped three places; driver n - 1 from the pit lane with
  driver 0 pinned on slot 1.

At n = 1 and n = 2 nearly everything collapses onto the drawn grid; the scenarios that need more drivers are left out."""
import functools
import zlib

import numpy as np

import grids_ref as GR
import paces_cases as PC
import strategy_ref as SR

DROP, PIN, PIT_LANE = GR.DROP, GR.PIN, GR.PIT_LANE
ALL_PINNED = 'all pinned'


def scenarios(name, case, grid0):
    """-> [(edits, plans)], {label: scenario index}."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    dry = case.get('track_condition', 'dry') == 'dry'
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    grid0 = [int(d) for d in grid0]
    pick = lambda: int(rng.integers(0, n))
    out, at = [({}, {})], {}
    out.append(({grid0[0]: (DROP, 1, 0.0)}, {}))
    out.append(({grid0[0]: (DROP, max(n - 1, 1), 0.0)}, {}))
    out.append(({pick(): (DROP, 255, 0.0)}, {}))
    if n >= 3:
        out.append(({grid0[0]: (DROP, 2, 0.0), grid0[1]: (DROP, 1, 0.0)}, {}))
    if dry and n >= 11:
        out.append(({grid0[9]: (DROP, 2, 0.0)}, {}))
        out.append(({grid0[0]: (PIN, 11, 0.0)}, {}))
    a = pick()
    b = (a + 1 + int(rng.integers(0, max(n - 1, 1)))) % n
    out.append(({a: (PIN, 1, 0.0), b: (PIN, n, 0.0)} if n >= 2 else {a: (PIN, 1, 0.0)}, {}))
    perm = [int(x) for x in rng.permutation(n)]
    at[ALL_PINNED] = len(out)
    out.append(({d: (PIN, slot + 1, 0.0) for slot, d in enumerate(perm)}, {}))
    p = pick()
    at['pit'] = len(out)
    out.append(({p: (PIT_LANE, 0, 2.5)}, {}))
    if n >= 2:
        out.append(({p: (PIT_LANE, 0, 0.0), (p + 1) % n: (PIT_LANE, 0, 7.25)}, {}))
    start = 2 if dry else 4 if case.get('track_condition') == 'damp' else 3
    stops = [(int(rng.integers(2, L + 1)), 1 if dry else start)] if L >= 2 else []
    out.append(({p: (PIT_LANE, 0, 2.5)}, {p: (start, 0, stops)}))
    if n >= 2:
        out.append(({a: (PIN, n - 1, 0.0), b: (PIT_LANE, 0, 1.0)}, {}))
        out.append(({n - 1: (DROP, 3, 0.0)}, {}))
        out.append(({n - 1: (PIT_LANE, 0, 3.5), 0: (PIN, 1, 0.0)}, {}))
    return out, at


# ---------------------------------------------------------------- the sweep over every input, for the tests
FUZZ_SIMS, FUZZ_OFFSET = PC.FUZZ_SIMS, PC.FUZZ_OFFSET
PARTS = 10                          # the inputs are dealt into this many slices, one per case of a parametrised test
# Inputs (of 100) on which, by grids_ref alone: an edit changed a driver's start compound; a finishing order moved; a
# pit-lane car was classified ahead of a car that started from the grid.  Measured with grids_ref on the CPU: MEASURED;
# the floors are a little below.
MEASURED = (49, 94, 97)
FLOORS = (44, 88, 90)


@functools.lru_cache(maxsize=None)
def fuzz_inputs():
    return PC.fuzz_inputs()


@functools.lru_cache(maxsize=None)
def wanted(part):
    """The restatement on slice `part` (of PARTS) of the inputs, computed once: [(name, case, seed, scen, at, orders
    [S][m][n], start slots [S][m][n])] and the three counts."""
    inputs, refs = fuzz_inputs()
    assert len(inputs) == 100
    out, marks = [], np.zeros(3, np.int64)
    for (name, case, seed), ref in list(zip(inputs, refs))[part::PARTS]:
        scen, at = scenarios(name, case, ref['grids'][0])
        want = [GR.orders(case, FUZZ_SIMS, seed, FUZZ_OFFSET, plans=pl, edits=ed, grids=ref['grids'], want_marks=True)
                for ed, pl in scen]
        want_o, want_s = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        comps = np.stack([w[2] for w in want])
        assert np.array_equal(want_o[0], ref['orders']), name               # the empty scenario is the oracle's race
        for i in range(FUZZ_SIMS):                                          # ... on the oracle's grid
            assert np.array_equal(np.argsort(want_s[0, i]), ref['grids'][i]), name
        tyres = any(not np.array_equal(comps[s], comps[0]) for s in range(1, len(scen)) if not scen[s][1])
        moved = any(not np.array_equal(want_o[s], want_o[0]) for s in range(1, len(scen)))
        ahead = False
        for s, (ed, _) in enumerate(scen):
            lane = [d for d, e in ed.items() if e[0] == PIT_LANE]
            pos = np.argsort(want_o[s], axis=1)                             # pos[i, d]
            for d in lane:
                others = [o for o in range(pos.shape[1]) if o not in lane]
                ahead |= bool(others) and bool((pos[:, [d]] < pos[:, others]).any())
        marks += (tyres, moved, ahead)
        out.append((name, case, seed, scen, at, want_o, want_s))
    return out, marks


def marks():
    """(start compound changed, order moved, pit-lane car ahead of a grid starter) over all inputs."""
    return tuple(int(x) for x in sum(wanted(p)[1] for p in range(PARTS)))


def check_floors(got, floors):
    assert all(m >= f for m, f in zip(got, floors)), (got, floors)


def check_against(got, case, want_o, want_s, m):
    """The outputs of the code under test (orders, hist, delta, start, gain) against the restatement's."""
    n = len(case['grid_probs'])
    for s in range(want_o.shape[0]):
        bad = [i for i in range(m) if not np.array_equal(got['orders'][s, i], want_o[s, i])]
        assert not bad, f'scenario {s}: {len(bad)} of {m} orders differ, first sim {bad[0]}'
    assert np.array_equal(got['hist'], GR.hist_counts(want_o, n))
    assert np.array_equal(got['delta'], SR.delta_counts(want_o, n))
    assert np.array_equal(got['start'], GR.start_counts(want_s, n))
    assert np.array_equal(got['gain'], GR.gain_counts(want_s, want_o, n))
