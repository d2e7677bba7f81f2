"""Random mixtures and whole-field edit sets for the tests of mcgp_run_grids at its limits, generated from a case's shape
(field size, laps, track condition) and seeded by CRC-32 of the case's name: the generator looks at nothing the code
under test returns (wanted(), below, hands the sets and the restatement's results to the caller's comparison and reads its
three counts from the restatement alone).  scenarios() gives one call per input, [(edits, plans)] as grids_ref takes them:

  0  the empty scenario (so scenario 0 is mcgp_run's race);
  `mixtures` random mixtures: every driver independently gets nothing, a drop, a pin or a pit-lane start; the drops are
     drawn from {1, 2, 3, n - 1, n, 31, 254, 255}, the pins are distinct random slots in front of the pit-lane slots, the
     pit-lane seconds are drawn from {0, 5e-324, 2.5, 1e6}; every other mixture also carries a start-tyre plan on one
     edited driver and a planned stop on another, where the race has the laps;
  every driver from the pit lane (the seconds rotate through the four values);
  every driver dropped 255 - d places; every driver dropped 1 + d % 3 places (the keys tie in runs);
  every driver but one pinned, the one free slot in the middle of the grid (n >= 2);
  drivers 0 .. n - 2 from the pit lane and driver n - 1 pinned on slot 1 (n >= 2).

A second reference for the start slots, which shares nothing with grids_ref.edited_grid, covers the scenarios that only
drop: reference_rule_slots, the reference project's own rule (sort by (drawn + drop, drawn), number from 1), fed the
oracle's grids; wanted() asserts it on every such scenario."""
import functools
import zlib

import numpy as np

import grids_cases as GC
import grids_ref as GR

DROP, PIN, PIT_LANE = GR.DROP, GR.PIN, GR.PIT_LANE
SECONDS = (0.0, 5e-324, 2.5, 1e6)
MIXTURES = 6


def drops_of(n):
    return [v for v in (1, 2, 3, n - 1, n, 31, 254, 255) if 1 <= v <= 255]


def _mixture(rng, n, L, dry, wet_start, planned):
    kind = rng.integers(0, 4, n)                            # 0 nothing, 1 drop, 2 pin, 3 pit lane
    lane = [d for d in range(n) if kind[d] == 3]
    pinned = [d for d in range(n) if kind[d] == 2]
    slots = rng.permutation(n - len(lane))[:len(pinned)]    # (there are at least as many slots as drivers outside the lane)
    edits = {}
    for d in range(n):
        if kind[d] == 1:
            edits[d] = (DROP, int(rng.choice(drops_of(n))), 0.0)
        elif kind[d] == 3:
            edits[d] = (PIT_LANE, 0, SECONDS[int(rng.integers(0, 4))])
    for d, slot in zip(pinned, slots):
        edits[d] = (PIN, int(slot) + 1, 0.0)
    plans = {}
    if planned and edits:
        who = [int(d) for d in rng.permutation(sorted(edits))]
        plans[who[0]] = (2 if dry else wet_start, 0, [])
        if len(who) > 1 and L >= 2:
            plans[who[1]] = (-1, 0, [(int(rng.integers(2, L + 1)), 1 if dry else wet_start)])
    return edits, plans


def scenarios(name, case, mixtures=MIXTURES):
    """-> [(edits, plans)]: 1 + mixtures + 5 scenarios (two fewer at n = 1, which has no second driver)."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    cond = case.get('track_condition', 'dry')
    dry, wet_start = cond == 'dry', 4 if cond == 'damp' else 3
    rng = np.random.default_rng(zlib.crc32(name.encode()) ^ 0x6c696d)
    out = [({}, {})]
    for k in range(mixtures):
        out.append(_mixture(rng, n, L, dry, wet_start, planned=k % 2 == 1))
    out.append(({d: (PIT_LANE, 0, SECONDS[d % 4]) for d in range(n)}, {}))
    out.append(({d: (DROP, 255 - d, 0.0) for d in range(n)}, {}))
    out.append(({d: (DROP, 1 + d % 3, 0.0) for d in range(n)}, {}))
    if n >= 2:
        free = int(rng.integers(0, n))
        slots = [p for p in rng.permutation(n) if p != n // 2]
        out.append(({d: (PIN, int(slot) + 1, 0.0) for d, slot in zip([d for d in range(n) if d != free], slots)}, {}))
        lane = {d: (PIT_LANE, 0, SECONDS[(d + 1) % 4]) for d in range(n - 1)}
        lane[n - 1] = (PIN, 1, 0.0)
        out.append((lane, {}))
    return out


def only_drops(edits):
    return bool(edits) and all(kind == DROP for kind, _, _ in edits.values())


def reference_rule_slots(grid, edits):
    """The start slots (0-based, by driver) of a drop-only edit set by the reference project's rule for grid penalties:
    sort the drivers by (drawn position + places, drawn position) and number them from 1."""
    drawn = {int(d): p + 1 for p, d in enumerate(grid)}
    ranked = sorted(drawn, key=lambda d: (drawn[d] + (edits[d][1] if d in edits else 0), drawn[d]))
    final = {d: i + 1 for i, d in enumerate(ranked)}
    return [final[d] - 1 for d in range(len(grid))]


def sim_marks(grid, edits, slots):
    """(jumped, tied) of one simulation, from the drawn grid, the edits and the restatement's start slots alone: an
    unplaced car's new slot lies behind a pinned slot that lay behind its drawn slot; two unplaced cars have equal
    drawn slot + drop."""
    drawn = {int(d): p for p, d in enumerate(grid)}
    pins = [v - 1 for kind, v, _ in edits.values() if kind == PIN]
    loose = [d for d in drawn if d not in edits or edits[d][0] == DROP]
    jumped = any(drawn[d] < p < slots[d] for d in loose for p in pins)
    keys = [drawn[d] + (edits[d][1] if d in edits else 0) for d in loose]
    return jumped, len(set(keys)) < len(keys)


# ---------------------------------------------------------------- the sweep over every input, for the tests
FUZZ_SIMS, FUZZ_OFFSET = GC.FUZZ_SIMS, GC.FUZZ_OFFSET
PARTS = 10                          # the inputs are dealt into this many slices, one per case of a parametrised test
# Inputs (of 100) with a simulation in which, by grids_ref and the oracle's grids alone: an unplaced car's new slot lies
# behind a pinned slot that lay behind its drawn slot; two unplaced cars have equal drawn slot + drop; a finishing order
# differs from scenario 0's.  Measured with grids_ref on the CPU: MEASURED; the floors are about a tenth below.
MEASURED = (85, 99, 95)
FLOORS = (76, 89, 85)


def restate(case, seed, scen, grids, m, offset):
    """grids_ref under every scenario -> (orders [S][m][n], start slots [S][m][n]), the drop-only scenarios' slots
    checked against the reference project's rule."""
    want = [GR.orders(case, m, seed, offset, plans=pl, edits=ed, grids=grids) for ed, pl in scen]
    want_o, want_s = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    for s, (ed, _) in enumerate(scen):
        if only_drops(ed):
            for i in range(m):
                assert list(want_s[s, i]) == reference_rule_slots(grids[i], ed), (s, i)
    return want_o, want_s


@functools.lru_cache(maxsize=None)
def wanted(part):
    """The restatement on slice `part` (of PARTS) of the inputs, computed once: [(name, case, seed, scen, orders
    [S][m][n], start slots [S][m][n])] and the three counts."""
    inputs, refs = GC.fuzz_inputs()
    assert len(inputs) == 100
    out, marks = [], np.zeros(3, np.int64)
    for (name, case, seed), ref in list(zip(inputs, refs))[part::PARTS]:
        scen = scenarios(name, case)
        want_o, want_s = restate(case, seed, scen, ref['grids'], FUZZ_SIMS, FUZZ_OFFSET)
        assert np.array_equal(want_o[0], ref['orders']), name               # the empty scenario is the oracle's race
        hits = [sim_marks(ref['grids'][i], ed, want_s[s, i]) for s, (ed, _) in enumerate(scen) for i in range(FUZZ_SIMS)]
        moved = any(not np.array_equal(want_o[s], want_o[0]) for s in range(1, len(scen)))
        marks += (any(j for j, _ in hits), any(t for _, t in hits), moved)
        out.append((name, case, seed, scen, want_o, want_s))
    return out, marks


def marks():
    """(a pin jumped, keys tied, order moved) over all inputs."""
    return tuple(int(x) for x in sum(wanted(p)[1] for p in range(PARTS)))


check_floors, check_against = GC.check_floors, GC.check_against


# ---------------------------------------------------------------- the counting loops' call: F33 under 64 scenarios
MAX_SCENARIOS = 64


def full_scenarios(name, case):
    """64 scenarios of the generator: the empty one, 58 mixtures and the five whole-field sets."""
    scen = scenarios(name, case, mixtures=MAX_SCENARIOS - 6)
    assert len(scen) == MAX_SCENARIOS
    return scen


def edited_slots(scen, grids):
    """Start slots [S][m][n] of grids_ref.edited_grid on drawn grids [m][n]: no race is run."""
    m, n = grids.shape
    out = np.zeros((len(scen), m, n), np.int64)
    for s, (ed, _) in enumerate(scen):
        for i in range(m):
            out[s, i, GR.edited_grid(grids[i], ed)] = np.arange(n)
    return out
