"""Override sets for the fuzz tests of mcgp_run_events (tests/test_gpu_events_fuzz.py), generated from a case's shape
and seeded by CRC-32 of the case's name: nothing here looks at what the code under test returns.  A set is [(overrides,
plans)] as events_ref takes them: the empty scenario; a scenario of up to 8 random ranges of random kinds that always
holds an override contradicting what simulation `sim` draws on that lap (read from the oracle's Philox) and, where the
race is long enough, a forced safety car with a planned stop of driver 0 on the same lap; and the complement scenario:
no event on every lap that has one drawn in `sim`, a VSC on the first lap that has none."""
import zlib

import numpy as np

import events_ref as ER


def scenarios(name, case, seed, sim, first):
    """-> ([(overrides, plans)], contradicted laps of `sim`)."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    out = [([], {})]
    if first > L:
        return out, 0
    rng = np.random.default_rng(zlib.crc32(name.encode()) + first)
    drawn = {lap: ER.drawn_event(case, seed, sim, lap)[0] for lap in range(first, L + 1)}
    # random ranges over a random subset of the laps, then the two laps every set holds
    forced = {}
    for _ in range(int(rng.integers(1, 7))):
        a = int(rng.integers(first, L + 1))
        b = min(L, a + int(rng.integers(0, 4)))
        kind = int(rng.integers(0, 4))
        for lap in range(a, b + 1):
            forced[lap] = kind
    x = int(rng.integers(first, L + 1))                     # the contradiction
    forced[x] = (drawn[x] + 1 + int(rng.integers(0, 3))) % 4
    plans = {}
    if L - first >= 2:
        y = first + (x - first + 1) % (L - first + 1)       # another lap: a safety car and a stop under it
        forced[y] = ER.SC
        plans = {0: (-1, 0, [(y, 1 + (y % 2))])}
    laps = sorted(forced)
    ranges = []
    for lap in laps:
        if ranges and ranges[-1][1] == lap - 1 and ranges[-1][2] == forced[lap]:
            ranges[-1] = (ranges[-1][0], lap, forced[lap])
        else:
            ranges.append((lap, lap, forced[lap]))
    assert len(ranges) <= 64
    out.append((ranges, plans))
    contradicted = sum(forced[lap] != drawn[lap] for lap in laps)
    assert contradicted >= 1
    # the complement: what `sim` drew is taken away, and a VSC stands where it drew nothing
    comp = [(lap, lap, ER.NONE) for lap in range(first, L + 1) if drawn[lap] != ER.NONE][:63]
    quiet = [lap for lap in range(first, L + 1) if drawn[lap] == ER.NONE]
    if quiet:
        comp.append((quiet[0], quiet[0], ER.VSC))
    out.append((sorted(comp), {}))
    return out, contradicted
