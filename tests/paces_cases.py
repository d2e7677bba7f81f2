"""Offset sets for the fuzz tests of mcgp_run_paces, generated from a case's shape and seeded by CRC-32 of the case's
name: the generator looks at nothing the code under test returns (fuzz_sweep, below, hands it to the caller's comparison and
reads its three conditions from the restatement alone).  A set is [(offsets, plans)] as paces_ref takes them:

  0  the empty scenario;
  1  up to 6 random LAPS ranges (a driver's ranges share no lap) of 0.4 .. 3 s of either sign on random drivers, one of
     them lap 1 alone, and an UNTIL_STOP offset of a driver under the model's rule from a lap in the first third of the
     race (a rule stop clears it where the car makes one);
  2  driver 0 slowed from a lap p until a planned stop on a lap q >= p (cleared there unless the car retires first), the
     last driver (if there is another) slowed from lap `first` under a plan without stops (carried to the flag, or cut
     by its retirement), and a LAPS offset on the same laps as driver 0's UNTIL_STOP offset."""
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import generic_cases as G
import oracle_py as O
import paces_ref as PR
import resume_ref as RR
import strategy_ref as SR


def scenarios(name, case, first=1):
    n, L = len(case['grid_probs']), case['config']['total_laps']
    out = [([], {})]
    if first > L:
        return out
    rng = np.random.default_rng(zlib.crc32(name.encode()) + first)
    sec = lambda: float(np.round(rng.uniform(0.4, 3.0), 3)) * (1 if rng.integers(0, 2) else -1)
    # ---- 1: random ranges, lap `first` alone, an UNTIL_STOP offset under the rule
    offs, taken = [], set()
    who = int(rng.integers(0, n))
    offs.append(PR.laps(who, first, first, sec()))
    taken.add((who, first))
    for _ in range(int(rng.integers(1, 6))):
        d = int(rng.integers(0, n))
        a = int(rng.integers(first, L + 1))
        b = min(L, a + int(rng.integers(0, max(L // 2, 1))))
        if any((d, lap) in taken for lap in range(a, b + 1)):
            continue
        taken.update((d, lap) for lap in range(a, b + 1))
        offs.append(PR.laps(d, a, b, sec()))
    offs.append(PR.until_stop(int(rng.integers(0, n)), int(rng.integers(first, first + max((L - first) // 3, 0) + 1)), sec()))
    out.append((offs, {}))
    # ---- 2: cleared by a planned stop; carried to the flag under a plan without stops
    p = int(rng.integers(first, L + 1))
    offs, plans = [PR.until_stop(0, p, abs(sec()))], {}
    q = max(p, 2, first)
    if q <= L:
        q = int(rng.integers(q, L + 1))
        plans[0] = (-1, 0, [(q, 1 + (q % 2))])
        offs.append(PR.laps(0, p, q, sec()))
    if n > 1:
        plans[n - 1] = (-1, 0, [])
        offs.append(PR.until_stop(n - 1, first, sec()))
    out.append((offs, plans))
    return out


# ---------------------------------------------------------------- the sweep over every input, for the tests
FUZZ_SIMS, FUZZ_OFFSET = 8, 3
STATE_FLOORS = (75, 65, 85)         # state_sweep's floors for MOVED, CLEARED and KEPT, below its measured figures


def fuzz_sweep(inputs, refs, compare):
    """The generated offset sets on every input: compare(case, seed, scen, want_o, want_c) checks the code under test
    against the restatement's orders and laps carried.  Asserts the three conditions that keep the sweep from passing
    empty, all of them read from the restatement alone."""
    moved = cleared = kept = 0
    for (name, case, seed), ref in zip(inputs, refs):
        scen = scenarios(name, case)
        want = [PR.orders(case, FUZZ_SIMS, seed, FUZZ_OFFSET, plans=pl, offsets=offs, grids=ref['grids'], want_fates=True)
                for offs, pl in scen]
        want_o, want_c = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        fates = np.stack([w[2] for w in want])
        assert np.array_equal(want_o[0], ref['orders']), name
        compare(case, seed, scen, want_o, want_c)
        moved += any(not np.array_equal(want_o[s], want_o[0]) for s in range(1, len(scen)))
        cleared += bool((fates == PR.FATE_STOP).any())
        kept += bool(((fates == PR.FATE_FLAG) | (fates == PR.FATE_RETIRED)).any())
    assert len(inputs) == 100
    assert moved >= 80 and cleared >= 60 and kept >= 20, (moved, cleared, kept)


def state_sweep(inputs, refs, compare):
    """The same from states: on the inputs of generic_cases.resume_inputs() (picked from `inputs`, with their traced runs)
    the oracle's state of simulation FUZZ_OFFSET after k = max(1, L // 2), continued as simulations 0 .. FUZZ_SIMS - 1
    under scenarios(name, case, first=k + 1); compare(case, seed, scen, want_o, want_c, state).  The conditions, read from
    the restatement alone: an order moves on MOVED inputs, an offset is cleared by a stop on CLEARED and carried to the
    flag or cut by a retirement on KEPT (measured: 82, 74 and 93 of 94; from a state all 8 simulations share who has
    retired, so fewer inputs show a stop than from the grid)."""
    resume = {name for name, _, _ in G.resume_inputs()}
    done = moved = cleared = kept = 0
    for (name, case, seed), ref in zip(inputs, refs):
        if name not in resume:
            continue
        k = max(1, case['config']['total_laps'] // 2)
        state = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, FUZZ_OFFSET, k))
        scen = scenarios(name, case, first=k + 1)
        want = [PR.orders(case, FUZZ_SIMS, seed, 0, plans=pl, offsets=offs, state=state, want_fates=True) for offs, pl in scen]
        want_o, want_c = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        fates = np.stack([w[2] for w in want])
        compare(case, seed, scen, want_o, want_c, state)
        moved += any(not np.array_equal(want_o[s], want_o[0]) for s in range(1, len(scen)))
        cleared += bool((fates == PR.FATE_STOP).any())
        kept += bool(((fates == PR.FATE_FLAG) | (fates == PR.FATE_RETIRED)).any())
        done += 1
    assert done == 94
    assert moved >= STATE_FLOORS[0] and cleared >= STATE_FLOORS[1] and kept >= STATE_FLOORS[2], (moved, cleared, kept)


def fuzz_inputs():
    inputs = G.run_inputs()
    O.lib()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        refs = list(pool.map(lambda a: RR.traced_run(a[1], FUZZ_SIMS, a[2], FUZZ_OFFSET), inputs))
    return inputs, refs


def check_against(got, case, want_o, want_c, m):
    """The outputs of the code under test (orders, hist, delta, carried counts) against the restatement's."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    for s in range(want_o.shape[0]):
        bad = [i for i in range(m) if not np.array_equal(got['orders'][s, i], want_o[s, i])]
        assert not bad, f'scenario {s}: {len(bad)} of {m} orders differ, first sim {bad[0]}'
    assert np.array_equal(got['hist'], PR.hist_counts(want_o, n))
    assert np.array_equal(got['delta'], SR.delta_counts(want_o, n))
    assert np.array_equal(got['carried'], PR.carried_counts(want_c, L))
