"""Scenarios for the fuzz tests of mcgp_run_combined on the host build (test_combined_host_build.py) and on the device
(test_gpu_combined_fuzz.py), generated from a case's shape and seeded by CRC-32 of the case's name plus `first`: the
generator looks at nothing the code under test returns.  expectation() pairs them with the restatement's results
(combined_ref.ref_run) and reads from the restatement alone what they show; fuzz_sweep() hands both to the caller's
comparison over every input and asserts the conditions that keep the sweep from passing empty.

scenarios(name, case, first, pace_first, from_state) -> [combined_ref.scenario()], scaled to n cars and L laps; `first` is
the first lap with a pit step (2 from the grid, k + 1 from a state after lap k), `pace_first` the first lap an offset may
name (1 from the grid, k + 1 from a state):

  0  the empty scenario;
  1  a mix under rule stops, no plans: paces_cases' scenario 1 (LAPS ranges, lap `pace_first` alone, one UNTIL_STOP);
     SERVE penalties on up to three drivers pending from laps in the first half of what is left; FLAG penalties on up to
     three; ON_LAP additions of which one lap carries min(n, 3), drivers 0 and n - 1 among them (so the index
     lap_first + popc(lap_mask & (bit - 1)) is taken with a popcount above zero); up to four overrides on distinct
     laps, one of each kind, the NONE a range;
  2  thresholds astride one planned stop on lap q of drivers 0 and n - 1, under a forced safety car, both with an ON_LAP
     addition on q: driver 0 SERVE pending from exactly q (served) and, where q < L, UNTIL_STOP from q + 1 (not cleared);
     driver n - 1 SERVE pending from q + 1 (not served) and UNTIL_STOP from a lap <= q (cleared);
  3  a forced red flag on lap r, where driver 0 has a planned stop, a SERVE and an UNTIL_STOP both from before r (the
     stop serves and clears); driver n - 1 the same two items under a plan without stops (the red flag's tyre change
     serves and clears nothing); a FLAG penalty on one more driver, a LAPS offset over all the laps left on another.

Degenerate shapes shrink the list: first > L >= pace_first (a one-lap race from the grid): the empty scenario and one
with offsets on lap 1 and FLAG penalties; pace_first > L (a state after lap L): the empty scenario and a FLAG-only one;
first == L: no scenario 3, and scenario 2 without what would name lap L + 1; n == 1: everything lands on driver 0, who
then gets driver 0's items only.

What the restatement shows at FUZZ_SIMS = 8, FUZZ_OFFSET = 3 (inputs on which each occurs at least once; measured on
the CPU, the floors of FLOORS are set below these figures):

                                                            from the grid (100)   from states (94)
  an order differs from scenario 0                                   96                  85
  fate SERVED                                                        96                  69
  fate FLAG                                                          91                  88
  fate RETIRED                                                       95                  81
  an offset cleared by a stop                                        97                  86
  an offset carried to the flag or cut by retirement                100                  93
  scenario 2: driver 0 served and not cleared                        92                  66
  scenario 2: driver n - 1 cleared and not served                    90                  75
  two ON_LAP additions reach running cars on one lap                 94                  78
  scenario 3: driver 0 served and cleared on the red-flag lap,
              driver n - 1 unserved and uncleared                    93                  66

From a state all 8 simulations share who has retired by then, driver 0 in 26 of the 94 states, which is what the right
column loses.

Nothing here looks at what the code under test returns."""
import zlib

import numpy as np

import combined_ref as CR
import generic_cases as G
import paces_cases as PC
import paces_ref as PR
import penalties_cases as NC
import resume_ref as RR

SERVE, FLAG, LAP = CR.SERVE, CR.FLAG, CR.LAP
NONE, RED, SC, VSC = CR.NONE, CR.RED, CR.SC, CR.VSC
FUZZ_SIMS, FUZZ_OFFSET = PC.FUZZ_SIMS, PC.FUZZ_OFFSET
SHOWS = ('moved', 'served', 'flag', 'retired', 'cleared', 'kept', 'serve_only', 'clear_only', 'two_added', 'red_stop')
# Floors of the conditions, in inputs, from the grid (of 100) and from states (of 94); the figures are in the docstring.
FLOORS = {
    'grid': dict(moved=93, served=90, flag=85, retired=88, cleared=90, kept=93, serve_only=85, clear_only=83, two_added=88,
                 red_stop=85),
    'state': dict(moved=80, served=62, flag=80, retired=72, cleared=78, kept=85, serve_only=58, clear_only=66, two_added=70,
                  red_stop=58),
}
# Inputs on which no scenario of scenarios() changes any of the 8 finishing orders (at most 7 may be listed).  From a
# state, one with fewer than two cars still running has nothing left to reorder and needs no entry (fuzz_sweep reads that
# from the oracle's trace): F19, F27, F29, F52, X_all_out_lap1, X_all_out_lap2 and X_half_out after max(1, L // 2).
NO_BITE = {
    'F09': 'from the state: two cars left of three, 10 s apart with 11 laps to go, and neither draws what would swap them',
    'F27': 'a two-car wet race over 78 laps: one of the two retires in every one of the 8 simulations',
    'F52': 'a two-car race over 66 laps: one of the two retires in every one of the 8 simulations',
    'F63': 'from the state: two cars left of five, 25 minutes apart with 22 laps to go',
    'X_all_out_lap1': 'every car retires on lap 1: nobody runs where time is added or a pace is read',
    'n1': 'one car',
}


def _seconds(rng):
    return float(np.round(rng.uniform(0.4, 3.0), 3)) * (1 if rng.integers(0, 2) else -1)


def _pick(rng, n, k):
    return [int(d) for d in rng.choice(n, size=min(n, k), replace=False)]


def _flag_penalties(rng, n):
    """On up to three drivers; the first one's is ten minutes, which reorders fields that finish minutes apart."""
    return [(d, FLAG, 0, 600.0 if j == 0 else float(rng.choice(NC.SECONDS))) for j, d in enumerate(_pick(rng, n, 3))]


def _mix(rng, n, L, first, pace_first):
    """Scenario 1."""
    half = lambda: int(rng.integers(first, first + (L - first) // 2 + 1))
    # offsets: paces_cases' scenario 1
    offs, taken = [], set()
    who = int(rng.integers(0, n))
    offs.append(PR.laps(who, pace_first, pace_first, _seconds(rng)))
    taken.add((who, pace_first))
    for _ in range(int(rng.integers(1, 6))):
        d = int(rng.integers(0, n))
        a = int(rng.integers(pace_first, L + 1))
        b = min(L, a + int(rng.integers(0, max(L // 2, 1))))
        if any((d, lap) in taken for lap in range(a, b + 1)):
            continue
        taken.update((d, lap) for lap in range(a, b + 1))
        offs.append(PR.laps(d, a, b, _seconds(rng)))
    offs.append(PR.until_stop(int(rng.integers(0, n)),
                              int(rng.integers(pace_first, pace_first + max((L - pace_first) // 3, 0) + 1)), _seconds(rng)))
    # penalties
    pens = [(d, SERVE, half(), float(rng.choice(NC.SECONDS))) for d in _pick(rng, n, 3)]
    pens += _flag_penalties(rng, n)
    crowd = half()
    who = sorted({0, n - 1} | ({int(rng.integers(0, n))} if n >= 3 else set()))
    while len(who) < min(n, 3):
        who = sorted(set(who) | {int(rng.integers(0, n))})
    added = {(d, crowd) for d in who}
    for _ in range(2):
        added.add((int(rng.integers(0, n)), int(rng.integers(first, L + 1))))
    pens += [(d, LAP, lap, 0.5 + 0.125 * ((3 * d + lap) % 16)) for d, lap in sorted(added)]
    # overrides: up to four distinct laps, one kind each, the NONE stretched to a range over free laps
    laps = sorted(int(x) for x in rng.choice(np.arange(first, L + 1), size=min(4, L - first + 1), replace=False))
    kinds = [int(k) for k in rng.permutation([SC, VSC, RED, NONE])][:len(laps)]
    evs = []
    for j, (lap, kind) in enumerate(zip(laps, kinds)):
        last = lap
        if kind == NONE:
            last = min(lap + 3, (laps[j + 1] - 1) if j + 1 < len(laps) else L)
        evs.append((lap, last, kind))
    perm = rng.permutation(len(pens))
    return CR.scenario({}, [pens[j] for j in perm], evs, offs)


def _astride(rng, n, L, first, pace_first):
    """Scenario 2."""
    q = int(rng.integers(first, min(L - 1, first + (L - first) // 2) + 1)) if L > first else L
    plans = {0: (-1, 0, [(q, 1 + q % 2)])}
    pens = [(0, SERVE, q, 5.0), (0, LAP, q, 1.25)]
    offs = [PR.until_stop(0, q + 1, abs(_seconds(rng)))] if q + 1 <= L else []
    if n > 1:
        z = n - 1
        plans[z] = (-1, 0, [(q, 2 - q % 2)])
        pens.append((z, LAP, q, 0.75))
        if q + 1 <= L:
            pens.append((z, SERVE, q + 1, 10.0))
        offs.append(PR.until_stop(z, int(rng.integers(pace_first, q + 1)), _seconds(rng)))
    return CR.scenario(plans, pens, [(q, q, SC)], offs)


def _red_stop(rng, n, L, first, pace_first):
    """Scenario 3, for first < L."""
    r = int(rng.integers(first + 1, min(L, first + 1 + (L - first) // 3) + 1))
    plans, pens, offs = {0: (-1, 0, [(r, 2)])}, [], []
    for d in sorted({0, n - 1}):
        if d:
            plans[d] = (-1, 0, [])
        pens.append((d, SERVE, int(rng.integers(first, r)), 5.0 + d / 8))
        offs.append(PR.until_stop(d, int(rng.integers(pace_first, r)), abs(_seconds(rng))))
    pens.append((1 if n >= 3 else 0, FLAG, 0, float(rng.choice(NC.SECONDS))))
    offs.append(PR.laps(2 if n >= 4 else n - 1, pace_first, L, 10.0 * _seconds(rng)))     # 4 .. 30 s a lap: minutes
    return CR.scenario(plans, pens, [(r, r, RED)], offs)


def scenarios(name, case, first, pace_first, from_state=False):
    n, L = len(case['grid_probs']), case['config']['total_laps']
    assert (pace_first == first) if from_state else (first, pace_first) == (2, 1)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + first)
    out = [CR.scenario()]
    if pace_first > L:                                      # a state after lap L: nothing is raced
        return out + [CR.scenario(penalties=_flag_penalties(rng, n))]
    if first > L:                                           # a race of one lap from the grid
        offs = [PR.laps(d, 1, 1, _seconds(rng)) for d in _pick(rng, n, 2)] + [PR.until_stop(n - 1, 1, _seconds(rng))]
        return out + [CR.scenario(penalties=_flag_penalties(rng, n), paces=offs)]
    out.append(_mix(rng, n, L, first, pace_first))
    out.append(_astride(rng, n, L, first, pace_first))
    if first < L:
        out.append(_red_stop(rng, n, L, first, pace_first))
    return out


# ---------------------------------------------------------------- what a run must give, and what it shows
def state_after(case, seed, ref, k, sim=0, offset=FUZZ_OFFSET):
    """The oracle's state of traced simulation `sim` (id offset + sim) after lap k, as combined_ref takes it."""
    return RR.state_arrays(ref, sim, k), k, RR.drs_disabled_until(case, seed, offset + sim, k)


def expectation(name, case, seed, ref, k=None, m=FUZZ_SIMS):
    """The scenarios of a case with the restatement's results: from the grid (k None: simulations FUZZ_OFFSET ..
    FUZZ_OFFSET + m - 1, the traced ones) or from the state of traced simulation 0 after lap k, continued as simulations
    0 .. m - 1.  -> dict(scen, want (orders, fates, event laps, laps carried), state, offset, shows {name of SHOWS: bool})."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    if k is None:
        state, offset, first, pace_first, kw = None, FUZZ_OFFSET, 2, 1, dict(grids=ref['grids'][:m])
    else:
        state = state_after(case, seed, ref, k)
        offset, first, pace_first, kw = 0, k + 1, k + 1, dict(state=state)
    scen = scenarios(name, case, first, pace_first, k is not None)
    assert scen[0] == CR.scenario()
    o, f, e, c, ends, most = CR.ref_run(case, scen, m, seed, offset, want_ends=True, **kw)
    if k is None:
        assert np.array_equal(o[0], ref['orders'][:m]), name       # scenario 0 is the oracle's race
    shows = dict(moved=any(not np.array_equal(o[s], o[0]) for s in range(1, len(scen))),
                 served=bool((f == CR.FATE_SERVED).any()), flag=bool((f == CR.FATE_FLAG).any()),
                 retired=bool((f == CR.FATE_RETIRED).any()), cleared=bool((ends == PR.FATE_STOP).any()),
                 kept=bool(((ends == PR.FATE_FLAG) | (ends == PR.FATE_RETIRED)).any()), two_added=bool((most >= 2).any()),
                 serve_only=False, clear_only=False, red_stop=False)
    z = n - 1
    if len(scen) >= 3 and scen[2]['plans']:
        shows['serve_only'] = bool(((f[2][:, 0] == CR.FATE_SERVED) & (ends[2][:, 0] != PR.FATE_NONE)
                                    & (ends[2][:, 0] != PR.FATE_STOP)).any())
        if n > 1:
            shows['clear_only'] = bool(((ends[2][:, z] == PR.FATE_STOP) & (f[2][:, z] != CR.FATE_NONE)
                                        & (f[2][:, z] != CR.FATE_SERVED)).any())
    if len(scen) == 4 and n > 1:
        (r, _, _), = scen[3]['events']
        p = [a for d, kind, a, _, _ in scen[3]['paces'] if d == 0 and kind == PR.UNTIL_STOP][0]
        here = (f[3][:, 0] == CR.FATE_SERVED) & (ends[3][:, 0] == PR.FATE_STOP) & (c[3][:, 0] == r - p + 1)
        there = (f[3][:, z] != CR.FATE_SERVED) & (f[3][:, z] != CR.FATE_NONE) & (ends[3][:, z] != PR.FATE_STOP) \
            & (ends[3][:, z] != PR.FATE_NONE)
        shows['red_stop'] = bool((here & there).any())
    return dict(scen=scen, want=(o, f, e, c), state=state, offset=offset, shows=shows)


# ---------------------------------------------------------------- the sweep over every input, for the tests
def fuzz_inputs():
    """paces_cases.fuzz_inputs(): the 100 run inputs and the oracle's traced run of each, made in a pool of threads."""
    return PC.fuzz_inputs()


def fuzz_sweep(inputs, refs, compare, from_state=False, m=FUZZ_SIMS):
    """The generated scenarios on every input, from the grid or (from_state) on the inputs of resume_inputs() from the
    oracle's state of simulation FUZZ_OFFSET after max(1, L // 2): compare(case, seed, scen, want, m, offset, state) checks
    the code under test against the restatement's (orders, fates, event laps, laps carried) and ends in
    combined_host_build.check_against.  Asserts that no input is left out and the conditions of FLOORS, all read from the
    restatement alone before `compare` is called."""
    if from_state:
        resume = {name for name, _, _ in G.resume_inputs()}
        pairs = [(a, ref) for a, ref in zip(inputs, refs) if a[0] in resume]
    else:
        pairs = list(zip(inputs, refs))
    shown, quiet, done = dict.fromkeys(SHOWS, 0), [], 0
    for (name, case, seed), ref in pairs:
        L = case['config']['total_laps']
        k = max(1, L // 2) if from_state else None
        e = expectation(name, case, seed, ref, k, m)
        for key in SHOWS:
            shown[key] += e['shows'][key]
        if not e['shows']['moved'] and not (from_state and (ref['trace']['dnf'][0, k - 1] == 0).sum() < 2):
            quiet.append(name)
        compare(case, seed, e['scen'], e['want'], m, e['offset'], e['state'])
        done += 1
    assert done == (94 if from_state else 100)
    assert len(NO_BITE) <= 7 and set(quiet) <= set(NO_BITE), quiet
    floors = FLOORS['state' if from_state else 'grid']
    assert all(shown[key] >= floors[key] for key in SHOWS), shown
    return shown
