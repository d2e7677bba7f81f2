"""Inputs shared by the tests of the generic kernel family (race_kernel, race_resume_kernel, race_trace_kernel,
race_scenario_kernel, race_gaps_kernel, race_conditions_kernel, race_stints_kernel, race_moves_kernel,
race_fastest_kernel) on the host build (test_generic_host_build.py, test_gaps_host_build.py,
test_conditions_host_build.py, test_stints_host_build.py, test_moves_host_build.py, test_penalties_host_build.py,
test_fastest_host_build.py) and on the device (test_gpu_generic_fuzz.py for trace, resume and strategies,
test_gpu_gaps_conditions_fuzz.py for gaps and conditions, test_gpu_stints_moves_fuzz.py for stints and moves with their
counting kernels, test_gpu_penalties_fuzz.py for penalties, whose scenarios are in penalties_cases.py,
test_gpu_bonus_live_fuzz.py for the fastest lap): the configurations, the laps a race is resumed from, and the
plan scenarios, all scaled to a case's field size and lap count.  Nothing here looks at what the code under test returns."""
import copy
import json

import numpy as np

import oracle_py as O
import resume_ref as RR

GOLDEN = ('S60', 'S78', 'S50', 'EVT', 'HET', 'DMP', 'WET', 'N10')
FIELD_SIZES = (1, 2, 3, 19, 31, 32)
N_FUZZ, N_FUZZ_STRATEGY, MIN_STRATEGY_LAPS = 84, 75, 8
SOFT, MEDIUM, HARD, INTER, WET = range(5)
# Configurations in which no scenario of grid_scenarios can change a finishing order (at most 4 may be listed):
NO_BITE = {
    'X_all_out_lap1': 'every car retires on lap 1: nobody runs on a stop lap',
    'F27': 'a two-car wet race: the cars finish minutes apart or one retires, a stop of 30 s moves neither',
    'F29': 'a three-car wet race, mostly decided by retirements (D01: p = 0.2 a lap): no scenario moves any of 32 orders',
}

_fuzz = None


def fuzz_cases():
    """The 84 configurations of tests/golden/fuzz_cases.json, {name: case} (each case carries its own seed)."""
    global _fuzz
    if _fuzz is None:
        with open(O.GOLDEN_DIR + '/fuzz_cases.json') as f:
            _fuzz = json.load(f)
        assert len(_fuzz) == N_FUZZ
    return _fuzz


def near_zero_case():
    """S60 with a field lapping in about 5 s: overtakes land at times around 0.1 s, where the max(0.1, ahead - 0.1)
    of the reference (:528) decides."""
    case = copy.deepcopy(O.load_case('S60'))
    case['base_pace'] = {d: 5.0 + 0.1 * i for i, d in enumerate(case['base_pace'])}
    return case


def floor_case():
    """S60 over 12 laps with a field lapping in 0.05 to 0.25 s: the leaders' cumulative times stay under 0.2 s for several
    laps, so an overtaking car's new time, ahead - 0.1, falls below the 0.1 floor of the reference (:528) -- which
    near_zero_case never reaches: its cumulative times pass 5 s on lap 1.  (Without the floor, 84 of the first 200
    finishing orders of seed 11 differ.)"""
    case = copy.deepcopy(O.load_case('S60'))
    case['base_pace'] = {d: 0.05 + 0.01 * i for i, d in enumerate(case['base_pace'])}
    case['config']['total_laps'] = 12
    return case


def run_inputs():
    """[(name, case, seed)]: 8 golden cases, 84 fuzz configurations, lap times near zero and at the overtake's floor, six
    synthetic field sizes."""
    return resume_inputs() + [(f'n{n}', RR.field_case(n), 5) for n in FIELD_SIZES]


def resume_inputs():
    """[(name, case, seed)]: 8 golden cases, 84 fuzz configurations, lap times near zero and at the overtake's floor."""
    out = [(name, O.load_case(name), 42) for name in GOLDEN]
    out += [(name, c, c['seed']) for name, c in fuzz_cases().items()]
    return out + [('near_zero', near_zero_case(), 11), ('floor', floor_case(), 11)]


def strategy_inputs():
    """[(name, case, seed)] of every fuzz configuration with at least 8 laps; the caller asserts that these are 75."""
    return [(name, c, c['seed']) for name, c in fuzz_cases().items() if c['config']['total_laps'] >= MIN_STRATEGY_LAPS]


def resume_laps(case, seed, sim):
    """The laps after which simulation `sim` is resumed: 1, 2, L // 2, L - 1, L where they exist, the lap of its first
    race event and the lap after it."""
    L = case['config']['total_laps']
    laps = {1, 2, L // 2, L - 1, L}
    e = RR.first_event_lap(case, seed, sim)
    if e is not None:
        laps |= {e, e + 1}
    return sorted(k for k in laps if 1 <= k <= L)


def many_from_one_lap(ref, i, L):
    """The lap after which traced simulation i's state is continued as many simulations: L // 2 if two cars still run
    there, else the last lap after which two do (a state with nobody running has nothing left to redraw or order), else
    L // 2."""
    running = (ref['trace']['dnf'][i] == 0).sum(axis=1)            # after lap 1 .. L
    k = max(1, L // 2)
    if running[k - 1] >= 2:
        return k
    laps = np.nonzero(running >= 2)[0]
    return int(laps[-1]) + 1 if laps.size else k


def grid_scenarios(n, L):
    """Six scenarios of a race of L >= 8 laps from the grid, as strategy_ref takes them ({driver: (start compound or -1,
    start age, [(lap, compound)])}): none; one stop; two stops; a start on aged HARD; as many stops on consecutive laps
    as a plan holds (laps 2..9, cut at L); stops on the first and the last lap that can have one."""
    assert L >= MIN_STRATEGY_LAPS
    return [
        {},
        {0: (-1, 0, [(max(2, L // 4), MEDIUM)])},
        {min(1, n - 1): (-1, 0, [(L // 3, HARD), (L - 1, SOFT)])},
        {n - 1: (HARD, 2, [(L // 2, MEDIUM)])},
        {0: (-1, 0, [(lap, (SOFT, MEDIUM, HARD)[lap % 3]) for lap in range(2, min(9, L) + 1)])},
        {n // 2: (-1, 0, [(2, HARD), (L, SOFT)])},
    ]


def state_scenarios(n, L, k):
    """Two scenarios of a race resumed after lap k = L // 2 (L >= 8): none; the first and the last driver stop on laps
    k + 1, k + 2 and L."""
    assert k + 2 < L
    stops = [(k + 1, MEDIUM), (k + 2, HARD), (L, SOFT)]
    return [{}, {d: (-1, 0, list(stops)) for d in sorted({0, n - 1})}]


def smallest_lap_time_ties(ref):
    """From the oracle's trace alone: the number of (simulation, lap >= 2) with two running cars sharing the smallest
    lap time of that lap."""
    tr = ref['trace']
    t = np.where(tr['dnf'][:, 1:, :] == 0, tr['last'][:, 1:, :], np.inf)
    best = t.min(axis=2, keepdims=True)
    return int((((t == best) & np.isfinite(t)).sum(axis=2) >= 2).sum())


def fastest_lap_ties(ref):
    """From the oracle's trace alone: (simulations whose smallest running lap time of the race, laps >= 2, is shared by
    two different drivers, simulations in which it is set on two different laps)."""
    tr = ref['trace']
    t = np.where(tr['dnf'][:, 1:, :] == 0, tr['last'][:, 1:, :], np.inf)          # [m][L - 1][n]
    if t.shape[1] == 0:
        return 0, 0
    hit = (t == t.min(axis=(1, 2), keepdims=True)) & np.isfinite(t)
    return int((hit.any(axis=1).sum(axis=1) >= 2).sum()), int((hit.any(axis=2).sum(axis=1) >= 2).sum())


def run_input_slices(k):
    """run_inputs() dealt into k lists for tests that take a slice each: together every input once, the 84 fuzz
    configurations among them."""
    inputs = run_inputs()
    parts = [inputs[i::k] for i in range(k)]
    names = [name for part in parts for name, _, _ in part]
    assert sorted(names) == sorted(name for name, _, _ in inputs) and len(set(names)) == len(inputs)
    assert sum(name in fuzz_cases() for name in names) == N_FUZZ
    return parts
