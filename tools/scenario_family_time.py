"""The five scenario calls from the grid and from a mid-race state, timed in one process, for comparing two builds.

    [MCGP_LIB=/path/to/another/build/libmcgp_hip.so] python tools/scenario_family_time.py [--simulations 1000000]
                                       [--repeats 3] [--lap 30] [--seed 42] [--dump FILE.npz]

run_strategies, run_penalties, run_events, run_paces and run_combined on S60, each over TWO scenarios of
`--simulations` simulations: an empty one and one with the call's item (a planned stop onto HARD for the driver with the
best base pace; 5 s to serve; a safety car; +0.6 s until the next stop; all of them), from the grid and from the state the
CPU oracle traced for simulation 0 after `--lap` laps.  After a warm-up call of 10^5 every call is timed `--repeats`
times: the device time of the whole call from the library's events (mcgp_last_kernel_ms).  Prints one JSON line
({call_source: {ms: [...], kernel: name}}, the library and its build hash).  --dump keeps every integer array of the
last timed results (hist, delta, fate, events, carried) in an .npz, so that two builds can be compared with
numpy.array_equal.  The library is this tree's unless MCGP_LIB names another: profiles/scenario_family_time.txt runs
parent / new / parent / new that way, each process a fresh one.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import oracle_py as O  # noqa: E402
import resume_ref as RR  # noqa: E402
from monte_carlo_gp_amd import PaceOffset, PitPlan, RaceConfig, RaceEvent, RaceSimulator, TimePenalty  # noqa: E402
from monte_carlo_gp_amd import _native as N  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=1_000_000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--lap', type=int, default=30)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--dump', default=None)
    args = ap.parse_args()
    c = O.load_case('S60')
    drivers = list(c['grid_probs'])
    focus = min(drivers, key=lambda d: c['base_pace'][d])
    L = c['config']['total_laps']
    ref = RR.traced_run(c, 1, args.seed)
    state = RR.race_state(RR.state_arrays(ref, 0, args.lap), args.lap, RR.drs_disabled_until(c, args.seed, 0, args.lap),
                          drivers)
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    base = dict(seed=args.seed, track_condition=c['track_condition'], drivers=drivers)
    out, dump = {}, {}
    for src in ('grid', 'state'):
        kw = dict(base, grid_probs=c['grid_probs']) if src == 'grid' else dict(base, state=state)
        first = 2 if src == 'grid' else args.lap + 1
        mid = max((first + L) // 2, first)
        pen, ev = [TimePenalty(focus, 5.0)], [RaceEvent('sc', mid)]
        off = [PaceOffset(focus, 0.6, until_stop_from=min(first + 3, L))]
        everything = dict(penalties=pen, events=ev, paces=off, plans=[PitPlan(focus, [(mid, 'HARD')])])

        def call(name, n):
            if name == 'strategies':
                r = sim.run_strategies(n, {'a': [], 'b': [PitPlan(focus, [(mid, 'HARD')])]}, *inputs,
                                       allow_single_compound=True, **kw)
            elif name == 'penalties':
                r = sim.run_penalties(n, {'none': [], 'item': pen}, None, *inputs, **kw)
            elif name == 'events':
                r = sim.run_events(n, {'none': [], 'item': ev}, None, *inputs, **kw)
            elif name == 'paces':
                r = sim.run_paces(n, {'none': [], 'item': off}, None, *inputs, **kw)
            else:
                r = sim.run_combined(n, {'none': {}, 'item': everything}, *inputs, allow_single_compound=True, **kw)
            ms = C.c_float()
            N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
            return ms.value, r, N.lib().mcgp_last_kernel_name(0).decode()

        for name in ('strategies', 'penalties', 'events', 'paces', 'combined'):
            call(name, 100_000)
            runs = [call(name, args.simulations) for _ in range(args.repeats)]
            out[f'{name}_{src}'] = dict(ms=[round(t, 3) for t, _, _ in runs], kernel=runs[-1][2])
            if args.dump:
                for k, v in vars(runs[-1][1]).items():
                    if isinstance(v, np.ndarray) and v.dtype.kind in 'iu':
                        dump[f'{name}_{src}.{k}'] = v
    if args.dump:
        np.savez_compressed(args.dump, **dump)
    print(json.dumps(dict(tool='scenario_family_time', lib=os.environ.get('MCGP_LIB', 'tree'), build_hash=N.build_hash(),
                          simulations=args.simulations, arrays=len(dump), **out)))


if __name__ == '__main__':
    main()
