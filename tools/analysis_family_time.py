"""The five analysis calls from the grid and from a mid-race state, and the matchups call, timed in one process, for
comparing two builds.

    [MCGP_LIB=/path/to/another/build/libmcgp_hip.so] python tools/analysis_family_time.py [--simulations 1000000]
                                       [--repeats 3] [--lap 30] [--seed 42] [--dump FILE.npz]

On S60, `--simulations` simulations each: run_trace from the grid; run_gaps (the default edges, two pairs),
run_conditions (six conditions, with the conditional histograms), run_stints and run_moves (every output) from the grid
and from the state the CPU oracle traced for simulation 0 after `--lap` laps; run_matchups with the podium counts.  After
a warm-up call of the same size (code objects, the workspace at its full size) every call is timed `--repeats` times:
the device time of the whole call from the library's events (mcgp_last_kernel_ms: the counting kernels included).
Prints one JSON line ({call_source: {ms: [...], kernel: name}}, the library and its build hash).  --dump keeps every
integer array of the last timed results in an .npz, so that two builds can be compared with numpy.array_equal.  The
library is this tree's unless MCGP_LIB names another: profiles/analysis_family_time.txt runs parent / new alternating
that way, each process a fresh one.
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
from monte_carlo_gp_amd import RaceConfig, RaceSimulator  # noqa: E402
from monte_carlo_gp_amd import _native as N  # noqa: E402


def integer_arrays(result):
    """{name: array} of a result object's integer arrays (ConditionResult keeps its counts in a dict)."""
    out = {k: v for k, v in vars(result).items() if isinstance(v, np.ndarray) and v.dtype.kind in 'iu'}
    if isinstance(getattr(result, 'counts', None), dict):
        out['counts'] = np.array(list(result.counts.values()), np.uint64)
    return out


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
    a, b, d = drivers[0], drivers[1], drivers[2]
    ref = RR.traced_run(c, 1, args.seed)
    state = RR.race_state(RR.state_arrays(ref, 0, args.lap), args.lap, RR.drs_disabled_until(c, args.seed, 0, args.lap),
                          drivers)
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = dict(base_pace=c['base_pace'], tire_deg=c['tire_deg'], driver_variance=c['driver_variance'],
                  driver_dnf_rates=c['driver_dnf_rates'], seed=args.seed, track_condition=c['track_condition'])
    texts = {'double': f'{a}.wins & {b}.podium', 'sc': 'sc>=1', 'out': f'{b}.dnf', 'gain': f'{d}.gain>=3',
             'few': 'finishers<16', 'beats': f'{b}.beats.{a}'}
    sources = {'grid': dict(grid_probs=c['grid_probs']), 'state': dict(state=state, drivers=drivers)}
    calls = {'trace_grid': lambda m: sim.run_trace(m, c['grid_probs'], **inputs),
             'matchups_grid': lambda m: sim.run_matchups(m, c['grid_probs'], **inputs)}
    for src, kw in sources.items():
        calls[f'gaps_{src}'] = lambda m, kw=kw: sim.run_gaps(m, pairs=[(a, b), (b, d)], **kw, **inputs)
        calls[f'conditions_{src}'] = lambda m, kw=kw: sim.run_conditions(m, texts, **kw, **inputs)
        calls[f'stints_{src}'] = lambda m, kw=kw: sim.run_stints(m, **kw, **inputs)
        calls[f'moves_{src}'] = lambda m, kw=kw: sim.run_moves(m, **kw, **inputs)

    def timed(call, m):
        r = call(m)
        ms = C.c_float()
        N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
        return ms.value, r, N.lib().mcgp_last_kernel_name(0).decode()

    out, dump = {}, {}
    for name, call in calls.items():
        timed(call, args.simulations)                            # warm-up at the timed size: code objects, the workspace
        runs = [timed(call, args.simulations) for _ in range(args.repeats)]
        out[name] = dict(ms=[round(t, 3) for t, _, _ in runs], kernel=runs[-1][2])
        if args.dump:
            for k, v in integer_arrays(runs[-1][1]).items():
                dump[f'{name}.{k}'] = v
    if args.dump:
        np.savez_compressed(args.dump, **dump)
    print(json.dumps(dict(tool='analysis_family_time', lib=os.environ.get('MCGP_LIB', 'tree'), build_hash=N.build_hash(),
                          simulations=args.simulations, arrays=len(dump), **out)))


if __name__ == '__main__':
    main()
