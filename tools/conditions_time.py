"""Cost of combination and conditional odds (mcgp_run_conditions) on the device, against the race trace (mcgp_run_trace)
and the plain generic run (mcgp_run under MCGP_FORCE_GENERIC=1) of another build of the library.

    python tools/conditions_time.py [--simulations 1000000] [--case S60] [--seed 42] [--lap 30] [--repeats 3] [--rounds 2]
                                    [--conditions 1 16 64] [--parent-lib PATH]

Times RaceSimulator.run_conditions on the golden case from the grid and from the state the CPU oracle traced for
simulation 0 after `--lap` laps, with C = each of --conditions conditions of 8 atoms (seeded, wide ranges, so that the
conjunctions are met by a part of the simulations), with and without the conditional histograms, `--repeats` times each
after a warm-up, and prints one JSON line: the device time the library's events give for each call (mcgp_last_kernel_ms:
the whole call, the counting kernel included), medians, spreads (max - min) and the met fractions.

--parent-lib PATH: also time mcgp_run_trace and the plain generic mcgp_run of that build (the parent commit's
libmcgp_hip.so; MCGP_LIB names the library a process loads).  Every measurement runs in a child process of its own kind,
this tree's and the parent's alternating `--rounds` times; the process that prints never opens the device.  The line
then carries the two relations: conditions (C = 64, grid, histograms) / parent trace, and conditions (C = 1, grid,
histograms) / parent generic run.  The split of a call into race_conditions_kernel and conditions_count comes from a run
under `rocprofv3 --kernel-trace --stats -- python tools/conditions_time.py --child own --repeats 1`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def kernel_ms(N):
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    return round(ms.value, 3)


def timing_conditions(count, n, L, seed=1):
    """`count` conditions of 8 atoms: seven wide atoms (nearly always true) and one that splits the field."""
    import numpy as np
    from monte_carlo_gp_amd import _native as N
    from monte_carlo_gp_amd.conditions import INT_MAX, INT_MIN, Atom, Condition
    rng = np.random.default_rng(seed)
    out = {}
    for c in range(count):
        d = [int(x) for x in rng.permutation(n)[:4]]
        atoms = [Atom(N.FACT_POSITION, d[0], 0, 1, int(rng.integers(n // 4 + 1, n + 1))),        # the splitting atom
                 Atom(N.FACT_GRID, d[1], 0, 1, n - 1), Atom(N.FACT_RETIRED_LAP, d[2], 0, 0, L // 2),
                 Atom(N.FACT_AHEAD_BY, d[0], d[3], -n, n), Atom(N.FACT_GAINED, d[1], 0, -n + 2, INT_MAX),
                 Atom(N.FACT_FINISHERS, 0, 0, n - 8, INT_MAX), Atom(N.FACT_SAFETY_CARS, 0, 0, INT_MIN, 4),
                 Atom(N.FACT_VSCS, 0, 0, 0, 0, negate=bool(c & 1))]
        out[f'c{c}'] = Condition(tuple(atoms))
    return out


def child(args):
    import oracle_py as O
    import resume_ref as RR
    from monte_carlo_gp_amd import RaceConfig, RaceSimulator
    from monte_carlo_gp_amd import _native as N
    c = O.load_case(args.case)
    drivers = list(c['grid_probs'])
    n, L = len(drivers), c['config']['total_laps']
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(seed=args.seed, track_condition=c['track_condition'])
    out = {}
    if args.child == 'parent':
        def trace(m):
            sim.run_trace(m, c['grid_probs'], *inputs, **kw)
            return kernel_ms(N)

        def generic(m):
            os.environ['MCGP_FORCE_GENERIC'] = '1'
            try:
                sim.run_monte_carlo(m, c['grid_probs'], *inputs, **kw)
                return kernel_ms(N)
            finally:
                del os.environ['MCGP_FORCE_GENERIC']
        trace(100_000), generic(100_000)                         # warm-up: code objects, buffers
        out = {'trace': [], 'generic': []}
        for _ in range(args.repeats):
            out['trace'].append(trace(args.simulations))
            out['generic'].append(generic(args.simulations))
        out['generic_kernel'] = N.lib().mcgp_last_kernel_name(0).decode()
    else:
        ref = RR.traced_run(c, 1, args.seed)
        state = RR.race_state(RR.state_arrays(ref, 0, args.lap), args.lap, RR.drs_disabled_until(c, args.seed, 0, args.lap),
                              drivers)
        sets = {k: timing_conditions(k, n, L) for k in args.conditions}
        met = {}

        def run(m, k, path, hists):
            start = dict(grid_probs=c['grid_probs']) if path == 'grid' else dict(state=state, drivers=drivers)
            res = sim.run_conditions(m, sets[k], base_pace=c['base_pace'], tire_deg=c['tire_deg'],
                                     driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'],
                                     histograms=hists, **start, **kw)
            met[f'{path}_C{k}'] = round(sum(res.counts.values()) / (k * m), 4)
            return kernel_ms(N)
        keys = [(k, path, hists) for k in args.conditions for path in ('grid', 'state') for hists in (True, False)]
        for k, path, hists in keys:
            run(100_000, k, path, hists)
        for _ in range(args.repeats):
            for k, path, hists in keys:
                out.setdefault(f'{path}_C{k}_{"hist" if hists else "count"}', []).append(run(args.simulations, k, path, hists))
        out['met_fraction'] = met
        out['kernel'] = N.lib().mcgp_last_kernel_name(0).decode()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=1_000_000)
    ap.add_argument('--case', default='S60')
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--lap', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=3, help='timed calls of each kind per child process')
    ap.add_argument('--rounds', type=int, default=2, help='child processes of each library, alternating')
    ap.add_argument('--conditions', type=int, nargs='+', default=[1, 16, 64])
    ap.add_argument('--parent-lib', default=None, help="another build's libmcgp_hip.so: its trace and generic run")
    ap.add_argument('--child', choices=('own', 'parent'), default=None, help='measure in this process (profiler runs)')
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    base = [sys.executable, os.path.abspath(__file__), '--simulations', str(args.simulations), '--case', args.case, '--seed',
            str(args.seed), '--lap', str(args.lap), '--repeats', str(args.repeats), '--conditions'] + \
        [str(k) for k in args.conditions]
    own, parent = {}, {}

    def merge(into, part):
        for k, v in part.items():
            if isinstance(v, list):
                into.setdefault(k, []).extend(v)
            else:
                into[k] = v

    for _ in range(args.rounds):
        if args.parent_lib:
            env = dict(os.environ, MCGP_LIB=os.path.abspath(args.parent_lib))
            r = subprocess.run(base + ['--child', 'parent'], env=env, capture_output=True, text=True, check=True)
            merge(parent, json.loads(r.stdout.strip().splitlines()[-1]))
        env = {k: v for k, v in os.environ.items() if k != 'MCGP_LIB'}
        r = subprocess.run(base + ['--child', 'own'], env=env, capture_output=True, text=True, check=True)
        merge(own, json.loads(r.stdout.strip().splitlines()[-1]))
    times = {k: v for k, v in own.items() if isinstance(v, list)}
    spread = lambda v: round(max(v) - min(v), 3)
    out = dict(case=args.case, simulations=args.simulations, lap=args.lap, kernel=own.get('kernel'),
               conditions_device_ms=times, conditions_device_ms_median={k: statistics.median(v) for k, v in times.items()},
               conditions_device_ms_spread={k: spread(v) for k, v in times.items()}, met_fraction=own.get('met_fraction'))
    if args.parent_lib:
        t, g = parent['trace'], parent['generic']
        out.update(parent_lib=args.parent_lib, parent_trace_device_ms=t, parent_trace_device_ms_median=statistics.median(t),
                   parent_trace_device_ms_spread=spread(t), parent_generic_device_ms=g,
                   parent_generic_device_ms_median=statistics.median(g), parent_generic_device_ms_spread=spread(g),
                   parent_generic_kernel=parent.get('generic_kernel'))
        top, one = f'grid_C{max(args.conditions)}_hist', f'grid_C{min(args.conditions)}_hist'
        out['ratio_to_parent_trace'] = {top: round(statistics.median(times[top]) / statistics.median(t), 4)}
        out['ratio_to_parent_generic'] = {one: round(statistics.median(times[one]) / statistics.median(g), 4)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
