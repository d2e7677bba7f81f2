"""Price of per-simulation pace draws on the device, against the calls they are nearest to.

    python tools/priors_time.py [--simulations 1000000] [--case S60] [--seed 42] [--repeats 5] [--parent-lib PATH]
                                [--out FILE]

Every figure is the device time of one call (mcgp_last_kernel_ms: the race kernel and the counting kernel) over TWO
scenarios of `--simulations` simulations each of the golden case from the grid, in ms per 10^6 simulations:

    strategies_empty2   mcgp_run_strategies, two empty scenarios
    paces_all           mcgp_run_paces, an empty scenario and one with a LAPS [1, L] offset on every driver: the nearest
                        existing call, doing the same addition at every read of the base pace
    priors_empty2       mcgp_run_priors, two empty scenarios (the deltas counted, as in strategies_empty2)
    priors_drawn        mcgp_run_priors, an empty scenario and one with own sigma 0.15 on every driver and pair groups
                        (2t, 2t + 1) of sigma 0.2, the deltas and the by-draw counts over five edges counted

Each figure is taken `--repeats` times.  This process never opens the device: every round starts fresh child processes,
first one that loads the library at --parent-lib (a build of the parent commit, through MCGP_LIB; it times
strategies_empty2 and paces_all), then one that loads this tree's library and times all four, so the two builds
alternate on the same machine.  The spread of the parent's figures is the noise the others are read against.  Prints the
table, the launch shapes and one JSON line; --out also writes them to a file.
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

CONFIGS = ('strategies_empty2', 'paces_all', 'priors_empty2', 'priors_drawn')
EDGES = (-0.3, -0.1, 0.0, 0.1, 0.3)


def child(args):
    """One round in this process: warm every call up, then time each once; prints {config: ms per 10^6} and, under
    'shape', {config: [grid, block, LDS bytes]} of the call's race launch."""
    import oracle_py as O
    from monte_carlo_gp_amd import PaceOffset, RaceConfig, RaceSimulator
    from monte_carlo_gp_amd import _native as N
    c = O.load_case(args.case)
    drivers = list(c['grid_probs'])
    L = c['config']['total_laps']
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(grid_probs=c['grid_probs'], seed=args.seed, track_condition=c['track_condition'], drivers=drivers)
    has_priors = hasattr(N.lib(), 'mcgp_run_priors')
    drawn = []
    if has_priors:
        from monte_carlo_gp_amd import PacePrior
        drawn = [PacePrior.driver(d, 0.15) for d in drivers] + [PacePrior.group(drivers[i:i + 2], 0.2)
                                                                for i in range(0, len(drivers), 2)]
    shapes = {}

    def call(name, n):
        if name == 'strategies_empty2':
            sim.run_strategies(n, {'a': [], 'b': []}, *inputs, **kw)
        elif name == 'paces_all':
            sim.run_paces(n, {'none': [], 'all': [PaceOffset(d, 0.05 * (i % 5 - 2), laps=(1, L)) for i, d in enumerate(drivers)]},
                          None, *inputs, **kw)
        else:
            sim.run_priors(n, {'none': [], 'drawn': drawn if name == 'priors_drawn' else []}, EDGES, None, *inputs, **kw)
        ms = C.c_float()
        N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
        g, b, l = C.c_uint32(), C.c_uint32(), C.c_uint32()
        if N.lib().mcgp_last_launch_info(0, C.byref(g), C.byref(b), C.byref(l)) == 0:
            shapes[name] = [g.value, b.value, l.value]
        return ms.value

    names = [n for n in CONFIGS if has_priors or not n.startswith('priors')]
    if args.only:
        names = [n for n in names if n in args.only.split(',')]
    for name in names:                                      # warm-up: code objects, buffers
        call(name, min(args.simulations, 100_000))
    out = {name: call(name, args.simulations) / (args.simulations / 1e6) for name in names}
    out['shape'] = shapes
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=1_000_000)
    ap.add_argument('--case', default='S60')
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent-lib', default=None, help="a build of the parent commit's library, timed in alternation")
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--only', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    def round_of(lib, only=None):
        env = dict(os.environ)
        env.pop('MCGP_LIB', None)
        if lib:
            env['MCGP_LIB'] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', '--simulations', str(args.simulations), '--case',
               args.case, '--seed', str(args.seed)] + (['--only', only] if only else [])
        run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            raise SystemExit(f'a child failed ({run.returncode}): {run.stderr[-2000:]}')
        return json.loads(run.stdout.strip().splitlines()[-1])

    shared = ('strategies_empty2', 'paces_all')
    parent, tree, shape = {name: [] for name in shared}, {name: [] for name in CONFIGS}, {}
    for _ in range(args.repeats):
        if args.parent_lib:
            got = round_of(args.parent_lib, ','.join(shared))
            for name in shared:
                parent[name].append(got[name])
        got = round_of(None)
        shape = got.pop('shape')
        for name, ms in got.items():
            tree[name].append(ms)
    rows = ([(f'parent: {name}', parent[name]) for name in shared] if args.parent_lib else []) + [(name, tree[name]) for name in CONFIGS]
    lines = [f'{args.case}, {args.simulations} simulations x 2 scenarios per call, device ms per 10^6 simulations, '
             f'{args.repeats} runs each (fresh processes, the two builds alternating)',
             f"{'call':28} {'median':>8} {'min':>8} {'max':>8} {'max-min':>8}   runs"]
    for name, v in rows:
        lines.append(f'{name:28} {statistics.median(v):8.3f} {min(v):8.3f} {max(v):8.3f} {max(v) - min(v):8.3f}   '
                     + ' '.join(f'{x:.3f}' for x in v))
    med = statistics.median
    if args.parent_lib:
        lines.append(f"noise (spread of the parent's runs): strategies_empty2 {max(parent['strategies_empty2']) - min(parent['strategies_empty2']):.3f} ms, "
                     f"paces_all {max(parent['paces_all']) - min(parent['paces_all']):.3f} ms")
        lines.append(f"priors_empty2 / parent strategies_empty2, medians: x{med(tree['priors_empty2']) / med(parent['strategies_empty2']):.3f}; "
                     f"priors_drawn / parent paces_all: x{med(tree['priors_drawn']) / med(parent['paces_all']):.3f}; "
                     f"this tree's strategies_empty2 / the parent's: x{med(tree['strategies_empty2']) / med(parent['strategies_empty2']):.3f}")
    lines.append('race launch (grid x scenarios, block, LDS bytes): ' + '; '.join(f'{k} {v}' for k, v in shape.items()))
    doc = dict(case=args.case, simulations=args.simulations, scenarios=2, repeats=args.repeats,
               **{f'parent_{name}': [round(x, 3) for x in v] for name, v in parent.items()},
               **{name: [round(x, 3) for x in v] for name, v in tree.items()}, shape=shape)
    text = '\n'.join(lines) + '\n' + json.dumps(doc) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
