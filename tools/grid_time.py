"""Price of grid scenarios on the device, against the pit-strategy comparison they are built on.

    python tools/grid_time.py [--simulations 1000000] [--case S60] [--seed 42] [--repeats 5] [--parent-lib PATH]
                              [--out FILE]

Every figure is the device time of one call (mcgp_last_kernel_ms: the race kernel and the counting kernels) over TWO
scenarios of `--simulations` simulations each of the golden case from the grid, in ms per 10^6 simulations:

    strategies_empty2   mcgp_run_strategies, two empty scenarios
    grids_empty2        mcgp_run_grids, two empty scenarios, start_out and gain_out not wanted
    drop_one            mcgp_run_grids, an empty scenario and one that drops the first driver ten places, start_out and
                        gain_out not wanted
    pit_lane_counted    mcgp_run_grids, an empty scenario and one that starts the first driver from the pit lane, with
                        start_out and gain_out

Each figure is taken `--repeats` times.  This process never opens the device: every round starts fresh child processes,
first one that loads the library at --parent-lib (a build of the parent commit, through MCGP_LIB; it times
strategies_empty2 only), then one that loads this tree's library and times all four, so the two builds alternate on the
same machine.  The spread of the parent's figures is the noise the others are read against.  Prints the table and one
JSON line; --out also writes both to a file.
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

CONFIGS = ('strategies_empty2', 'grids_empty2', 'drop_one', 'pit_lane_counted')


def child(args):
    """One round in this process: warm every call up, then time each once; prints {config: ms per 10^6}."""
    import grids_ref as GR
    import oracle_py as O
    import resume_ref as RR
    import strategy_ref as SR
    from monte_carlo_gp_amd import _native as N
    case = O.load_case(args.case)
    prob = RR.problem(case)
    has_grids = hasattr(N.lib(), 'mcgp_run_grids')
    runs = dict(grids_empty2=([{}, {}], False), drop_one=([{}, {0: (GR.DROP, 10, 0.0)}], False),
                pit_lane_counted=([{}, {0: (GR.PIT_LANE, 0, 2.5)}], True))

    def call(name, n):
        if name == 'strategies_empty2':
            rc = SR.run_c(case, [{}, {}], n, args.seed, orders=False, prob=prob)[0]
        else:
            edits, counted = runs[name]
            rc = GR.run_c(case, None, edits, n, args.seed, orders=False, start=counted, gain=counted, prob=prob)[0]
        N.check(rc)
        ms = C.c_float()
        N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
        return ms.value

    names = [n for n in CONFIGS if n == 'strategies_empty2' or has_grids]
    if args.only:
        names = [n for n in names if n in args.only.split(',')]
    for name in names:                                      # warm-up: code objects, buffers
        call(name, min(args.simulations, 100_000))
    out = {name: call(name, args.simulations) / (args.simulations / 1e6) for name in names}
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

    parent, tree = [], {name: [] for name in CONFIGS}
    for _ in range(args.repeats):
        if args.parent_lib:
            parent.append(round_of(args.parent_lib, 'strategies_empty2')['strategies_empty2'])
        for name, ms in round_of(None).items():
            tree[name].append(ms)
    rows = ([('parent: strategies_empty2', parent)] if parent else []) + [(name, tree[name]) for name in CONFIGS]
    lines = [f'{args.case}, {args.simulations} simulations x 2 scenarios per call, device ms per 10^6 simulations, '
             f'{args.repeats} runs each (fresh processes, the two builds alternating)',
             f"{'call':28} {'median':>8} {'min':>8} {'max':>8} {'max-min':>8}   runs"]
    for name, v in rows:
        lines.append(f'{name:28} {statistics.median(v):8.3f} {min(v):8.3f} {max(v):8.3f} {max(v) - min(v):8.3f}   '
                     + ' '.join(f'{x:.3f}' for x in v))
    if parent:
        ref = statistics.median(parent)
        lines.append(f'noise (spread of the parent\'s runs): {max(parent) - min(parent):.3f} ms; against the parent\'s median: '
                     + ', '.join(f'{name} x{statistics.median(tree[name]) / ref:.4f}' for name in CONFIGS))
    doc = dict(case=args.case, simulations=args.simulations, scenarios=2, repeats=args.repeats,
               parent_strategies_empty2=[round(x, 3) for x in parent],
               **{name: [round(x, 3) for x in v] for name, v in tree.items()})
    text = '\n'.join(lines) + '\n' + json.dumps(doc) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
