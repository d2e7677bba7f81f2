"""Price of combined what-if scenarios on the device, against the four single-kind calls they compose.

    python tools/combined_time.py [--simulations 1000000] [--case S60] [--seed 42] [--repeats 5] [--parent-lib PATH]
                                  [--out FILE]

Every figure is the device time of one call (mcgp_last_kernel_ms: the race kernel and the counting kernels) over TWO
scenarios of `--simulations` simulations each of the golden case from the grid, in ms per 10^6 simulations:

    strategies          mcgp_run_strategies, two empty scenarios
    penalties           mcgp_run_penalties, an empty scenario and one with 5 s to serve for the driver with the best base pace
    events              mcgp_run_events, an empty scenario and one with a safety car on lap L // 2
    paces               mcgp_run_paces, an empty scenario and one with +0.6 s from lap 5 until that driver's next stop
    combined_empty2     mcgp_run_combined, two empty scenarios
    combined_penalty    mcgp_run_combined, an empty scenario and the scenario of `penalties`
    combined_event      ... of `events`
    combined_pace       ... of `paces`
    combined_all        mcgp_run_combined, an empty scenario and one with all three items and that driver's stop on
                        lap L // 2

Each figure is taken `--repeats` times.  This process never opens the device: every round starts fresh child processes,
first one that loads the library at --parent-lib (a build of the parent commit, through MCGP_LIB; it times the four
single-kind calls, which is all it has), then one that loads this tree's library and times all nine, so the two builds
alternate on the same machine.  The spread of the parent's figures is the noise the others are read against; the
reference point of the combined figures is the dearest single-kind call of the parent.  Prints the table and one JSON
line; --out also writes both to a file.
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

SINGLE = ('strategies', 'penalties', 'events', 'paces')
COMBINED = ('combined_empty2', 'combined_penalty', 'combined_event', 'combined_pace', 'combined_all')


def child(args):
    """One round in this process: warm every call up, then time each once; prints {config: ms per 10^6}."""
    import oracle_py as O
    from monte_carlo_gp_amd import PaceOffset, PitPlan, RaceConfig, RaceEvent, RaceSimulator, TimePenalty
    from monte_carlo_gp_amd import _native as N
    c = O.load_case(args.case)
    drivers = list(c['grid_probs'])
    focus = min(drivers, key=lambda d: c['base_pace'][d])
    L = c['config']['total_laps']
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(grid_probs=c['grid_probs'], seed=args.seed, track_condition=c['track_condition'], drivers=drivers)
    mid = max(L // 2, 2)
    pen, ev = [TimePenalty(focus, 5.0)], [RaceEvent('sc', mid)]
    off = [PaceOffset(focus, 0.6, until_stop_from=min(5, L))]
    combined = dict(combined_empty2={}, combined_penalty=dict(penalties=pen), combined_event=dict(events=ev),
                    combined_pace=dict(paces=off),
                    combined_all=dict(penalties=pen, events=ev, paces=off, plans=[PitPlan(focus, [(mid, 'HARD')])]))

    def call(name, n):
        if name == 'strategies':
            sim.run_strategies(n, {'a': [], 'b': []}, *inputs, **kw)
        elif name == 'penalties':
            sim.run_penalties(n, {'none': [], 'item': pen}, None, *inputs, **kw)
        elif name == 'events':
            sim.run_events(n, {'none': [], 'item': ev}, None, *inputs, **kw)
        elif name == 'paces':
            sim.run_paces(n, {'none': [], 'item': off}, None, *inputs, **kw)
        else:
            sim.run_combined(n, {'none': {}, 'item': combined[name]}, *inputs, allow_single_compound=True, **kw)
        ms = C.c_float()
        N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
        return ms.value

    names = list(SINGLE) + (list(COMBINED) if hasattr(N.lib(), 'mcgp_run_combined') else [])
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

    parent, tree = {name: [] for name in SINGLE}, {name: [] for name in SINGLE + COMBINED}
    for _ in range(args.repeats):
        if args.parent_lib:
            for name, ms in round_of(args.parent_lib, ','.join(SINGLE)).items():
                parent[name].append(ms)
        for name, ms in round_of(None).items():
            tree[name].append(ms)
    rows = ([(f'parent: {name}', parent[name]) for name in SINGLE] if args.parent_lib else []) \
        + [(name, tree[name]) for name in SINGLE + COMBINED]
    lines = [f'{args.case}, {args.simulations} simulations x 2 scenarios per call, device ms per 10^6 simulations, '
             f'{args.repeats} runs each (fresh processes, the two builds alternating)',
             f"{'call':28} {'median':>8} {'min':>8} {'max':>8} {'max-min':>8}   runs"]
    for name, v in rows:
        lines.append(f'{name:28} {statistics.median(v):8.3f} {min(v):8.3f} {max(v):8.3f} {max(v) - min(v):8.3f}   '
                     + ' '.join(f'{x:.3f}' for x in v))
    if args.parent_lib:
        med = {name: statistics.median(parent[name]) for name in SINGLE}
        dearest = max(med, key=med.get)
        lines.append(f'dearest single-kind call of the parent: {dearest}, {med[dearest]:.3f} ms (spread '
                     f'{max(parent[dearest]) - min(parent[dearest]):.3f}); against it, medians: '
                     + ', '.join(f'{name} {statistics.median(tree[name]) / med[dearest] - 1:+.1%}' for name in COMBINED))
    doc = dict(case=args.case, simulations=args.simulations, scenarios=2, repeats=args.repeats,
               parent={name: [round(x, 3) for x in v] for name, v in parent.items()},
               **{name: [round(x, 3) for x in v] for name, v in tree.items()})
    text = '\n'.join(lines) + '\n' + json.dumps(doc) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
