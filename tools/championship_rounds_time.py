"""Cost of the championship by round (mcgp_run_championship_rounds) against the plain championship call, and of this
tree's plain call against the parent commit's.

    python tools/championship_rounds_time.py --parent-lib PATH [--repeats 5] [--simulations 10000000] [--season 2024]
    python tools/championship_rounds_time.py --child plain|rounds [--simulations ...]        # one measurement

The first form starts one child process per measurement, one at a time (a child = warm-up of 100 000 simulations, then
the season's Grands Prix once at --simulations; device time from the library's events, mcgp_last_kernel_ms), in rounds
of: the parent's library running the plain call (MCGP_LIB=PATH: libmcgp_hip.so built from the parent commit), this
tree's plain call, this tree's by-round call.  Alternating the three keeps clock and thermal drift out of the ratios.
It prints every sample, then one JSON line with the medians, the spread (min, max) and the ratios new / parent.

The split of the by-round call's device time over its kernels comes from a run of its own:
`rocprofv3 --kernel-trace --stats -- python tools/championship_rounds_time.py --child rounds`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    from monte_carlo_gp_amd import cli, run_championship
    from monte_carlo_gp_amd import _native as N
    races = cli.championship_races(cli.championship_jobs(args.season, args.seed))
    by_round = args.child == 'rounds'
    run_championship(races, 100_000, by_round=by_round)                 # warm-up: code objects, buffers
    t0 = time.perf_counter()
    res = run_championship(races, args.simulations, by_round=by_round)
    wall = time.perf_counter() - t0
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    out = dict(mode=args.child, races=len(races), simulations=args.simulations, wall_s=round(wall, 4),
               device_ms=round(ms.value, 3), leader=max(res.title_probabilities, key=res.title_probabilities.get))
    if by_round:
        out['decided_by_round'] = [round(x, 6) for x in res.decided_by_round]
    print(json.dumps(out), flush=True)


def sample(mode, args, lib=None):
    env = dict(os.environ)
    env.pop('MCGP_LIB', None)
    if lib:
        env['MCGP_LIB'] = lib
    cmd = [sys.executable, os.path.abspath(__file__), '--child', mode, '--simulations', str(args.simulations),
           '--season', str(args.season), '--seed', str(args.seed)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f'{mode} child failed ({r.returncode}): {r.stderr[-2000:]}')
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=10_000_000)
    ap.add_argument('--season', type=int, default=2024)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent-lib', type=str, default=None, help="libmcgp_hip.so built from the parent commit")
    ap.add_argument('--child', choices=['plain', 'rounds'], default=None)
    ap.add_argument('--child-timeout', type=int, default=300)
    args = ap.parse_args()
    if args.child:
        return child(args)
    series = {'tree_plain': [], 'tree_rounds': []}
    if args.parent_lib:
        series = {'parent_plain': [], **series}
    for k in range(args.repeats):
        for name in series:
            s = sample('rounds' if name == 'tree_rounds' else 'plain', args,
                       os.path.abspath(args.parent_lib) if name == 'parent_plain' else None)
            series[name].append(s['device_ms'])
            print(f'repeat {k} {name:12} device {s["device_ms"]:9.3f} ms  wall {s["wall_s"]:.3f} s  leader {s["leader"]}',
                  flush=True)
    out = dict(simulations=args.simulations, repeats=args.repeats)
    for name, v in series.items():
        out[name] = dict(median_ms=round(statistics.median(v), 3), min_ms=min(v), max_ms=max(v))
    med = lambda k: out[k]['median_ms']
    out['rounds_over_plain'] = round(med('tree_rounds') / med('tree_plain'), 4)
    if args.parent_lib:
        out['rounds_over_parent'] = round(med('tree_rounds') / med('parent_plain'), 4)
        out['plain_over_parent'] = round(med('tree_plain') / med('parent_plain'), 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
