"""Cost of the race movement counts (mcgp_run_moves) on the device against the race trace (mcgp_run_trace).

    python tools/moves_time.py [--simulations 1000000] [--case S60] [--seed 42] [--repeats 5] [--trace-lib PATH]
                                [--skip-trace] [--skip-moves]

Runs the golden case through RaceSimulator.run_moves and through mcgp_run_trace with the same seed, after a small
warm-up of each, alternating them `--repeats` times, and prints one JSON line: the device time the library's events give
for each call (mcgp_last_kernel_ms: the whole call, counting kernels included), the medians, the max - min spread of the
trace repeats and the allowance of the expectation stated before the first measurement: the race kernel stages (L + 2) n
bytes per simulation where the trace stages L n, so race_moves_kernel should sit within the trace kernel's own spread
plus 2 / L of the trace median.  The JSON line reports the whole call's excess over the trace median beside that
allowance; the call also runs two counting kernels of its own, whose time the profiler run gives.

--trace-lib PATH: take mcgp_run_trace from another build of the library (the parent commit's libmcgp_hip.so), so that
the yardstick is not this tree's own trace build.  MCGP_LIB names the library a process loads, so every measured call
then runs in a child process of its own (warm-up, then one timed call), trace and moves in turn; this process never
opens the device.  The split of the moves call into race_moves_kernel, moves_count_laps and moves_count_drivers comes
from a run under
`rocprofv3 --kernel-trace --stats -- python tools/moves_time.py --skip-trace --repeats 1`.
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

import oracle_py as O  # noqa: E402
from monte_carlo_gp_amd import RaceConfig, RaceSimulator  # noqa: E402
from monte_carlo_gp_amd import _native as N  # noqa: E402


def kernel_ms():
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    return round(ms.value, 3)


class Runner:
    """The two calls on one case, in this process (whose library MCGP_LIB chose)."""

    def __init__(self, args):
        c = O.load_case(args.case)
        self.sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
        self.inputs = (c['grid_probs'], c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
        self.kw = dict(seed=args.seed, track_condition=c['track_condition'])

    def trace(self, count):
        res = self.sim.run_trace(count, *self.inputs, **self.kw)
        return kernel_ms(), res

    def moves(self, count):
        res = self.sim.run_moves(count, *self.inputs, **self.kw)
        return kernel_ms(), res


def child(args, what, lib=None):
    """One timed call of `what` ('trace' or 'moves') after its warm-up, in a process of its own -> device ms."""
    cmd = [sys.executable, os.path.abspath(__file__), '--one', what, '--simulations', str(args.simulations), '--case',
           args.case, '--seed', str(args.seed)]
    env = dict(os.environ, MCGP_LIB=os.path.abspath(lib)) if lib else dict(os.environ)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, check=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=1_000_000)
    ap.add_argument('--case', default='S60')
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--trace-lib', default=None, help="another build's libmcgp_hip.so to take mcgp_run_trace from")
    ap.add_argument('--skip-trace', action='store_true', help='time the moves call only (profiler runs)')
    ap.add_argument('--skip-moves', action='store_true',
                    help='with --trace-lib: time the trace call only (its spread, before the first moves measurement)')
    ap.add_argument('--one', choices=('trace', 'moves'), default=None, help=argparse.SUPPRESS)      # a --trace-lib child
    args = ap.parse_args()
    if args.one:
        run = Runner(args)
        call = run.trace if args.one == 'trace' else run.moves
        call(100_000)                                       # warm-up: code objects, buffers
        ms, res = call(args.simulations)
        print(json.dumps(dict(device_ms=ms, wins=[int(x) for x in res.hist[:, 0]])))
        return
    s_dev, t_dev, name, per_race = [], [], 'mcgp::race_moves_kernel', None
    if args.trace_lib:
        for _ in range(args.repeats):
            t = child(args, 'trace', args.trace_lib)
            t_dev.append(t['device_ms'])
            if args.skip_moves:
                continue
            s = child(args, 'moves')
            assert t['wins'] == s['wins'], 'run_moves and run_trace histograms differ'
            s_dev.append(s['device_ms'])
    else:
        run = Runner(args)
        run.moves(100_000)
        if not args.skip_trace:
            run.trace(100_000)
        for _ in range(args.repeats):
            ms, res = run.moves(args.simulations)
            s_dev.append(ms)
            name = N.lib().mcgp_last_kernel_name(0).decode()
            per_race = res.expected_race_passes()
            if not args.skip_trace:
                ms, t = run.trace(args.simulations)
                t_dev.append(ms)
                assert (t.hist == res.hist).all(), 'run_moves and run_trace histograms differ'
    out = dict(case=args.case, simulations=args.simulations, kernel=name)
    if s_dev:
        out.update(moves_device_ms=s_dev, moves_device_ms_median=statistics.median(s_dev))
    if per_race is not None:
        out['on_track_passes_per_race'] = per_race
    if args.trace_lib:
        out['trace_lib'] = args.trace_lib
    if t_dev:
        med, spread = statistics.median(t_dev), round(max(t_dev) - min(t_dev), 3)
        laps = O.load_case(args.case)['config']['total_laps']
        allowance = round(spread + 2.0 / laps * med, 3)
        out.update(trace_device_ms=t_dev, trace_device_ms_median=med, trace_spread_ms=spread,
                   race_kernel_allowance_ms=allowance)
        if s_dev:
            out['excess_ms'] = round(out['moves_device_ms_median'] - med, 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
