"""Cost of the race time gaps (mcgp_run_gaps) on the device against the race trace (mcgp_run_trace).

    python tools/gaps_time.py [--simulations 1000000] [--case S60] [--seed 42] [--repeats 5] [--pairs 0 4]
                              [--trace-lib PATH] [--skip-trace]

Runs the golden case through RaceSimulator.run_gaps with the default edges, once per --pairs count (pairs of the first
drivers), and through mcgp_run_trace, with the same seed, after a small warm-up of each, alternating them `--repeats`
times, and prints one JSON line: the device time the library's events give for each call (mcgp_last_kernel_ms: the whole
call, counting kernels included), the medians, each gaps median's ratio to the trace median, and the staging-byte ratio
(n + 1 + P) / n the gaps call is expected to stay within.

--trace-lib PATH: take mcgp_run_trace from another build of the library (the parent commit's libmcgp_hip.so), in a child
process of its own (MCGP_LIB names the library a process loads) that runs before this one opens the device, so that the
yardstick is not this tree's own trace build.  The split of the gaps call into race_gaps_kernel and gaps_count_rows
comes from a run under
`rocprofv3 --kernel-trace --stats -- python tools/gaps_time.py --skip-trace --repeats 1`.
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import oracle_py as O  # noqa: E402
from monte_carlo_gp_amd import RaceConfig, RaceSimulator  # noqa: E402
from monte_carlo_gp_amd import _native as N  # noqa: E402


def kernel_ms():
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    return ms.value


def trace_times(args):
    """Device ms of `--repeats` mcgp_run_trace calls after a warm-up, in this process (whose library MCGP_LIB chose)."""
    c = O.load_case(args.case)
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['grid_probs'], c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(seed=args.seed, track_condition=c['track_condition'])
    sim.run_trace(100_000, *inputs, **kw)
    out = []
    for _ in range(args.repeats):
        sim.run_trace(args.simulations, *inputs, **kw)
        out.append(round(kernel_ms(), 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=1_000_000)
    ap.add_argument('--case', default='S60')
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--pairs', type=int, nargs='+', default=[0, 4], help='numbers of pairs to time')
    ap.add_argument('--trace-lib', default=None, help="another build's libmcgp_hip.so to take mcgp_run_trace from")
    ap.add_argument('--skip-trace', action='store_true', help='time the gaps calls only (profiler runs)')
    ap.add_argument('--trace-only', action='store_true', help=argparse.SUPPRESS)      # the --trace-lib child
    args = ap.parse_args()
    if args.trace_only:
        print(json.dumps(dict(trace_device_ms=trace_times(args))))
        return
    lib_trace = []
    if args.trace_lib:
        # first, while this process has not touched the device: a child started afterwards would be a fork of a process
        # with the GPU open
        cmd = [sys.executable, os.path.abspath(__file__), '--trace-only', '--simulations', str(args.simulations), '--case',
               args.case, '--seed', str(args.seed), '--repeats', str(args.repeats)]
        r = subprocess.run(cmd, env=dict(os.environ, MCGP_LIB=os.path.abspath(args.trace_lib)), capture_output=True,
                           text=True, check=True)
        lib_trace = json.loads(r.stdout.strip().splitlines()[-1])['trace_device_ms']
    c = O.load_case(args.case)
    drivers = list(c['grid_probs'])
    n = len(drivers)
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['grid_probs'], c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(seed=args.seed, track_condition=c['track_condition'])
    pair_sets = {p: [(drivers[i], drivers[i + 1]) for i in range(p)] for p in args.pairs}

    def gaps(count, pairs):
        t0 = time.perf_counter()
        res = sim.run_gaps(count, *inputs, pairs=pairs, **kw)
        return time.perf_counter() - t0, kernel_ms(), res

    for pairs in pair_sets.values():
        gaps(100_000, pairs)                                # warm-up: code objects, buffers
    own_trace = not args.skip_trace and not args.trace_lib
    if own_trace:
        sim.run_trace(100_000, *inputs, **kw)
    g_dev = {p: [] for p in pair_sets}
    t_dev, res, name = [], None, ''
    for _ in range(args.repeats):
        for p, pairs in pair_sets.items():
            _, dev, res = gaps(args.simulations, pairs)
            g_dev[p].append(round(dev, 3))
            name = N.lib().mcgp_last_kernel_name(0).decode()
        if own_trace:
            t = sim.run_trace(args.simulations, *inputs, **kw)
            t_dev.append(round(kernel_ms(), 3))
            assert (t.hist == res.hist).all(), 'run_gaps and run_trace histograms differ'
    out = dict(case=args.case, simulations=args.simulations, kernel=name,
               gaps_device_ms={str(p): v for p, v in g_dev.items()},
               gaps_device_ms_median={str(p): statistics.median(v) for p, v in g_dev.items()},
               winning_margin_under_5s=res.winning_margin_under(5.0))
    if args.trace_lib:
        t_dev = lib_trace
        out['trace_lib'] = args.trace_lib
    if t_dev:
        med = statistics.median(t_dev)
        out.update(trace_device_ms=t_dev, trace_device_ms_median=med,
                   ratio_to_trace={str(p): round(statistics.median(v) / med, 4) for p, v in g_dev.items()},
                   staging_byte_ratio={str(p): round((n + 1 + p) / n, 4) for p in g_dev})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
