"""Cost of the race trace (lap-by-lap counts) on the device against the generic kernel's plain race.

    python tools/trace_time.py [--simulations 10000000] [--case S60] [--seed 42] [--repeats 3] [--skip-plain]

Runs the golden case through RaceSimulator.run_trace and through RaceSimulator.run_monte_carlo on the generic LDS kernel
(MCGP_FORCE_GENERIC=1, set by this script: the trace runs on that kernel's code), with the same seed, after a small
warm-up of both, alternating the two `--repeats` times, and prints one JSON line: the device time the library's events
give for each call (mcgp_last_kernel_ms: the whole trace call, counting kernels included; the race kernel of the plain
call), their medians and ratio, and the wall time of each.  The split of the trace call into race_trace_kernel and the
counting kernels comes from a run of this script under
`rocprofv3 --kernel-trace --stats -- python tools/trace_time.py --skip-plain --repeats 1`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ['MCGP_FORCE_GENERIC'] = '1'
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=10_000_000)
    ap.add_argument('--case', default='S60')
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--skip-plain', action='store_true', help='time the trace call only (profiler runs)')
    args = ap.parse_args()
    c = O.load_case(args.case)
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['grid_probs'], c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(seed=args.seed, track_condition=c['track_condition'])

    def trace(n):
        t0 = time.perf_counter()
        res = sim.run_trace(n, *inputs, **kw)
        return time.perf_counter() - t0, kernel_ms(), res

    def plain(n):
        t0 = time.perf_counter()
        sim.run_monte_carlo(n, *inputs, **kw)
        return time.perf_counter() - t0, kernel_ms(), sim.last_histogram

    trace(100_000)                                          # warm-up: code objects, buffers
    if not args.skip_plain:
        plain(100_000)
    t_dev, t_wall, p_dev, p_wall = [], [], [], []
    for _ in range(args.repeats):
        wall, dev, res = trace(args.simulations)
        t_wall.append(round(wall, 4))
        t_dev.append(round(dev, 3))
        if not args.skip_plain:
            wall, dev, hist = plain(args.simulations)
            p_wall.append(round(wall, 4))
            p_dev.append(round(dev, 3))
            assert (hist == res.hist).all(), 'run_trace and run_monte_carlo histograms differ'
    lap1 = max(res.leader_probabilities.items(), key=lambda kv: kv[1][0])
    fl = max(res.fastest_lap_probabilities.items(), key=lambda kv: kv[1])
    out = dict(case=args.case, simulations=args.simulations, trace_device_ms=t_dev, trace_wall_s=t_wall,
               trace_device_ms_median=statistics.median(t_dev), lap1_leader=lap1[0], lap1_leader_p=float(lap1[1][0]),
               fastest_lap=fl[0], fastest_lap_p=fl[1], sc_p=res.event_probabilities['safety_car']['probability'])
    if not args.skip_plain:
        out.update(generic_device_ms=p_dev, generic_wall_s=p_wall, generic_device_ms_median=statistics.median(p_dev),
                   device_ratio=round(statistics.median(t_dev) / statistics.median(p_dev), 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
