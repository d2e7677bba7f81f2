"""Cost of resuming a race from a mid-race state on the device.

    python tools/resume_time.py [--simulations 1000000] [--case S60] [--lap 30] [--states 1] [--seed 42] [--repeats 3]
                                [--skip-full]

Takes the state the CPU oracle traced for simulation 0 of the golden case after `--lap` laps, and times
RaceSimulator.run_from_state from `--states` copies of it against the full race under MCGP_FORCE_GENERIC=1 (the same
generic LDS kernel, grid sampling and lap 1 included) with the same seed, after a small warm-up of both, alternating the
two `--repeats` times.  Prints one JSON line: the device time the library's events give for each call
(mcgp_last_kernel_ms: the whole resume call; the race kernel of the full call), their medians and ratio, and the wall
time of each.  Kernel times alone come from a run of this script under
`rocprofv3 --kernel-trace --stats -- python tools/resume_time.py --repeats 1`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import oracle_py as O  # noqa: E402
import resume_ref as RR  # noqa: E402
from monte_carlo_gp_amd import RaceConfig, RaceSimulator  # noqa: E402
from monte_carlo_gp_amd import _native as N  # noqa: E402


def kernel_ms():
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=1_000_000)
    ap.add_argument('--case', default='S60')
    ap.add_argument('--lap', type=int, default=30)
    ap.add_argument('--states', type=int, default=1)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--skip-full', action='store_true', help='time the resume call only (profiler runs)')
    args = ap.parse_args()
    c = O.load_case(args.case)
    drivers = list(c['grid_probs'])
    ref = RR.traced_run(c, 1, args.seed)
    state = RR.race_state(RR.state_arrays(ref, 0, args.lap), args.lap,
                          RR.drs_disabled_until(c, args.seed, 0, args.lap), drivers)
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(seed=args.seed, track_condition=c['track_condition'])

    def resume(n):
        t0 = time.perf_counter()
        sim.run_from_state(n, [state] * args.states, *inputs, drivers=drivers, **kw)
        return time.perf_counter() - t0, kernel_ms(), sim.last_histogram

    def full(n):
        os.environ['MCGP_FORCE_GENERIC'] = '1'
        try:
            t0 = time.perf_counter()
            sim.run_monte_carlo(n, c['grid_probs'], *inputs, **kw)
            return time.perf_counter() - t0, kernel_ms()
        finally:
            del os.environ['MCGP_FORCE_GENERIC']

    resume(100_000)                                         # warm-up: code objects, buffers
    if not args.skip_full:
        full(100_000)
    r_dev, r_wall, f_dev, f_wall = [], [], [], []
    for _ in range(args.repeats):
        wall, dev, hist = resume(args.simulations)
        r_wall.append(round(wall, 4))
        r_dev.append(round(dev, 3))
        if not args.skip_full:
            wall, dev = full(args.simulations)
            f_wall.append(round(wall, 4))
            f_dev.append(round(dev, 3))
    h = hist[0]
    out = dict(case=args.case, lap=args.lap, states=args.states, simulations=args.simulations, resume_device_ms=r_dev,
               resume_wall_s=r_wall, resume_device_ms_median=statistics.median(r_dev),
               win=drivers[int(h[:, 0].argmax())], win_p=int(h[:, 0].max()) / args.simulations)
    if not args.skip_full:
        out.update(generic_full_device_ms=f_dev, generic_full_wall_s=f_wall,
                   generic_full_device_ms_median=statistics.median(f_dev),
                   device_ratio=round(statistics.median(r_dev) / statistics.median(f_dev), 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
