"""Cost of a pit-strategy comparison on the device, and the pairing it gives.

    python tools/strategy_time.py [--simulations 1000000] [--case S60] [--scenarios 8] [--lap 30] [--seed 42]
                                  [--repeats 3]

Runs RaceSimulator.run_strategies on the golden case with `--scenarios` scenarios (the model's own strategy, then a
one-stop pit window onto HARD for the driver with the best base pace, one lap apart), from the grid and from the state
the CPU oracle traced for simulation 0 after `--lap` laps (a window after that lap), after a small warm-up of each,
alternating the two `--repeats` times.  Prints one JSON line: the device time the library's events give for each call
(mcgp_last_kernel_ms: the whole call, race and counting kernels), their medians, the device time per scenario and 10^6
simulations, and, for the first window scenario against the model, the paired standard error of the mean position
gain (from delta) next to the one two independent runs would give (from the two histograms).
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
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, pit_window  # noqa: E402
from monte_carlo_gp_amd import _native as N  # noqa: E402


def kernel_ms():
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=1_000_000)
    ap.add_argument('--case', default='S60')
    ap.add_argument('--scenarios', type=int, default=8)
    ap.add_argument('--lap', type=int, default=30)
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    c = O.load_case(args.case)
    drivers = list(c['grid_probs'])
    focus = min(drivers, key=lambda d: c['base_pace'][d])
    L = c['config']['total_laps']
    ref = RR.traced_run(c, 1, args.seed)
    state = RR.race_state(RR.state_arrays(ref, 0, args.lap), args.lap,
                          RR.drs_disabled_until(c, args.seed, 0, args.lap), drivers)
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    k = args.scenarios - 1
    grid_s = dict({'model': []}, **pit_window(focus, range(12, 12 + k), 'HARD'))
    state_s = dict({'model': []}, **pit_window(focus, range(args.lap + 1, min(L, args.lap + 1 + k)), 'HARD'))
    kw = dict(seed=args.seed, track_condition=c['track_condition'], drivers=drivers, allow_single_compound=True)

    def grid(n):
        t0 = time.perf_counter()
        r = sim.run_strategies(n, grid_s, *inputs, grid_probs=c['grid_probs'], **kw)
        return time.perf_counter() - t0, kernel_ms(), r

    def resume(n):
        t0 = time.perf_counter()
        r = sim.run_strategies(n, state_s, *inputs, state=state, **kw)
        return time.perf_counter() - t0, kernel_ms(), r

    grid(100_000)                                            # warm-up: code objects, buffers
    resume(100_000)
    g_dev, g_wall, s_dev, s_wall = [], [], [], []
    for _ in range(args.repeats):
        wall, dev, rg = grid(args.simulations)
        g_wall.append(round(wall, 4))
        g_dev.append(round(dev, 3))
        wall, dev, rs = resume(args.simulations)
        s_wall.append(round(wall, 4))
        s_dev.append(round(dev, 3))
    per = lambda ms, S: round(ms / S / (args.simulations / 1e6), 3)
    cmp_g = rg.compare(rg.names[1], focus)
    cmp_s = rs.compare(rs.names[1], focus)
    out = dict(case=args.case, simulations=args.simulations, scenarios=len(grid_s), focus=focus,
               grid_device_ms=g_dev, grid_wall_s=g_wall, grid_device_ms_median=statistics.median(g_dev),
               grid_ms_per_scenario_per_1e6=per(statistics.median(g_dev), len(grid_s)),
               state_lap=args.lap, state_scenarios=len(state_s), state_device_ms=s_dev, state_wall_s=s_wall,
               state_device_ms_median=statistics.median(s_dev),
               state_ms_per_scenario_per_1e6=per(statistics.median(s_dev), len(state_s)),
               grid_compare=dict(scenario=rg.names[1], **{k_: round(v, 6) for k_, v in cmp_g.items()}),
               state_compare=dict(scenario=rs.names[1], **{k_: round(v, 6) for k_, v in cmp_s.items()}),
               kernel=N.lib().mcgp_last_kernel_name(0).decode())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
