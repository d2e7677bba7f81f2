"""Cost of a championship run against the races it is made of.

    python tools/championship_time.py [--simulations 10000000] [--season 2024] [--seed 7] [--skip-races]

Runs the season's Grands Prix (cli.championship_jobs: the backtest's inputs and seeds) once through run_championship
and once as separate RaceSimulator.run_monte_carlo calls with the same seeds, after a small warm-up of both, and
prints one JSON line: wall time of each and the device time the library's events give (mcgp_last_kernel_ms: the
whole championship call; the sum over the race calls).  The split of the championship's device time into race
kernels and champ_accumulate / champ_rank comes from a run of this script under
`rocprofv3 --kernel-trace --stats -- python tools/championship_time.py --skip-races`.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monte_carlo_gp_amd import RaceSimulator, cli, run_championship  # noqa: E402
from monte_carlo_gp_amd import _native as N  # noqa: E402


def kernel_ms():
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    return ms.value


def run_races(races, n_sims):
    wall, dev = 0.0, 0.0
    for r in races:
        sim = RaceSimulator(r['config'])
        t0 = time.perf_counter()
        sim.run_monte_carlo(n_sims, r['grid_probs'], r['base_pace'], r['tire_deg'], r['driver_variance'],
                            r['driver_dnf_rates'], seed=r['seed'], track_condition=r['track_condition'])
        wall += time.perf_counter() - t0
        dev += kernel_ms()
    return wall, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=10_000_000)
    ap.add_argument('--season', type=int, default=2024)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--skip-races', action='store_true', help='time the championship call only (profiler runs)')
    args = ap.parse_args()
    races = cli.championship_races(cli.championship_jobs(args.season, args.seed))
    run_championship(races, 100_000)                        # warm-up: code objects, buffers
    if not args.skip_races:
        run_races(races[:2], 100_000)
    t0 = time.perf_counter()
    res = run_championship(races, args.simulations)
    champ_wall = time.perf_counter() - t0
    out = dict(races=len(races), simulations=args.simulations, championship_wall_s=round(champ_wall, 4),
               championship_device_ms=round(kernel_ms(), 3),
               leader=max(res.title_probabilities, key=res.title_probabilities.get))
    if not args.skip_races:
        wall, dev = run_races(races, args.simulations)
        out.update(races_wall_s=round(wall, 4), races_device_ms=round(dev, 3),
                   wall_ratio=round(champ_wall / wall, 4), device_ratio=round(out['championship_device_ms'] / dev, 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
