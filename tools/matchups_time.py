"""Cost of counting head-to-heads and podiums on the device against the plain race.

    python tools/matchups_time.py [--simulations 10000000] [--case S60] [--seed 42] [--repeats 3] [--skip-plain]

Runs the golden case through RaceSimulator.run_matchups (podiums included) and through RaceSimulator.run_monte_carlo
with the same seed, after a small warm-up of both, alternating the two `--repeats` times, and prints one JSON line: the
device time the library's events give for each call (mcgp_last_kernel_ms: the whole matchups call; the race kernel of
the plain call), their medians and ratio, and the wall time of each.  The split of the matchups call into race kernels
and race_matchups comes from a run of this script under
`rocprofv3 --kernel-trace --stats -- python tools/matchups_time.py --skip-plain --repeats 1`.
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
    ap.add_argument('--skip-plain', action='store_true', help='time the matchups call only (profiler runs)')
    args = ap.parse_args()
    c = O.load_case(args.case)
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['grid_probs'], c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(seed=args.seed, track_condition=c['track_condition'])

    def matchups(n):
        t0 = time.perf_counter()
        res = sim.run_matchups(n, *inputs, **kw)
        return time.perf_counter() - t0, kernel_ms(), res

    def plain(n):
        t0 = time.perf_counter()
        sim.run_monte_carlo(n, *inputs, **kw)
        return time.perf_counter() - t0, kernel_ms(), sim.last_histogram

    matchups(100_000)                                       # warm-up: code objects, buffers
    if not args.skip_plain:
        plain(100_000)
    m_dev, m_wall, p_dev, p_wall = [], [], [], []
    for _ in range(args.repeats):
        wall, dev, res = matchups(args.simulations)
        m_wall.append(round(wall, 4))
        m_dev.append(round(dev, 3))
        if not args.skip_plain:
            wall, dev, hist = plain(args.simulations)
            p_wall.append(round(wall, 4))
            p_dev.append(round(dev, 3))
            assert (hist == res.hist).all(), 'run_matchups and run_monte_carlo histograms differ'
    top = res.most_likely_podiums(1)[0]
    out = dict(case=args.case, simulations=args.simulations, matchups_device_ms=m_dev, matchups_wall_s=m_wall,
               matchups_device_ms_median=statistics.median(m_dev), top_podium=list(top[0]), top_podium_p=top[1])
    if not args.skip_plain:
        out.update(plain_device_ms=p_dev, plain_wall_s=p_wall, plain_device_ms_median=statistics.median(p_dev),
                   device_ratio=round(statistics.median(m_dev) / statistics.median(p_dev), 4))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
