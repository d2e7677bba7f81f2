"""Cost of the pit-window call (mcgp_run_pit_windows) on the device beside the time gaps (mcgp_run_gaps) without pairs.

    python tools/window_time.py [--simulations 1000000] [--case S60] [--seed 42] [--repeats 5] [--windows 1 20 64]

Runs the golden case through RaceSimulator.run_pit_windows with the default edges, once per --windows count (every
driver at the configured pit loss, then at 11 s, 5 s and no loss, until the count is reached), and through
RaceSimulator.run_gaps with no pairs, with the same seed, after a small warm-up of each, alternating them `--repeats`
times in one process, and prints one JSON line: the device time the library's events give for each call
(mcgp_last_kernel_ms: the whole call, counting kernels included), the medians, each window median's ratio to the gaps
median, the bytes staged per simulation (recorded laps x 5 W against recorded laps x (n + 1)) and the chunks each call
takes.  The histograms of the two calls are compared on the way.  The split of the window call into race_window_kernel
and window_count_rows comes from a run under
`rocprofv3 --kernel-trace --stats -- python tools/window_time.py --repeats 1`; the race kernel's registers, scratch and
LDS from the build's resource report (tools/resources.sh).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import oracle_py as O  # noqa: E402
from monte_carlo_gp_amd import RaceConfig, RaceSimulator  # noqa: E402
from monte_carlo_gp_amd import _native as N  # noqa: E402

OTHER_LOSSES = (11.0, 5.0, 0.0)
WINDOW_STAGE_BYTES, GAPS_STAGE_BYTES = 1024 << 20, 512 << 20         # csrc/mcgp_hip.hip: kWindowStageBytes, kGapsStageBytes


def kernel_ms():
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    return ms.value


def window_set(drivers, pit_loss, count):
    every = [(d, x) for x in (pit_loss,) + OTHER_LOSSES for d in drivers]
    if not 1 <= count <= min(len(every), N.MAX_PIT_WINDOWS):
        raise SystemExit(f'--windows {count}: 1 to {min(len(every), N.MAX_PIT_WINDOWS)} for this case')
    return every[:count]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=1_000_000)
    ap.add_argument('--case', default='S60')
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--windows', type=int, nargs='+', default=[1, 20, 64], help='numbers of windows to time')
    args = ap.parse_args()
    c = O.load_case(args.case)
    drivers = list(c['grid_probs'])
    n, L = len(drivers), int(c['config']['total_laps'])
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=O.load_cases()['set_pop'])
    inputs = (c['grid_probs'], c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    kw = dict(seed=args.seed, track_condition=c['track_condition'])
    sets = {w: window_set(drivers, float(c['config']['pit_loss']), w) for w in args.windows}

    def windows(count, wins):
        res = sim.run_pit_windows(count, *inputs, windows=wins, **kw)
        return kernel_ms(), res

    for wins in sets.values():
        windows(100_000, wins)                              # warm-up: code objects, buffers
    sim.run_gaps(100_000, *inputs, **kw)
    w_dev, g_dev, res, name = {w: [] for w in sets}, [], None, ''
    for _ in range(args.repeats):
        for w, wins in sets.items():
            dev, res = windows(args.simulations, wins)
            w_dev[w].append(round(dev, 3))
            name = N.lib().mcgp_last_kernel_name(0).decode()
        g = sim.run_gaps(args.simulations, *inputs, **kw)
        g_dev.append(round(kernel_ms(), 3))
        assert (g.hist == res.hist).all(), 'run_pit_windows and run_gaps histograms differ'
    med = statistics.median(g_dev)
    chunks = lambda budget, per_sim: -(-args.simulations // max(1, budget // per_sim // 256 * 256))     # (before the round rule)
    print(json.dumps(dict(
        case=args.case, simulations=args.simulations, kernel=name,
        window_device_ms={str(w): v for w, v in w_dev.items()},
        window_device_ms_median={str(w): statistics.median(v) for w, v in w_dev.items()},
        gaps_device_ms=g_dev, gaps_device_ms_median=med,
        ratio_to_gaps={str(w): round(statistics.median(v) / med, 4) for w, v in w_dev.items()},
        staged_bytes_per_simulation=dict({str(w): L * 5 * w for w in sets}, gaps=L * (n + 1)),
        chunks_at_most=dict({str(w): chunks(WINDOW_STAGE_BYTES, L * 5 * w) for w in sets}, gaps=chunks(GAPS_STAGE_BYTES, L * (n + 1))),
        free_stop_last_lap={f'{d} {x:g}': round(float(res.free_stop_probability(i)[-1]), 4)
                            for i, (d, x) in enumerate(res.windows[:3])})))


if __name__ == '__main__':
    main()
