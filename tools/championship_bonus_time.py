"""Cost of the fastest-lap bonus (mcgp_run_championship_bonus) on the device.

    python tools/championship_bonus_time.py --parent-lib PATH [--repeats 5] [--simulations 1000000] [--season-simulations 1000000]
    python tools/championship_bonus_time.py --child trace|race_bonus|season_bonus|season_plain [...]     # one measurement

Every measurement is a child process of its own (warm-up of 100 000 simulations, then the timed call; device time of
the whole call from the library's events, mcgp_last_kernel_ms), started one at a time under a time limit; a child that
fails ends the run.  In this order:

  1. The yardstick, first and alone: mcgp_run_trace of the parent commit's library (MCGP_LIB=PATH) on S60, seed 42,
     --simulations simulations, --repeats times.  Its median and max - min spread are printed, and with them the
     expectation, BEFORE anything of this tree is timed: a one-race season with the bonus (race_fastest_kernel, then
     champ_accumulate, champ_bonus and champ_rank) stays within the yardstick's median plus its spread, because the
     kernel stores n + 2 bytes per simulation where the trace stores L n.
  2. This tree's one-race season of S60 with a bonus of 1 within 10, same seed and size, --repeats times.
  3. The whole-season cost, recorded without a bound: the 2024 calendar at --season-simulations per race, the bonus on
     every race, and the parent's mcgp_run_championship at the same size, in turn, --repeats times.

One JSON line at the end.  The split of a call over its kernels comes from runs of their own:
`rocprofv3 --kernel-trace --stats -- python tools/championship_bonus_time.py --child season_bonus`.
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


def child(args):
    import oracle_py as O
    from monte_carlo_gp_amd import RaceConfig, RaceSimulator, cli, run_championship
    from monte_carlo_gp_amd import _native as N
    set_pop = O.load_cases()['set_pop']
    c = O.load_case(args.case)
    if args.child == 'trace':
        sim = RaceSimulator(RaceConfig(**c['config']), set_pop=set_pop)
        inputs = (c['grid_probs'], c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
        call = lambda m: sim.run_trace(m, *inputs, seed=args.seed, track_condition=c['track_condition'])
        probe = lambda res: [int(x) for x in res.hist[:, 0]]
        size = args.simulations
    elif args.child == 'race_bonus':
        race = dict(config=RaceConfig(**c['config']), grid_probs=c['grid_probs'], base_pace=c['base_pace'],
                    tire_deg=c['tire_deg'], driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'],
                    track_condition=c['track_condition'], seed=args.seed, fastest_lap_points=1, fastest_lap_within=10)
        call = lambda m: run_championship([race], m, set_pop=set_pop, return_race_histograms=True)
        probe = lambda res: [int(x) for x in res.race_histograms[0][:, 0]]
        size = args.simulations
    else:
        races = cli.championship_races(cli.championship_jobs(args.season, args.season_seed))
        if args.child == 'season_bonus':
            for r in races:
                r.update(fastest_lap_points=cli.FASTEST_LAP_POINT, fastest_lap_within=cli.FASTEST_LAP_WITHIN)
        call = lambda m: run_championship(races, m)
        probe = lambda res: max(res.title_probabilities, key=res.title_probabilities.get)
        size = args.season_simulations
    call(100_000)                                           # warm-up: code objects, buffers
    t0 = time.perf_counter()
    res = call(size)
    wall = time.perf_counter() - t0
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    print(json.dumps(dict(mode=args.child, simulations=size, device_ms=round(ms.value, 3), wall_s=round(wall, 4),
                          kernel=N.lib().mcgp_last_kernel_name(0).decode(), probe=probe(res))), flush=True)


def sample(mode, args, lib=None):
    env = dict(os.environ)
    env.pop('MCGP_LIB', None)
    if lib:
        env['MCGP_LIB'] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', mode, '--simulations', str(args.simulations),
           '--season-simulations', str(args.season_simulations), '--season', str(args.season), '--seed', str(args.seed),
           '--season-seed', str(args.season_seed), '--case', args.case]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f'{mode} child failed ({r.returncode}): {r.stderr[-2000:]}')
    s = json.loads(r.stdout.strip().splitlines()[-1])
    print(f'{mode:13} {"(parent lib)" if lib else "(this tree) "} device {s["device_ms"]:10.3f} ms  wall {s["wall_s"]:.3f} s  '
          f'{s["kernel"]}', flush=True)
    return s


def summary(v):
    return dict(ms=v, median_ms=round(statistics.median(v), 3), spread_ms=round(max(v) - min(v), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--simulations', type=int, default=1_000_000)
    ap.add_argument('--season-simulations', type=int, default=1_000_000)
    ap.add_argument('--case', default='S60')
    ap.add_argument('--seed', type=int, default=42)
    ap.add_argument('--season', type=int, default=2024)
    ap.add_argument('--season-seed', type=int, default=7)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent-lib', type=str, default=None, help='libmcgp_hip.so built from the parent commit')
    ap.add_argument('--child', choices=['trace', 'race_bonus', 'season_bonus', 'season_plain'], default=None)
    ap.add_argument('--child-timeout', type=int, default=240)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib:
        raise SystemExit('--parent-lib: the yardstick is the parent commit\'s mcgp_run_trace')
    out = dict(case=args.case, simulations=args.simulations, season_simulations=args.season_simulations, repeats=args.repeats)
    # 1. the yardstick, first and alone
    trace = [sample('trace', args, args.parent_lib) for _ in range(args.repeats)]
    out['parent_trace'] = summary([s['device_ms'] for s in trace])
    bound = round(out['parent_trace']['median_ms'] + out['parent_trace']['spread_ms'], 3)
    print(f'yardstick: parent mcgp_run_trace median {out["parent_trace"]["median_ms"]} ms, spread (max - min) '
          f'{out["parent_trace"]["spread_ms"]} ms\nexpectation, before the new kernel is timed: one-race bonus season median <= '
          f'{bound} ms', flush=True)
    # 2. the new kernel's call
    race = [sample('race_bonus', args) for _ in range(args.repeats)]
    assert all(s['probe'] == trace[0]['probe'] for s in race), 'the race histogram differs from mcgp_run_trace\'s'
    out['race_bonus'] = summary([s['device_ms'] for s in race])
    out['expectation_ms'] = bound
    out['excess_ms'] = round(out['race_bonus']['median_ms'] - out['parent_trace']['median_ms'], 3)
    out['within_expectation'] = bool(out['race_bonus']['median_ms'] <= bound)
    # 3. the whole season, no bound
    bonus, plain = [], []
    for _ in range(args.repeats):
        plain.append(sample('season_plain', args, args.parent_lib)['device_ms'])
        bonus.append(sample('season_bonus', args)['device_ms'])
    out['season_bonus'], out['parent_season_plain'] = summary(bonus), summary(plain)
    out['season_bonus_over_plain'] = round(out['season_bonus']['median_ms'] / out['parent_season_plain']['median_ms'], 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
