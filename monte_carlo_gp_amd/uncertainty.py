"""Pace-uncertainty command: how sure are these odds when the pace figures are themselves estimates, and what is a
tenth of pace worth to a driver?

    python -m monte_carlo_gp_amd.uncertainty --race Bahrain --season 2024 --offline \\
        --own 0.15 [--own VER:0.05] --team 0.2 [--team Ferrari:0.3] [--edges=-0.3,-0.1,0,0.1,0.3] \\
        [--driver VER] [--state lap30.json] --simulations N --seed S [--json FILE]

The weekend's race (F1Predictor.predict_weekend, or predict_from_state with --state) also runs through
RaceSimulator.run_priors: every simulation draws a pace error per driver -- an own component (--own, seconds a lap, for
everyone or DRIVER:SIGMA) and one shared by a team (--team, for every team or TEAM:SIGMA) -- and races under it, paired with
the forecast's simulation of the same id.  It prints the win odds and expected points as forecast and under the draws,
and for each --driver the odds by bin of the driver's own drawn error.  There are no default sigmas: nobody has measured
what a practice session's pace error is.

The command is a module of its own, built from cli.py's helpers, because cli.main's parser is pinned by a recorded
fixture."""
import argparse
import json
import sys

from . import cli
from .predictor import F1Predictor


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog='monte_carlo_gp_amd.uncertainty',
                                description='race odds under a pace error drawn per driver and team in every simulation, '
                                            'beside the odds as forecast')
    cli._add_race_arguments(p)
    p.add_argument('--state', type=str, default=None, help='race state JSON (RaceState.to_json) to start from')
    p.add_argument('--own', type=str, action='append', default=None,
                   help="standard deviation of every driver's own pace error in seconds a lap, or DRIVER:SIGMA for one "
                        'driver; repeat for more')
    p.add_argument('--team', type=str, action='append', default=None,
                   help="standard deviation of the pace error a team's drivers share, or TEAM:SIGMA for one team; repeat "
                        'for more')
    p.add_argument('--edges', type=str, default=None,
                   help='the bin edges of the drawn error in seconds a lap, comma-separated and increasing, at most 15 '
                        '(default: -0.3,-0.1,0,0.1,0.3; write --edges=-0.2,0,0.2 when the first is negative)')
    p.add_argument('--driver', type=str, action='append', default=None,
                   help='a driver whose odds by drawn error are shown; repeat for more')
    cli._add_run_arguments(p)
    return p


def sigma_argument(values, flag):
    """--own / --team values -> None (not given), a sigma for all, or {name: sigma}; a bare sigma beside NAME:SIGMA
    values stands for every name that has none of its own ('*')."""
    if not values:
        return None
    out = {}
    for text in values:
        name, sep, num = text.rpartition(':')
        try:
            sigma = float(num)
        except ValueError:
            raise SystemExit(f'error: {flag} {text!r}: SIGMA or NAME:SIGMA, e.g. 0.15 or VER:0.05') from None
        if not (sigma == sigma and 0.0 <= sigma <= 10.0):
            raise SystemExit(f'error: {flag} {text!r}: seconds a lap, in [0, 10]')
        key = name.strip() if sep else '*'
        if not key or key in out:
            raise SystemExit(f'error: {flag} {text!r}: ' + ('given twice' if key else 'a name before the colon'))
        out[key] = sigma
    return out['*'] if list(out) == ['*'] else out


def edges_argument(text):
    if text is None:
        return None
    try:
        edges = [float(x) for x in text.split(',')] if text.strip() else []
    except ValueError:
        raise SystemExit(f'error: --edges {text!r}: comma-separated seconds, e.g. -0.2,0,0.2') from None
    if len(edges) > 15 or any(not (b > a) for a, b in zip(edges, edges[1:])) or any(e != e or abs(e) == float('inf') for e in edges):
        raise SystemExit(f'error: --edges {text!r}: at most 15 finite, strictly increasing values')
    return edges


def argument_of(args, drivers, driver_teams) -> dict:
    """predict_weekend's pace_uncertainty argument from the parsed command line: '*' spread over the drivers or teams
    that have no sigma of their own."""
    own, team = sigma_argument(args.own, '--own'), sigma_argument(args.team, '--team')
    if own is None and team is None:
        raise SystemExit('error: give --own, --team or both (there are no default sigmas)')
    teams = sorted({driver_teams.get(d, 'Unknown') for d in drivers})
    spread = lambda given, names: given if not isinstance(given, dict) or '*' not in given else \
        {n: given.get(n, given['*']) for n in list(names) + [k for k in given if k != '*' and k not in names]}
    out = {}
    if own is not None:
        out['own'] = spread(own, drivers)
    if team is not None:
        out['team'] = spread(team, teams)
    edges = edges_argument(args.edges)
    if edges is not None:
        out['edges'] = edges
    return out


def print_block(block, drivers=None, label='') -> None:
    """The tables of a result's 'pace_uncertainty' block (predictor.pace_uncertainty_keys)."""
    rows = sorted(block['drivers'].items(), key=lambda kv: -kv[1]['forecast']['win'])
    print(f"\nPACE UNCERTAINTY{label}: odds as forecast and under the drawn pace errors ({block['n_simulations']} paired "
          f"simulations)\n" + '-' * 78)
    print(f"{'':5} {'win':>8} {'win drawn':>10} {'podium':>8} {'pod. drawn':>10} {'points':>8} {'pts drawn':>10} "
          f"{'P(better)':>10} {'P(worse)':>9}")
    for d, r in rows:
        f, u, c = r['forecast'], r['uncertain'], r['paired']
        print(f"{d:5} {f['win']:8.1%} {u['win']:10.1%} {f['podium']:8.1%} {u['podium']:10.1%} "
              f"{f['expected_points']:8.2f} {u['expected_points']:10.2f} {c['p_better']:10.1%} {c['p_worse']:9.1%}")
    fmt = lambda v: '-inf' if v is None else f'{v:+g}'
    for d in drivers or []:
        if d not in block['drivers']:
            print(f'\n{d}: not among the drivers')
            continue
        by = block['drivers'][d]['by_draw']
        print(f"\n{d} by its own drawn pace error (seconds a lap; negative = faster than estimated)\n" + '-' * 60)
        print(f"{'error':>18} {'share':>8} {'win':>8} {'expected points':>16}")
        for b, (lo, hi) in enumerate(block['bins']):
            bounds = f"[{fmt(lo)}, {'+inf' if hi is None else fmt(hi)})"
            win, pts = by['win'][b], by['expected_points'][b]
            print(f"{bounds:>18} {by['share'][b]:8.1%} {'-' if win is None else format(win, '.1%'):>8} "
                  f"{'-' if pts is None else format(pts, '.2f'):>16}")


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    sigma_argument(args.own, '--own'), sigma_argument(args.team, '--team'), edges_argument(args.edges)   # before the run
    if not args.own and not args.team:
        raise SystemExit('error: give --own, --team or both (there are no default sigmas)')
    fixture = cli.load_fixture(args)
    if fixture is None:
        return 2
    predictor = F1Predictor(device=args.device)
    inp = predictor.simulator_inputs(fixture, args.race)
    argument = argument_of(args, list(inp['grid_probs']), inp['config'].driver_teams)
    print(f"\n{'=' * 60}\nF1 Pace Uncertainty: {args.season} {args.race}")
    print(f"Simulations: {args.simulations}  seed: {args.seed}  data: "
          f"{'synthetic fixture' if fixture.get('synthetic') else args.fixture}")
    try:
        if args.state:
            state = cli.load_state(args.state)
            print(f"State: {args.state} (after lap {state.lap})")
            res = predictor.predict_from_state(args.season, args.race, fixture, state, n_simulations=args.simulations,
                                               seed=args.seed, pace_uncertainty=argument)
        else:
            res = predictor.predict_weekend(args.season, args.race, fixture, n_simulations=args.simulations, seed=args.seed,
                                            pace_uncertainty=argument)
    except ValueError as e:
        raise SystemExit(f'error: {e}') from None
    print('=' * 60)
    print_block(res['pace_uncertainty'], args.driver)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(dict({k: v for k, v in res.items() if k != 'full_distributions'},
                           **({'state': args.state} if args.state else {})), f)
    return 0


if __name__ == '__main__':
    sys.exit(main())
