"""Pit-window command: if this car stops at the end of this lap, where does it come out, behind whom, and is the stop free?

    python -m monte_carlo_gp_amd.pit_window --race Bahrain --season 2024 --offline \\
        [--state lap30.json] --driver NOR [--driver VER] [--loss 11] [--laps 25-45] \\
        [--gap-edges 0.5,1,2,5] --simulations N --seed S [--json FILE]

The weekend's race (F1Predictor.predict_weekend, or predict_from_state with --state) runs through
RaceSimulator.run_pit_windows: the unmodified simulations, nothing re-simulated -- the race AFTER a stop is the
`strategy` command's question.  windows = drivers x ({the config's pit_loss} + the --loss values), at most 64.  Per
window and shown lap it prints P(free stop), the median rejoin position, the likeliest car ahead at rejoin and P(clear
air) at the edge nearest to the model's dirty_air_threshold, all given that the driver is running.

The command is a module of its own, built from cli.py's helpers, because cli.main's parser is pinned by a recorded
fixture.  The package also exports the strategy helper pit_window(driver, laps, compound) (simulation.pit_window) under
this module's name: importing the module rebinds the package attribute to it, so the module stays callable as that
helper (_Module below)."""
import argparse
import json
import sys
import types

from . import _native as N
from . import cli
from .predictor import F1Predictor
from .simulation import pit_window as _strategy_windows


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog='monte_carlo_gp_amd.pit_window',
                                description='rejoin position, places lost and traffic by lap for a pit stop (nothing is '
                                            're-simulated: see the strategy command for the race after a stop)')
    cli._add_race_arguments(p)
    p.add_argument('--state', type=str, default=None, help='race state JSON (RaceState.to_json) to start from')
    p.add_argument('--driver', type=str, action='append', required=True, help='the driver who stops; repeat for more')
    p.add_argument('--loss', type=float, action='append', default=None,
                   help="a pit loss in seconds to ask about beside the race's own pit_loss (e.g. a stop under a safety "
                        'car); repeat for more')
    p.add_argument('--laps', type=str, default=None, help='the laps shown, FIRST-LAST or one lap (default: every recorded lap)')
    p.add_argument('--gap-edges', type=str, default=None,
                   help='the bin edges of the gaps in seconds, comma-separated and increasing (default: 0.5 ... 120)')
    cli._add_run_arguments(p)
    return p


def windows_argument(args) -> list:
    """[(driver, loss or None: the race's pit_loss)]: the drivers x (pit_loss + the --loss values), driver-major."""
    drivers, losses = [], [None]
    for d in args.driver:
        if d.strip() and d.strip() not in drivers:
            drivers.append(d.strip())
    for x in args.loss or []:
        if not (x == x and 0 <= x < float('inf')):
            raise SystemExit(f'error: --loss {x!r}: seconds, finite and not negative')
        if x not in losses:
            losses.append(x)
    windows = [(d, x) for d in drivers for x in losses]
    if not 1 <= len(windows) <= N.MAX_PIT_WINDOWS:
        raise SystemExit(f'error: {len(drivers)} drivers x {len(losses)} losses = {len(windows)} windows: 1 to '
                         f'{N.MAX_PIT_WINDOWS} can be counted in one run')
    return windows


def laps_argument(text, first_lap, total_laps) -> list:
    """The laps shown: --laps FIRST-LAST (or one lap) cut to the recorded laps; all of them without it."""
    lo, hi = first_lap, total_laps
    if text:
        a, sep, b = text.partition('-')
        try:
            lo, hi = int(a), int(b) if sep else int(a)
        except ValueError:
            raise SystemExit(f'error: --laps {text!r}: FIRST-LAST or one lap, e.g. 25-45') from None
        if lo > hi:
            raise SystemExit(f'error: --laps {text!r}: the first lap is after the last')
    return list(range(max(lo, first_lap), min(hi, total_laps) + 1))


def print_block(block, laps_text=None, label='') -> None:
    """The table of a result's 'pit_window' block (predictor.pit_window_keys)."""
    laps = laps_argument(laps_text, block['first_lap'], block['total_laps'])
    pct = lambda x: '     -' if x is None else f'{x:6.1%}'
    for w in block['windows']:
        print(f"\nPIT WINDOW{label}: {w['driver']} losing {w['loss']:g} s (given that {w['driver']} is running; "
              f"nothing is re-simulated)\n" + '-' * 72)
        print(f"{'lap':>4} {'free stop':>10} {'rejoins P':>10} {'likeliest car ahead':>26} "
              f"{'clear air >= ' + format(block['clear_air_seconds'], 'g') + ' s':>20}")
        for lap in laps:
            k = lap - 1
            ahead, median = w['likeliest_ahead'][k], w['median_rejoin_position'][k]
            who = '-' if ahead is None else f'{ahead[0]} ({ahead[1]:.0%})'
            print(f"{lap:4} {pct(w['free_stop'][k]):>10} {'-' if median is None else median:>10} {who:>26} "
                  f"{pct(w['clear_air'][k]):>20}")
        if not laps:
            print('no recorded lap in the range asked for')
        print(f"laps with P(free stop) >= 50%: {', '.join(str(x) for x in w['open_laps']) or 'none'}")


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    windows = windows_argument(args)
    argument = {'windows': windows}
    if args.gap_edges:
        try:
            argument['edges'] = [float(x) for x in args.gap_edges.split(',')]
        except ValueError:
            raise SystemExit(f'error: --gap-edges {args.gap_edges!r}: comma-separated seconds, e.g. 1,2,5') from None
    laps_argument(args.laps, 1, 1)                                    # (a malformed --laps is reported before the run)
    fixture = cli.load_fixture(args)
    if fixture is None:
        return 2
    print(f"\n{'=' * 60}\nF1 Pit Window: {args.season} {args.race}")
    print(f"Simulations: {args.simulations}  seed: {args.seed}  data: "
          f"{'synthetic fixture' if fixture.get('synthetic') else args.fixture}")
    predictor = F1Predictor(device=args.device)
    if args.state:
        state = cli.load_state(args.state)
        print(f"State: {args.state} (after lap {state.lap})")
        res = predictor.predict_from_state(args.season, args.race, fixture, state, n_simulations=args.simulations,
                                           seed=args.seed, pit_window=argument)
    else:
        res = predictor.predict_weekend(args.season, args.race, fixture, n_simulations=args.simulations, seed=args.seed,
                                        pit_window=argument)
    print('=' * 60)
    print_block(res['pit_window'], args.laps)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(dict({k: v for k, v in res.items() if k != 'full_distributions'},
                           **({'state': args.state} if args.state else {})), f)
    return 0


class _Module(types.ModuleType):
    """This module, callable as the strategy helper whose name it shares in the package (see the module docstring)."""

    def __call__(self, *args, **kwargs):
        return _strategy_windows(*args, **kwargs)


sys.modules[__name__].__class__ = _Module

if __name__ == '__main__':
    sys.exit(main())
