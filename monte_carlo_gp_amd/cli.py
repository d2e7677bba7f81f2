"""Command line: the reference's main.py / backtest.py flags, working offline.

    python -m monte_carlo_gp_amd.cli predict  --race Bahrain --season 2024 --simulations 10000 --seed 42 --offline
    python -m monte_carlo_gp_amd.cli backtest --seasons 2024 --seed 42 --simulations 10000000 [--fixtures DIR]
    python -m monte_carlo_gp_amd.cli export-fixtures --seasons 2024 --out DIR
    python -m monte_carlo_gp_amd.cli championship --season 2024 --from-round 18 --simulations 10000000 --seed 7
    python -m monte_carlo_gp_amd.cli championship --season 2024 --from-round 24 --standings before24.json \
        --state lap40.json --needs NOR --needs VER --simulations 1000000 --seed 7
    python -m monte_carlo_gp_amd.cli in-race --race Bahrain --season 2024 --offline --state lap30.json --simulations 1000000
    python -m monte_carlo_gp_amd.cli strategy --race Bahrain --season 2024 --offline --driver VER --plan one=:25/HARD \
        --plan two=SOFT:15/MEDIUM,38/SOFT --window 15-30/HARD --simulations 1000000 --seed 7
    python -m monte_carlo_gp_amd.cli penalty --race Bahrain --season 2024 --offline --give NOR:5 --give VER:5:flag \
        --driver NOR --plan box=:30/HARD --simulations 1000000 --seed 7
    python -m monte_carlo_gp_amd.cli events --race Bahrain --season 2024 --offline --state lap30.json --event sc=sc@31 \
        --driver NOR --plan sc=:31/HARD --event green=none@31-57
    python -m monte_carlo_gp_amd.cli pace --race Bahrain --season 2024 --offline --driver NOR --offset damage=NOR:0.6@12+ \
        --offset 'box now=NOR:0.6@12+' --plan 'box now=:13/HARD' --offset push=NOR:-0.15@40-49
    python -m monte_carlo_gp_amd.cli what-if --race Bahrain --season 2024 --offline --state lap30.json --driver NOR \
        --event 'sc=sc@31' --plan 'sc=:31/HARD' --give 'sc=NOR:5' --offset 'sc=VER:0.4@31+'
    python -m monte_carlo_gp_amd.cli weather --race Bahrain --season 2024 --offline --driver NOR --change 'rain=damp@30-45' \
        --plan 'rain=:30/INTERMEDIATE,46/MEDIUM' [--state lap29.json] [--wrong-tyre dry:INTERMEDIATE=3.0]
    python -m monte_carlo_gp_amd.cli grid --race Bahrain --season 2024 --offline --driver VER --drop 'new engine=VER:engine' \
        --pit-lane 'pit lane=VER:2.5' --plan 'pit lane=VER:HARD@0:30/MEDIUM' --pin 'front row=NOR:1' --pin 'front row=VER:2'

Flags kept from the reference: --season, --race, --prediction-point, --simulations (main.py:8-16);
--seasons, --seed (backtest.py:9-14).  Unlike the reference, --simulations and --seed reach the
simulator (the reference parses --simulations and drops it, main.py:14-15 vs predictor.py:284).
--offline / --fixture replace the FastF1 sessions with a race fixture (see predictor.py); without
--fixture a synthetic weekend is used (SURVEY.md 8d canonical inputs) and labelled as such.  predict --matchups also
prints the teammate head-to-heads and the most likely podiums (counted on the device) and adds them to --json;
predict --trace prints who leads after lap 1 and at the flag, laps led, fastest lap, pit stops and safety-car odds
(counted lap by lap on the device) and adds them to --json.  predict --gaps [--gap-edges 1,2,5] [--gap-pair VER:NOR]...
(also on in-race) prints the winning margin, each driver's odds of finishing within about 1 s / 5 s / 20 s of the winner
(the nearest edges present) and the named pairs' gaps (time gaps counted on the device) and adds a 'gaps' block to --json.
predict --if TEXT (repeatable, also on in-race) evaluates the condition inside every simulation on the device
(conditions.py: e.g. --if 'VER.wins & NOR.podium' --if 'sc>=1' --if 'LEC.pole'), prints its probability with the leading
win odds given it beside the unconditional ones, and adds a 'conditions' block to --json.  predict --tyres (also on
in-race) prints per driver the odds of 0 / 1 / 2 / 3 / 4+ pit stops, the first-stop window, the most likely compound
sequence and the win odds by stop count (stints counted on the device) and adds a 'tyres' block to --json.  predict
--moves (also on in-race) prints per driver the expected places gained, the expected start gain and the passes made and
lost, the expected on-track passes per race with their 10-90 % range and the five commonest (a, b) pairs (order changes
between lap ends, counted on the device) and adds a 'moves' block to --json.
in-race runs the rest of the race from one or more mid-race state files (RaceState JSON, simulation.py); with several
--state files every state sees the same random futures and the columns compare the scenarios.
championship --state FILE resumes round --from-round from a mid-race state (the other rounds from the grid); --needs DRIVER
(repeatable, with --needs-round K, default --from-round) prints that driver's title odds by finishing position in the
round, with the two strongest rivals' given that finish (counted on the device), and adds 'title_needs' to --json.
strategy compares pit strategies for one driver: `model` (the race model's own stops) first, then each --plan
NAME=START:LAP/COMP,LAP/COMP (START empty: the model's start) and each lap of a --window A-B/COMP sweep, all with common
random numbers, from the grid or from a --state file.
penalty gives time penalties (--give DRIVER:SECONDS[:serve|flag|lap][@LAP]: served at the car's first pit stop from LAP
on or else added at the flag; added at the flag; or lost on LAP) and compares `none`, `penalised` and, for each --plan of
--driver, `penalised + NAME`: win and podium odds and expected position, and for each penalised driver the paired change
against `none` and where its penalty ended up (served in the pits, added at the flag, retired first).
events sets the race's events on chosen laps (--event NAME=KIND@LAP[-LAP], KIND sc | vsc | red | none; several per NAME
make one scenario; a --plan of --driver whose NAME matches joins that scenario) and compares the scenarios with
`as drawn` (no override, no plan), which comes first unless the first --event or --plan names its own baseline by using
that name: win and podium odds and their change against the first scenario, and the expected number of event laps.
pace adds lap-time offsets (--offset NAME=DRIVER:SECONDS@LAP-LAP on a range of laps, NAME=DRIVER:SECONDS@LAP+ from LAP until
the car's next pit stop; negative seconds are faster; several per NAME make one scenario; a --plan of --driver whose NAME
matches joins that scenario) and compares the scenarios with `as is` (no offset, no plan): for --driver the win, podium
and expected-position change against the first scenario and, for an until-stop offset, the distribution of the laps it
was carried.
weather changes the track condition on chosen laps (--change NAME=CONDITION@LAP[-LAP], CONDITION dry | damp | wet; several
per NAME make one scenario; a --plan of --driver whose NAME matches joins that scenario, and a plan without a stop on the
change lap stays out) and compares the scenarios with `as forecast` (no change, no plan): for --driver the win, podium and
expected-position change against the first scenario and the expected laps on the wrong class of tyres.  Cars without a
plan cross over by the model's rule.  --wrong-tyre CONDITION:COMPOUND=SECONDS replaces a cell of the project's default
table of seconds lost per lap.
grid edits the starting grid that every simulation draws (--drop NAME=DRIVER:PLACES, PLACES a number, a reference
penalty name such as engine, or back; --pin NAME=DRIVER:SLOT; --pit-lane NAME=DRIVER[:SECONDS], the seconds lost on lap 1,
by default the project's own assumption; several per NAME make one scenario; a --plan NAME=DRIVER:START[@AGE]:LAP/COMP,...
joins the scenario of that NAME) and compares the scenarios with `forecast grid` (no edit, no plan): for --driver the win,
podium and expected-position change against the first scenario, the expected start slot and the places gained from it.
Under torch.distributed.run the backtest shards RACES over ranks (independent problems, no collective
on the data path; results are gathered once).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np

from . import config as K
from .predictor import F1Predictor, circuit_info
from .validation import brier_score, calibration_analysis, podium_accuracy


def synthetic_fixture(drivers=None) -> dict:
    """Canonical synthetic weekend: Elo 1700 - 20 i, pace 90 + 0.1 i, deg 0.05, empty features."""
    drivers = list(drivers or K.DRIVER_TEAMS)
    return dict(
        drivers=drivers,
        quali_ratings={d: 1700.0 - 20.0 * i for i, d in enumerate(drivers)},
        quali_features={}, race_features={},
        practice=dict(base_pace={d: 90.0 + 0.1 * i for i, d in enumerate(drivers)},
                      tire_deg={d: 0.05 for d in drivers}, tire_compounds=None),
        weather={'rainfall': False},
        synthetic=True,
    )


def _bars(title, probs, top=10):
    print(title)
    print('-' * 40)
    for i, (d, p) in enumerate(sorted(probs.items(), key=lambda kv: kv[1], reverse=True)[:top], 1):
        print(f"{i:2}. {d:4} {p:6.1%} {'#' * int(p * 30)}")


def load_fixture(args):
    """The race fixture of a command: the --fixture file, else the synthetic weekend under --offline, else None after the
    error line (the command then ends with status 2)."""
    if args.fixture:
        with open(args.fixture) as f:
            return json.load(f)
    if args.offline:
        return synthetic_fixture()
    print('error: live FastF1 data is not available in this build; use --offline or --fixture FILE', file=sys.stderr)
    return None


def load_state(path):
    """The RaceState of a --state file (RaceState.to_json)."""
    from .simulation import RaceState
    with open(path) as f:
        return RaceState.from_json(json.load(f))


def cmd_predict(args) -> int:
    fixture = load_fixture(args)
    if fixture is None:
        return 2
    print(f"\n{'=' * 60}\nF1 Race Prediction: {args.season} {args.race}\nPrediction point: {args.prediction_point}")
    print(f"Simulations: {args.simulations}  seed: {args.seed}  data: "
          f"{'synthetic fixture' if fixture.get('synthetic') else args.fixture}\n{'=' * 60}\n")
    t0 = time.perf_counter()
    extra = {'trace': True} if args.trace else {}
    if args.gaps:
        extra['gaps'] = gaps_argument(args)
    if args.conditions:
        extra['conditions'] = conditions_argument(args)
    if args.tyres:
        extra['tyres'] = True
    if args.moves:
        extra['moves'] = True
    res = F1Predictor(device=args.device).predict_weekend(
        args.season, args.race, fixture, prediction_point=args.prediction_point,
        n_simulations=args.simulations, seed=args.seed, matchups=args.matchups, **extra)
    dt = time.perf_counter() - t0
    print(f"Weather: {'Wet' if res['weather'].get('rainfall') else 'Dry'}")
    print(f"Confidence: {res['confidence']}   ({args.simulations / dt:,.0f} simulations/s incl. setup)\n")
    _bars('POLE POSITION PROBABILITIES', res['pole_probabilities'])
    print()
    _bars('RACE WINNER PROBABILITIES', res['win_probabilities'])
    print()
    _bars('PODIUM PROBABILITIES', res['podium_probabilities'])
    if args.matchups:
        print('\nTEAMMATE HEAD-TO-HEAD\n' + '-' * 40)
        for b in res['teammate_battles']:
            (a, c), (pa, pc) = b['drivers'], b['probabilities']
            print(f"{b['team'][:16]:16} {a:4} {pa:6.1%} - {pc:6.1%} {c:4}")
        print('\nMOST LIKELY PODIUMS\n' + '-' * 40)
        for i, row in enumerate(res['likely_podiums'], 1):
            print(f"{i:2}. {' - '.join(f'{d:4}' for d in row['podium'])} {row['probability']:6.2%}")
    if args.trace:
        _print_trace(res)
    if args.gaps:
        _print_gaps(res['gaps'])
    if args.conditions:
        _print_conditions(res['conditions'])
    if args.tyres:
        _print_tyres(res['tyres'])
    if args.moves:
        _print_moves(res['moves'])
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({k: v for k, v in res.items() if k != 'full_distributions'}, f)
    return 0


def _print_trace(res) -> None:
    """predict --trace: the lap-by-lap block of a predict_weekend(trace=True) result."""
    leader = res['leader_by_lap']
    laps = len(next(iter(leader.values()), []))
    print('\nLAP LEADER\n' + '-' * 40)
    for k in sorted({1, laps}):
        top = sorted(leader.items(), key=lambda kv: kv[1][k - 1], reverse=True)[:3]
        print(f"after lap {k:<4} " + '  '.join(f"{d:4} {p[k - 1]:6.1%}" for d, p in top))
    print('\nLAPS LED (expected)\n' + '-' * 40)
    for i, (d, x) in enumerate(sorted(res['expected_laps_led'].items(), key=lambda kv: kv[1], reverse=True)[:5], 1):
        print(f"{i:2}. {d:4} {x:6.1f}")
    print()
    _bars('FASTEST LAP', res['fastest_lap_probabilities'], top=5)
    print('\nPIT STOPS\n' + '-' * 40)
    dist = res['pit_stop_distribution']
    for d in list(dist)[:5]:
        print(f"{d:4} " + '  '.join(f"{j} stop{'s' if j != 1 else ''} {p:5.1%}" for j, p in enumerate(dist[d]) if p > 0))
    print('\nSAFETY CAR\n' + '-' * 40)
    for name, label in (('safety_car', 'safety car'), ('vsc', 'VSC'), ('red_flag', 'red flag')):
        ev = res['race_event_probabilities'][name]
        print(f"{label:10} P(at least one) {ev['probability']:6.1%}   expected {ev['expected']:.2f}")


def gaps_argument(args):
    """predict_weekend's / predict_from_state's gaps argument from --gaps, --gap-edges and --gap-pair: True without the
    two options, else {'edges': [...], 'pairs': [(a, b), ...]}."""
    opt = {}
    if args.gap_edges:
        try:
            opt['edges'] = [float(x) for x in args.gap_edges.split(',')]
        except ValueError:
            raise SystemExit(f'error: --gap-edges {args.gap_edges!r}: comma-separated seconds, e.g. 1,2,5') from None
    pairs = []
    for text in args.gap_pair or []:
        a, sep, b = text.partition(':')
        if not sep or not a.strip() or not b.strip():
            raise SystemExit(f'error: --gap-pair {text!r}: two drivers as A:B, e.g. VER:NOR')
        pairs.append((a.strip(), b.strip()))
    if pairs:
        opt['pairs'] = pairs
    return opt or True


def conditions_argument(args) -> dict:
    """predict_weekend's / predict_from_state's conditions argument from the --if options: {text: text}."""
    out = {}
    for text in args.conditions or []:
        name = text.strip()
        if name in out:
            raise SystemExit(f'error: --if {text!r} given twice')
        out[name] = text
    return out


def _print_conditions(block, label='', top=3) -> None:
    """--if: the block of a result's 'conditions' key (predictor.condition_keys)."""
    print(f"\nCONDITIONS{label}\n" + '-' * 40)
    for name, c in block.items():
        print(f"{name}: {c['probability']:6.1%} +- {c['standard_error']:.1%}  ({c['count']} simulations)")
        if not c['count']:
            print('    never met: no conditional odds')
            continue
        win = c['win']
        for d in sorted(win, key=lambda d: win[d]['given'], reverse=True)[:top]:
            print(f"    {d:4} wins {win[d]['given']:6.1%} if so (overall {win[d]['unconditional']:6.1%})   "
                  f"podium {c['podium'][d]['given']:6.1%} (overall {c['podium'][d]['unconditional']:6.1%})")


GAP_MARKS = (1.0, 5.0, 20.0)         # seconds behind the winner that --gaps reports: the nearest edges present


def _nearest_edges(edges):
    out = []
    for mark in GAP_MARKS:
        e = min(edges, key=lambda x: (abs(x - mark), x))
        if e not in out:
            out.append(e)
    return out


def _print_gaps(g, label='') -> None:
    """--gaps: the block of a result's 'gaps' key (predictor.gap_keys)."""
    edges = g['edges']
    bounds = [0.0] + edges
    print(f"\nWINNING MARGIN{label}\n" + '-' * 40)
    margin = g['winning_margin']
    for b, p in enumerate(margin[:-1]):
        if p > 0:
            hi = f"{edges[b]:g} s" if b < len(edges) else 'more'
            print(f"{bounds[b]:6g} s to {hi:8} {p:6.1%}")
    if margin[-1] > 0:
        print(f"{'fewer than two finish':20} {margin[-1]:6.1%}")
    marks = _nearest_edges(edges)
    print(f"\nWITHIN OF THE WINNER AT THE FLAG{label}\n" + '-' * 40)
    print('      ' + ''.join(f"{f'< {e:g} s':>10}" for e in marks))
    rows = g['within_at_flag']
    for d in sorted(rows, key=lambda d: rows[d][str(marks[-1])], reverse=True)[:10]:
        print(f"{d:4}  " + ''.join(f"{rows[d][str(e)]:10.1%}" for e in marks))
    if g['pairs']:
        print(f"\nPAIR GAPS AT THE FLAG{label}\n" + '-' * 40)
    for pr in g['pairs']:
        close = '  '.join(f"|gap| < {e:g} s {pr['within_by_lap'][str(e)][-1]:6.1%}" for e in marks)
        print(f"{pr['a']:4} ahead {pr['a_ahead']:6.1%}   {pr['b']:4} ahead {pr['b_ahead']:6.1%}   "
              f"either out {pr['either_out']:6.1%}   {close}")


def _print_tyres(t, label='', top=10) -> None:
    """--tyres: the block of a result's 'tyres' key (predictor.tyre_keys)."""
    print(f"\nTYRE STRATEGY{label} (laps {t['first_lap']} on)\n" + '-' * 40)
    print('      ' + ''.join(f"{h:>8}" for h in ('0 stops', '1 stop', '2 stops', '3 stops', '4+')) +
          '   first stop   most likely')
    for d, row in list(t['drivers'].items())[:top]:
        w = row['first_stop_window']
        window = f"laps {w[0]:>3}-{w[1]:<3}" if w else 'none       '
        st = row['strategy']
        print(f"{d:4}  " + ''.join(f"{p:8.1%}" for p in row['stops']) + f"   {window}  {st['sequence']} {st['probability']:6.1%}")
    print(f"\nWIN ODDS BY STOP COUNT{label}\n" + '-' * 40)
    for d, row in list(t['drivers'].items())[:top]:
        cells = [f"{s if s < 4 else '4+'} stop{'' if s == 1 else 's'} {p:6.1%}" for s, p in enumerate(row['win_by_stops'])
                 if p is not None]
        print(f"{d:4}  " + '   '.join(cells))


def _print_moves(mv, label='', top=10) -> None:
    """--moves: the block of a result's 'moves' key (predictor.move_keys)."""
    print(f"\nRACE MOVEMENT{label} (passes on laps {mv['first_lap']} on; order changes between lap ends)\n" + '-' * 40)
    print('      places gained  start gain   made   lost  via pits +/-')
    for d, row in list(mv['drivers'].items())[:top]:
        p = row['passes']
        start = f"{row['start_gain']:+10.2f}" if row['start_gain'] is not None else '         -'
        print(f"{d:4}  {row['places_gained']:+13.2f}  {start}  {p['made_on_track']:5.1f}  {p['lost_on_track']:5.1f}  "
              f"{p['gained_in_pits']:5.1f} / {p['lost_in_pits']:.1f}")
    r = mv['race_passes']
    print(f"on-track passes per race: {r['expected']:.1f} (10-90 %: {r['p10']}-{r['p90']})")
    for pr in mv['pairs']:
        print(f"  {pr['a']:4} on {pr['b']:4} {pr['per_race']:5.2f} per race")


def cmd_in_race(args) -> int:
    fixture = load_fixture(args)
    if fixture is None:
        return 2
    states = [load_state(path) for path in args.state]
    print(f"\n{'=' * 60}\nF1 In-Race Prediction: {args.season} {args.race}")
    print(f"Simulations: {args.simulations}  seed: {args.seed}  data: "
          f"{'synthetic fixture' if fixture.get('synthetic') else args.fixture}")
    for i, (path, st) in enumerate(zip(args.state, states)):
        print(f"State {i + 1}: {path} (after lap {st.lap})")
    print('=' * 60 + '\n')
    extra = {'gaps': gaps_argument(args)} if args.gaps else {}
    if args.conditions:
        extra['conditions'] = conditions_argument(args)
    if args.tyres:
        extra['tyres'] = True
    if args.moves:
        extra['moves'] = True
    res = F1Predictor(device=args.device).predict_from_state(args.season, args.race, fixture, states,
                                                             n_simulations=args.simulations, seed=args.seed, **extra)
    drivers = list(res[0]['win_probabilities'])
    for title, key in (('RACE WINNER PROBABILITIES', 'win_probabilities'), ('PODIUM PROBABILITIES', 'podium_probabilities')):
        print(title)
        print('-' * (6 + 9 * len(res)))
        print('      ' + ''.join(f"{'S' + str(i + 1):>9}" for i in range(len(res))))
        for d in sorted(drivers, key=lambda d: res[0][key][d], reverse=True)[:10]:
            print(f"{d:4}  " + ''.join(f"{r[key][d]:9.1%}" for r in res))
        print()
    if args.gaps:
        for i, r in enumerate(res):
            _print_gaps(r['gaps'], label=f' (S{i + 1})' if len(res) > 1 else '')
        print()
    if args.conditions:
        for i, r in enumerate(res):
            _print_conditions(r['conditions'], label=f' (S{i + 1})' if len(res) > 1 else '')
        print()
    if args.tyres:
        for i, r in enumerate(res):
            _print_tyres(r['tyres'], label=f' (S{i + 1})' if len(res) > 1 else '')
        print()
    if args.moves:
        for i, r in enumerate(res):
            _print_moves(r['moves'], label=f' (S{i + 1})' if len(res) > 1 else '')
        print()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump([dict({k: v for k, v in r.items() if k != 'full_distributions'}, state=path)
                       for r, path in zip(res, args.state)], f)
    return 0


def _compound(text: str) -> str:
    """A compound name, case-insensitive, or its first letter (S, M, H, I, W)."""
    from . import _native as N
    t = text.strip().upper()
    for c in N.COMPOUNDS:
        if t == c or (len(t) == 1 and c[0] == t):
            return c
    raise ValueError(f'unknown compound {text!r}: one of {", ".join(N.COMPOUNDS)} or its first letter')


def parse_plan(text: str, driver: str):
    """--plan NAME=START:LAP/COMP,LAP/COMP -> (NAME, PitPlan); START empty: the model's start; no stops after the
    colon: the car never stops."""
    from .simulation import PitPlan
    name, sep, rest = text.partition('=')
    if not sep or not name.strip():
        raise ValueError(f'--plan {text!r}: expected NAME=START:LAP/COMP,...')
    start, sep, stops_text = rest.partition(':')
    if not sep:
        raise ValueError(f'--plan {text!r}: expected NAME=START:LAP/COMP,... (START may be empty)')
    stops = []
    for item in filter(None, (x.strip() for x in stops_text.split(','))):
        lap, sep, comp = item.partition('/')
        if not sep or not lap.strip().isdigit():
            raise ValueError(f'--plan {text!r}: a stop is LAP/COMP, got {item!r}')
        stops.append((int(lap), _compound(comp)))
    return name.strip(), PitPlan(driver, stops, start=_compound(start) if start.strip() else None)


def parse_window(text: str):
    """--window A-B/COMP -> (range(A, B + 1), COMP)."""
    laps, sep, comp = text.partition('/')
    a, dash, b = laps.partition('-')
    if not sep or not dash or not a.strip().isdigit() or not b.strip().isdigit() or int(b) < int(a):
        raise ValueError(f'--window {text!r}: expected A-B/COMP with A <= B')
    return range(int(a), int(b) + 1), _compound(comp)


def strategy_scenarios(driver: str, plans=(), window=None) -> dict:
    """The strategy command's scenarios: 'model' (no plan) first, then each --plan, then the --window sweep."""
    from .simulation import pit_window
    out = {'model': []}
    for text in plans or ():
        name, plan = parse_plan(text, driver)
        if name in out:
            raise ValueError(f'--plan: scenario {name!r} given twice')
        out[name] = [plan]
    if window:
        laps, comp = parse_window(window)
        for name, plans_ in pit_window(driver, laps, comp).items():
            out.setdefault(name, plans_)
    return out


def _strategy_call(args):
    scenarios = strategy_scenarios(args.driver, args.plan, args.window)
    if len(scenarios) < 2:
        raise ValueError('give at least one --plan or --window to compare with the model')
    return (scenarios,)


def _strategy_table(args, kind, call, res) -> dict:
    d = args.driver
    rows = []
    print(f"{'scenario':16} {'win':>7} {'podium':>7} {'E[pts]':>7} {'E[pos]':>7} {'P(better)':>10}  gain +- SE")
    print('-' * 78)
    for name in res.names:
        row = dict(scenario=name, win=res.win_probability(name, d), podium=res.podium_probability(name, d),
                   expected_points=res.expected_points(name)[d], expected_position=res.expected_position(name)[d],
                   **_compared(res, name, d), win_probabilities={x: res.win_probability(name, x) for x in res.drivers})
        rows.append(row)
        print(f"{name[:16]:16} {row['win']:7.1%} {row['podium']:7.1%} {row['expected_points']:7.2f} "
              f"{row['expected_position']:7.2f} {row['p_better']:10.1%}  {row['mean_gain']:+.3f} +- {row['se']:.3f}")
    print(f"\nbest by expected points: {res.best(d)}")
    return {'driver': d, 'n_simulations': res.n_simulations, 'scenarios': rows}


def _compared(res, name, d) -> dict:
    """A driver's paired comparison of scenario `name` with the first scenario, as every what-if row holds it."""
    c = res.compare(name, d)
    return {k: c[k] for k in ('p_better', 'p_same', 'p_worse', 'mean_gain', 'se')}


ROW_KEYS = ('scenario', 'win_probabilities', 'podium_probabilities', 'expected_position', 'drivers')


def _scenario_row(res, name) -> dict:
    """What the JSON row of a scenario holds in every what-if command but `strategy`; 'drivers' is filled per command."""
    return dict(scenario=name, win_probabilities={x: res.win_probability(name, x) for x in res.drivers},
                podium_probabilities={x: res.podium_probability(name, x) for x in res.drivers},
                expected_position=res.expected_position(name), drivers={})


def _print_winners(res, row) -> None:
    lead = sorted(res.drivers, key=lambda x: -row['win_probabilities'][x])[:3]
    print('  most likely winners: ' + ', '.join(f"{x} {row['win_probabilities'][x]:.1%}" for x in lead) + '\n')


def _scenario_table(args, kind, call, res) -> dict:
    """The table and JSON document of events, pace, weather, grid and what-if: per scenario the drivers shown with their
    odds and the change against the first scenario.  The kind may add: 'shown' (args, call, res) -> the drivers to show
    (none: the five likeliest winners); 'scenario' (res, name, call) -> (text behind the scenario's heading, its extra row
    keys); 'driver' (res, name, d, call) -> (the driver's extra keys, the text of its extra columns, lines printed below
    it), with the extra columns' heading in 'columns'; 'row_keys', the order of a row's keys where it is not ROW_KEYS;
    'document' (call) -> extra top-level keys; 'position_change': False leaves the expected-position change out."""
    base = res.names[0]
    shown = kind.get('shown', lambda args, call, res: [args.driver] if args.driver else [])(args, call, res) \
        or sorted(res.drivers, key=lambda x: -res.win_probability(base, x))[:5]
    change = kind.get('position_change', True)
    epos0 = res.expected_position(base)
    rows = []
    for name in res.names:
        head, extra = kind['scenario'](res, name, call) if 'scenario' in kind else ('', {})
        print(f"scenario: {name}{head}")
        print(f"  {'driver':8} {'win':>7} {'change':>8} {'podium':>7} {'change':>8} {'E[pos]':>7} "
              + (f"{'change':>7} " if change else '') + f"{'P(better)':>10}  gain +- SE" + kind.get('columns', ''))
        row = dict(_scenario_row(res, name), **extra)
        for d in shown:
            win, pod, epos = row['win_probabilities'][d], row['podium_probabilities'][d], row['expected_position'][d]
            r = row['drivers'][d] = dict(win=win, win_change=win - res.win_probability(base, d), podium=pod,
                                         podium_change=pod - res.podium_probability(base, d), expected_position=epos)
            if change:
                r['expected_position_change'] = epos - epos0[d]
            r.update(_compared(res, name, d))
            more, columns, lines = kind['driver'](res, name, d, call) if 'driver' in kind else ({}, '', [])
            r.update(more)
            print(f"  {d[:8]:8} {win:7.1%} {r['win_change']:+8.1%} {pod:7.1%} {r['podium_change']:+8.1%} {epos:7.2f} "
                  + (f"{r['expected_position_change']:+7.2f} " if change else '')
                  + f"{r['p_better']:10.1%}  {r['mean_gain']:+.3f} +- {r['se']:.3f}" + columns)
            for line in lines:
                print(line)
            if (name, d) in (getattr(res, 'until_from', None) or {}):       # the laps its until-stop offset was carried
                dist = res.carried_distribution(name, d)
                r['laps_carried'] = [float(x) for x in dist]
                r['expected_laps_carried'] = res.expected_laps_carried(name, d)
                top = sorted(range(len(dist)), key=lambda k: -dist[k])[:5]
                print(f"    offset carried {r['expected_laps_carried']:.2f} laps on average; most likely: "
                      + ', '.join(f'{k} laps {dist[k]:.1%}' for k in sorted(top) if dist[k] > 0))
        _print_winners(res, row)
        rows.append({k: row[k] for k in kind.get('row_keys', ROW_KEYS) if k in row})
    return dict({'baseline': base, 'n_simulations': res.n_simulations},
                **(kind['document'](call) if 'document' in kind else {}), scenarios=rows)


def run_what_if(args) -> int:
    """The seven what-if commands, each a description in WHAT_IFS: 'title', the banner's first line over vars(args);
    'call' (args) -> the predictor's arguments behind the fixture (a ValueError is the user's mistake); 'method', the
    F1Predictor method; 'state': False where the command has no --state; 'table' (args, kind, call, result) -> the JSON
    document, printing the table on its way (default: _scenario_table, whose own entries are listed there)."""
    kind = WHAT_IFS[args.cmd]
    takes_state = kind.get('state', True)
    fixture = load_fixture(args)
    if fixture is None:
        return 2
    state = load_state(args.state) if takes_state and args.state else None
    try:
        call = kind['call'](args)
    except ValueError as e:
        print(f'error: {e}', file=sys.stderr)
        return 2
    print(f"\n{'=' * 60}\n{kind['title'].format(**vars(args))}")
    print(f"Simulations: {args.simulations}  seed: {args.seed}  data: "
          f"{'synthetic fixture' if fixture.get('synthetic') else args.fixture}"
          + (f"  from: {args.state} (after lap {state.lap})" if state else ''))
    print('=' * 60 + '\n')
    try:
        res = getattr(F1Predictor(device=args.device), kind['method'])(
            args.season, args.race, fixture, *call, **({'state': state} if takes_state else {}),
            n_simulations=args.simulations, seed=args.seed, allow_single_compound=args.allow_single_compound)
    except ValueError as e:
        print(f'error: {e}', file=sys.stderr)
        return 2
    doc = kind.get('table', _scenario_table)(args, kind, call, res)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(doc, f)
    return 0


def parse_give(text: str):
    """--give DRIVER:SECONDS[:serve|flag|lap][@LAP] -> TimePenalty (kind 'serve' unless given; 'lap' needs @LAP, 'flag'
    takes none)."""
    from .simulation import TimePenalty
    body, at, lap = text.partition('@')
    parts = [x.strip() for x in body.split(':')]
    if len(parts) not in (2, 3) or not parts[0]:
        raise ValueError(f'--give {text!r}: expected DRIVER:SECONDS[:serve|flag|lap][@LAP]')
    try:
        seconds = float(parts[1])
    except ValueError:
        raise ValueError(f'--give {text!r}: SECONDS must be a number, got {parts[1]!r}') from None
    if not 0 < seconds <= 1e6:
        raise ValueError(f'--give {text!r}: SECONDS must be in (0, 1e6]')
    kind = parts[2].lower() if len(parts) == 3 else 'serve'
    if kind not in ('serve', 'flag', 'lap'):
        raise ValueError(f"--give {text!r}: the kind is 'serve', 'flag' or 'lap', got {parts[2]!r}")
    if at and not lap.strip().isdigit():
        raise ValueError(f'--give {text!r}: @LAP must be a lap number')
    if kind == 'flag' and at:
        raise ValueError(f"--give {text!r}: a 'flag' penalty takes no @LAP")
    if kind == 'lap' and not at:
        raise ValueError(f"--give {text!r}: a 'lap' penalty needs @LAP")
    return TimePenalty(parts[0], seconds, kind, int(lap) if at else None)


def penalty_scenarios(gives, driver=None, plans=()):
    """The penalty command's scenarios -> (penalties, strategies): 'none', 'penalised' (every --give), and for each --plan
    of --driver 'penalised + NAME' (the same penalties with that plan)."""
    given = [parse_give(text) for text in gives or ()]
    if not given:
        raise ValueError('give at least one --give DRIVER:SECONDS[:serve|flag|lap][@LAP]')
    if plans and not driver:
        raise ValueError('--plan needs --driver')
    penalties, strategies = {'none': [], 'penalised': given}, {}
    for text in plans or ():
        name, plan = parse_plan(text, driver)
        name = f'penalised + {name}'
        if name in penalties:
            raise ValueError(f'--plan: scenario {name!r} given twice')
        penalties[name] = list(given)
        strategies[name] = [plan]
    return penalties, strategies


def _penalty_table(args, kind, call, res) -> dict:
    penalised = list(dict.fromkeys(p.driver for p in call[0]['penalised']))
    rows = []
    for name in res.names:
        print(f"scenario: {name}")
        print(f"  {'driver':8} {'win':>7} {'podium':>7} {'E[pos]':>7} {'P(better)':>10} {'P(worse)':>9}  gain +- SE"
              f"       served  at flag  retired")
        row = _scenario_row(res, name)
        for d in penalised:
            f = res.fate_probabilities(name, d)
            r = row['drivers'][d] = dict(win=row['win_probabilities'][d], podium=row['podium_probabilities'][d],
                                         expected_position=row['expected_position'][d], **_compared(res, name, d), fate=f)
            print(f"  {d[:8]:8} {r['win']:7.1%} {r['podium']:7.1%} {r['expected_position']:7.2f} "
                  f"{r['p_better']:10.1%} {r['p_worse']:9.1%}  {r['mean_gain']:+.3f} +- {r['se']:.3f}  "
                  f"{f['served']:7.1%} {f['at_flag']:8.1%} {f['retired']:8.1%}")
        _print_winners(res, row)
        rows.append(row)
    return {'penalised': penalised, 'n_simulations': res.n_simulations, 'scenarios': rows}


EVENT_BASELINE = 'as drawn'


def _parse_word_at_laps(flag: str, word: str, words: tuple, text: str):
    """NAME=WORD@LAP[-LAP], WORD one of `words` in either case -> (NAME, word, first lap, last lap or None); `word` is what
    the flag's usage calls it."""
    name, sep, rest = text.partition('=')
    if not sep or not name.strip():
        raise ValueError(f'{flag} {text!r}: expected NAME={word}@LAP[-LAP]')
    what, at, laps = rest.partition('@')
    what = what.strip().lower()
    if what not in words:
        raise ValueError(f"{flag} {text!r}: {word} is {', '.join(map(repr, words[:-1]))} or {words[-1]!r}, got {what!r}")
    a, dash, b = laps.partition('-')
    if not at or not a.strip().isdigit() or (dash and not b.strip().isdigit()):
        raise ValueError(f'{flag} {text!r}: expected @LAP or @LAP-LAP after the {word.lower()}')
    if dash and int(b) < int(a):
        raise ValueError(f'{flag} {text!r}: the range runs backwards')
    return name.strip(), what, int(a), int(b) if dash else None


def parse_event(text: str):
    """--event NAME=KIND@LAP[-LAP] -> (NAME, RaceEvent)."""
    from .simulation import RaceEvent
    name, kind, lo, hi = _parse_word_at_laps('--event', 'KIND', ('sc', 'vsc', 'red', 'none'), text)
    return name, RaceEvent(kind, lo, hi)


def _named_scenarios(baseline: str, usage: str, parse, items, driver, plans):
    """event_scenarios, weather_scenarios and pace_scenarios -> ({NAME: [item]}, strategies): `baseline` (no item, no plan)
    first, unless the user names a scenario so themselves (then theirs, wherever it stands, is the first); then one
    scenario per NAME, holding every item of that NAME and the --plan of that NAME."""
    if not items:
        raise ValueError(f'give at least one {usage}')
    if plans and not driver:
        raise ValueError('--plan needs --driver')
    out, strategies = {baseline: []}, {}
    for text in items:
        name, item = parse(text)
        out.setdefault(name, []).append(item)
    for text in plans or ():
        name, plan = parse_plan(text, driver)
        if name in strategies:
            raise ValueError(f'--plan: scenario {name!r} given twice')
        out.setdefault(name, [])
        strategies[name] = [plan]
    return out, strategies


def event_scenarios(events, driver=None, plans=()):
    """The events command's scenarios -> (events, strategies): 'as drawn' (no override, no plan) first, unless the user
    names a scenario 'as drawn' themselves (then theirs, wherever it stands, is moved to the front); then one scenario
    per NAME, holding every --event of that NAME and the --plan of that NAME."""
    return _named_scenarios(EVENT_BASELINE, '--event NAME=KIND@LAP[-LAP]', parse_event, events, driver, plans)


def _event_laps(res, name, call=None):
    ee = res.expected_events(name)
    return f"   (laps with: safety car {ee['sc']:.2f}, VSC {ee['vsc']:.2f}, red flag {ee['red']:.2f})", {'expected_events': ee}


WEATHER_BASELINE = 'as forecast'


def parse_change(text: str):
    """--change NAME=CONDITION@LAP[-LAP] -> (NAME, TrackChange)."""
    from .simulation import TrackChange
    name, cond, lo, hi = _parse_word_at_laps('--change', 'CONDITION', ('dry', 'damp', 'wet'), text)
    return name, TrackChange(lo, lo if hi is None else hi, cond)


def parse_wrong_tyre(items):
    """--wrong-tyre CONDITION:COMPOUND=SECONDS ... -> WeatherModel: the project's default table with those cells
    replaced (none given: the default table)."""
    from .simulation import DEFAULT_WRONG_TYRE_SECONDS, WeatherModel
    table = {c: dict(row) for c, row in DEFAULT_WRONG_TYRE_SECONDS.items()}
    for text in items or ():
        usage = f'--wrong-tyre {text!r}: expected CONDITION:COMPOUND=SECONDS'
        cell, sep, seconds = text.partition('=')
        cond, colon, comp = cell.partition(':')
        cond, comp = cond.strip().lower(), comp.strip().upper()
        if not sep or not colon:
            raise ValueError(usage)
        if cond not in table:
            raise ValueError(f"--wrong-tyre {text!r}: CONDITION is 'dry', 'damp' or 'wet', got {cond!r}")
        if comp not in table[cond]:
            raise ValueError(f'--wrong-tyre {text!r}: COMPOUND is one of {list(table[cond])}, got {comp!r}')
        try:
            table[cond][comp] = float(seconds)
        except ValueError:
            raise ValueError(f'--wrong-tyre {text!r}: SECONDS is a number, got {seconds.strip()!r}') from None
    model = WeatherModel(table)
    model.table()                                           # the range of every cell
    return model


def weather_scenarios(changes, driver=None, plans=()):
    """The weather command's scenarios -> (changes, strategies): 'as forecast' (no change, no plan) first, unless the user
    names a scenario 'as forecast' themselves; then one scenario per NAME, holding every --change of that NAME and the
    --plan of that NAME."""
    return _named_scenarios(WEATHER_BASELINE, '--change NAME=CONDITION@LAP[-LAP]', parse_change, changes, driver, plans)


def _wrong_tyre_laps(res, name, d, call):
    wrong = res.expected_wrong_tyre_laps(name, d)
    return dict(expected_wrong_tyre_laps=wrong,
                wrong_tyre_laps=[float(x) for x in res.wrong_tyre_laps_distribution(name, d)]), f"   {wrong:.2f}", []


GRID_BASELINE = 'forecast grid'


def _named_driver(flag, text, usage):
    """NAME=DRIVER[:REST] -> (NAME, DRIVER, REST or None)."""
    name, sep, rest = text.partition('=')
    driver, colon, what = rest.partition(':')
    if not sep or not name.strip() or not driver.strip():
        raise ValueError(f'{flag} {text!r}: expected {usage}')
    return name.strip(), driver.strip(), what.strip() if colon else None


def parse_drop(text: str):
    """--drop NAME=DRIVER:PLACES -> (NAME, GridEdit); PLACES a number of places, a PENALTY_TYPES name or 'back'."""
    from .simulation import GridEdit
    name, driver, places = _named_driver('--drop', text, 'NAME=DRIVER:PLACES')
    if not places:
        raise ValueError(f'--drop {text!r}: expected NAME=DRIVER:PLACES')
    if places.lower() == 'back':
        return name, GridEdit.back(driver)
    if places.isdigit():
        if not 1 <= int(places) <= 255:
            raise ValueError(f'--drop {text!r}: PLACES is in [1, 255]')
        return name, GridEdit.drop(driver, int(places))
    try:
        return name, GridEdit.drop(driver, places.lower())
    except ValueError:
        from .predictor import PENALTY_TYPES
        raise ValueError(f"--drop {text!r}: PLACES is a number, 'back' or one of {sorted(PENALTY_TYPES)}, "
                         f'got {places!r}') from None


def parse_pin(text: str):
    """--pin NAME=DRIVER:SLOT -> (NAME, GridEdit); SLOT is 1-based."""
    from .simulation import GridEdit
    name, driver, slot = _named_driver('--pin', text, 'NAME=DRIVER:SLOT')
    if not slot or not slot.isdigit() or int(slot) < 1:
        raise ValueError(f'--pin {text!r}: SLOT is a grid slot, 1 or more')
    return name, GridEdit.pin(driver, int(slot))


def parse_pit_lane(text: str):
    """--pit-lane NAME=DRIVER[:SECONDS] -> (NAME, GridEdit); SECONDS left out: the project's default."""
    from .simulation import GridEdit
    name, driver, seconds = _named_driver('--pit-lane', text, 'NAME=DRIVER[:SECONDS]')
    if seconds is None:
        return name, GridEdit.pit_lane(driver)
    try:
        sec = float(seconds)
    except ValueError:
        raise ValueError(f'--pit-lane {text!r}: SECONDS is a number, got {seconds!r}') from None
    if not (0.0 <= sec <= 1e6):
        raise ValueError(f'--pit-lane {text!r}: SECONDS is in [0, 1e6]')
    return name, GridEdit.pit_lane(driver, sec)


def parse_grid_plan(text: str):
    """--plan NAME=DRIVER:START[@AGE]:LAP/COMP,LAP/COMP -> (NAME, PitPlan): the strategy command's plan behind the
    driver's name, with the age of the start tyres after '@' (a pit-lane starter's free choice)."""
    usage = 'NAME=DRIVER:START[@AGE]:LAP/COMP,... (START may be empty)'
    name, driver, rest = _named_driver('--plan', text, usage)
    if rest is None or ':' not in rest:
        raise ValueError(f'--plan {text!r}: expected {usage}')
    start, _, stops = rest.partition(':')
    start, at, age = start.partition('@')
    if at and (not start.strip() or not age.strip().isdigit()):
        raise ValueError(f'--plan {text!r}: START@AGE needs a compound and a number of laps')
    _, plan = parse_plan(f'{name}={start}:{stops}', driver)
    if at:
        plan.start_age = int(age)
    return name, plan


def grid_scenarios(drops=(), pins=(), pit_lanes=(), plans=()):
    """The grid command's scenarios -> (edits, strategies): 'forecast grid' (no edit, no plan) first, unless the user names
    a scenario 'forecast grid' themselves; then one scenario per NAME in the order --drop, --pin, --pit-lane, --plan,
    holding every edit of that NAME and the --plan items of that NAME (one per driver)."""
    if not (drops or pins or pit_lanes):
        raise ValueError('give at least one --drop NAME=DRIVER:PLACES, --pin NAME=DRIVER:SLOT or --pit-lane '
                         'NAME=DRIVER[:SECONDS]')
    out, strategies = {GRID_BASELINE: []}, {}
    for flag, parse, items in (('--drop', parse_drop, drops), ('--pin', parse_pin, pins),
                               ('--pit-lane', parse_pit_lane, pit_lanes)):
        for text in items or ():
            name, ed = parse(text)
            if any(e.driver == ed.driver for e in out.get(name, [])):
                raise ValueError(f'{flag} {text!r}: {ed.driver} has an edit in scenario {name!r} already')
            out.setdefault(name, []).append(ed)
    for text in plans or ():
        name, plan = parse_grid_plan(text)
        if any(p.driver == plan.driver for p in strategies.get(name, [])):
            raise ValueError(f'--plan {text!r}: {plan.driver} has a plan in scenario {name!r} already')
        out.setdefault(name, [])
        strategies.setdefault(name, []).append(plan)
    return out, strategies


def _grid_edits(res, name, call):
    return ''.join(f'  [{e}]' for e in call[0].get(name, [])), {'expected_start': res.expected_start(name)}


def _grid_start(res, name, d, call):
    start, gained = res.expected_start(name)[d], res.expected_places_gained(name, d)
    return dict(expected_start=start, expected_places_gained=gained), f"   {start:8.2f}  {gained:+.2f}", []


PACE_BASELINE = 'as is'


def parse_offset(text: str):
    """--offset NAME=DRIVER:SECONDS@LAP-LAP or NAME=DRIVER:SECONDS@LAP+ ('+': until the car's next stop) -> (NAME,
    PaceOffset)."""
    from .simulation import PaceOffset
    usage = f'--offset {text!r}: expected NAME=DRIVER:SECONDS@LAP-LAP or NAME=DRIVER:SECONDS@LAP+'
    name, sep, rest = text.partition('=')
    if not sep or not name.strip():
        raise ValueError(usage)
    what, at, laps = rest.rpartition('@')
    driver, colon, seconds = what.partition(':')
    if not at or not colon or not driver.strip():
        raise ValueError(usage)
    try:
        sec = float(seconds)
    except ValueError:
        raise ValueError(f'--offset {text!r}: SECONDS is a number, got {seconds.strip()!r}') from None
    laps = laps.strip()
    if laps.endswith('+'):
        if not laps[:-1].strip().isdigit():
            raise ValueError(usage)
        return name.strip(), PaceOffset(driver.strip(), sec, until_stop_from=int(laps[:-1]))
    a, dash, b = laps.partition('-')
    if not dash or not a.strip().isdigit() or not b.strip().isdigit():
        raise ValueError(usage)
    if int(b) < int(a):
        raise ValueError(f'--offset {text!r}: the range runs backwards')
    return name.strip(), PaceOffset(driver.strip(), sec, laps=(int(a), int(b)))


def pace_scenarios(offsets, driver=None, plans=()):
    """The pace command's scenarios -> (paces, strategies): 'as is' (no offset, no plan) first, unless the user names a
    scenario 'as is' themselves; then one scenario per NAME, holding every --offset of that NAME and the --plan of that
    NAME."""
    return _named_scenarios(PACE_BASELINE, '--offset NAME=DRIVER:SECONDS@LAP-LAP or NAME=DRIVER:SECONDS@LAP+', parse_offset,
                            offsets, driver, plans)


WHAT_IF_BASELINE = 'as drawn'


def what_if_scenarios(driver=None, plans=(), window=None, gives=(), events=(), offsets=()):
    """The what-if command's scenarios -> {NAME: {'plans', 'penalties', 'events', 'paces'}} for run_combined: 'as drawn'
    (nothing) first, unless the user names a scenario 'as drawn' themselves; then one scenario per NAME in the order the
    names first appear (events, gives, offsets, plans), holding every item given under that NAME.  --give takes the
    penalty command's grammar behind NAME=.  --window [NAME=]A-B/COMP adds one scenario per lap, 'NAME L<lap>' (or
    '<driver> L<lap>'), with the items of NAME and --driver's single stop on that lap."""
    if not (plans or window or gives or events or offsets):
        raise ValueError('give at least one --event, --give, --offset, --plan or --window')
    if (plans or window) and not driver:
        raise ValueError('--plan and --window need --driver')
    out = {WHAT_IF_BASELINE: dict(plans=[], penalties=[], events=[], paces=[])}
    at = lambda name: out.setdefault(name, dict(plans=[], penalties=[], events=[], paces=[]))
    for text in events or ():
        name, ev = parse_event(text)
        at(name)['events'].append(ev)
    for text in gives or ():
        name, sep, rest = text.partition('=')
        if not sep or not name.strip():
            raise ValueError(f'--give {text!r}: expected NAME=DRIVER:SECONDS[:serve|flag|lap][@LAP]')
        at(name.strip())['penalties'].append(parse_give(rest))
    for text in offsets or ():
        name, off = parse_offset(text)
        at(name)['paces'].append(off)
    for text in plans or ():
        name, plan = parse_plan(text, driver)
        if at(name)['plans']:
            raise ValueError(f'--plan: scenario {name!r} given twice')
        out[name]['plans'] = [plan]
    if window:
        from .simulation import PitPlan
        name, sep, rest = window.partition('=')
        of = name.strip() if sep else None
        if sep and of not in out:
            raise ValueError(f'--window {window!r}: no scenario {of!r} to sweep')
        if of is not None and out[of]['plans']:
            raise ValueError(f'--window {window!r}: scenario {of!r} has a --plan already')
        laps, comp = parse_window(rest if sep else window)
        for lap in laps:
            sc = at(f'{of if of is not None else driver} L{lap}')
            if of is not None:
                sc.update({k: list(out[of][k]) for k in ('penalties', 'events', 'paces')})
            sc['plans'] = [PitPlan(driver, [(lap, comp)])]
    return out


def _what_if_shown(args, call, res):
    """--driver, then every driver an item names, in the order given."""
    named = ([args.driver] if args.driver else []) + [x.driver for sc in call[0].values()
                                                      for k in ('penalties', 'paces') for x in sc[k]]
    return list(dict.fromkeys(d for d in named if d in res.drivers))


def _what_if_event_laps(res, name, call):
    return _event_laps(res, name) if call[0].get(name, {}).get('events') else ('', {})


def _what_if_fate(res, name, d, call):
    """The fate of the driver's penalty to serve, if the scenario gives it one."""
    if not any(p.driver == d and p.kind == 'serve' for p in call[0].get(name, {}).get('penalties', ())):
        return {}, '', []
    f = res.fate_probabilities(name, d)
    return {'fate': f}, '', [f"    penalty served at a stop {f['served']:.1%}, added at the flag {f['at_flag']:.1%}, "
                             f"retired unserved {f['retired']:.1%}"]


WHAT_IFS = {
    'strategy': dict(title='F1 Pit Strategy: {season} {race}, {driver}', method='predict_strategies', call=_strategy_call,
                     table=_strategy_table),
    'penalty': dict(title='F1 Time Penalties: {season} {race}', method='predict_penalties', table=_penalty_table,
                    call=lambda args: penalty_scenarios(args.give, args.driver, args.plan)),
    'events': dict(title='F1 Event Scenarios: {season} {race}', method='predict_events',
                   call=lambda args: event_scenarios(args.event, args.driver, args.plan), scenario=_event_laps,
                   position_change=False, row_keys=('scenario', 'expected_events') + ROW_KEYS[1:]),
    'pace': dict(title='F1 Pace Scenarios: {season} {race}', method='predict_paces',
                 call=lambda args: pace_scenarios(args.offset, args.driver, args.plan)),
    'weather': dict(title='F1 Weather Scenarios: {season} {race}', method='predict_weather',
                    call=lambda args: weather_scenarios(args.change, args.driver, args.plan)
                    + (parse_wrong_tyre(args.wrong_tyre),),
                    driver=_wrong_tyre_laps, columns='   wrong-tyre laps',
                    document=lambda call: {'wrong_tyre_seconds': [[float(x) for x in r] for r in call[2].table()]}),
    'grid': dict(title='F1 Grid Scenarios: {season} {race}', method='predict_grids', state=False,
                 call=lambda args: grid_scenarios(args.drop, args.pin, args.pit_lane, args.plan), scenario=_grid_edits,
                 driver=_grid_start, columns='   E[start]  places gained',
                 row_keys=ROW_KEYS[:-1] + ('expected_start', 'drivers')),
    'what-if': dict(title='F1 What-If Scenarios: {season} {race}', method='predict_combined',
                    call=lambda args: (what_if_scenarios(args.driver, args.plan, args.window, args.give, args.event,
                                                         args.offset),),
                    shown=_what_if_shown, scenario=_what_if_event_laps, driver=_what_if_fate,
                    row_keys=('scenario', 'win_probabilities', 'podium_probabilities', 'drivers', 'expected_events',
                              'expected_position')),
}


def load_results(season: int) -> list:
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', f'results_{season}.json')
    with open(path) as f:
        return json.load(f)['races']


def _update_known_pairs(elo, key: str, drivers: list, ranked: list) -> None:
    """The reference's all-pairs Elo update (src/elo.py:45-122: deltas from the ratings BEFORE the event,
    K (actual - expected) / (n - 1) per pair) restricted to the pairs whose outcome the fixture knows:
    every driver in `ranked` beat every driver after it in `ranked` and every driver not in it."""
    n = len(drivers)
    before = {d: elo.ratings[d][key] for d in drivers}
    delta = {d: 0.0 for d in drivers}
    for i, a in enumerate(ranked):
        beaten = ranked[i + 1:] + [d for d in drivers if d not in ranked]
        for b in beaten:
            delta[a] += elo.k * (1.0 - elo.expected_score(before[a], before[b])) / (n - 1)
            delta[b] += elo.k * (0.0 - elo.expected_score(before[b], before[a])) / (n - 1)
    for d in drivers:
        elo.ratings[d][key] = before[d] + delta[d]


def season_fixtures(season: int, entries: list) -> list:
    """One race fixture per race of the season: the synthetic weekend with the Elo quali ratings the
    EARLIER races of that season produced, in calendar order.

    Mirrors the loop of reference validation.py:179-205: predict race k, then update the Elo system with
    race k's outcome before predicting race k+1 (K grows with the race index, reference src/elo.py:13-38).
    The outcome fixture only holds pole, winner and podium, so the update covers the pairs it knows
    (_update_known_pairs): the pole sitter out-qualified everybody; the podium finishers beat everybody
    behind them.  (As written, the reference's own update at validation.py:195-199 passes bare driver codes
    where update_*_ratings expects (driver, value) pairs; the ValueError is swallowed by its `except
    Exception: pass`, so its Elo never moves during a backtest.  This sweep applies the update that loop
    intends.)  Deterministic and cheap (24 x O(n^2) on the host): every rank builds the whole list, then
    races shard over ranks.
    """
    from .elo import F1EloSystem
    base = synthetic_fixture()
    drivers = base['drivers']
    elo = F1EloSystem()
    for d in drivers:
        elo.ratings[d] = {'quali': base['quali_ratings'][d], 'race': base['quali_ratings'][d]}
    out = []
    total = len(entries)
    for idx, entry in enumerate(entries):
        out.append(dict(base, quali_ratings={d: elo.ratings[d]['quali'] for d in drivers},
                        race_ratings={d: elo.ratings[d]['race'] for d in drivers}, race_index=idx))
        elo.set_recency_weight(0, idx, total)
        if entry.get('pole') in elo.ratings:
            _update_known_pairs(elo, 'quali', drivers, [entry['pole']])
        podium = [d for d in entry.get('podium', []) if d in elo.ratings]
        if podium:
            _update_known_pairs(elo, 'race', drivers, podium)
    return out


def fixture_file_name(season: int, index: int, race: str) -> str:
    """File name of a per-race fixture in a --fixtures directory: <season>_<NN>_<race with underscores>.json."""
    return f"{season}_{index + 1:02d}_{race.replace(' ', '_')}.json"


def backtest_jobs(seasons, seed, fixtures_dir=None):
    """(season, result entry, per-race seed, race fixture) for every race of the sweep, in calendar order.

    With fixtures_dir, a race whose file (fixture_file_name) exists there is predicted from THAT fixture -- what the
    reference's per-race practice-session extraction (src/predictor.py:409-569, out of scope) would hand over --
    and the others from the synthetic weekend with the evolved Elo ratings (season_fixtures)."""
    rng = random.Random(seed)
    jobs = []
    for season in seasons:
        entries = load_results(season)
        for idx, (entry, fx) in enumerate(zip(entries, season_fixtures(season, entries))):
            if fixtures_dir:
                path = os.path.join(fixtures_dir, fixture_file_name(season, idx, entry['race']))
                if os.path.exists(path):
                    with open(path) as f:
                        fx = dict(json.load(f), fixture_file=path)
            jobs.append((season, entry, rng.getrandbits(63), fx))
    return jobs


def shard_jobs(jobs, rank, world):
    """Round-robin share of the races for one rank: [(global index, job)]."""
    return [(i, j) for i, j in enumerate(jobs) if i % world == rank]


BATCH_MAX_SIMULATIONS = 1_000_000        # per race: up to here the races of a sweep share one launch


def backtest(seasons, seed=42, n_simulations=10000, device=0, rank=0, world=1, predictor_factory=None,
             fixtures_dir=None):
    """Sweep one prediction per race of each season and score it (reference validation.py:161-209).

    A fresh predictor per race, fed that race's fixture (season_fixtures: Elo evolved over the earlier
    races).  Each race gets its own seed drawn from random.Random(seed) (the reference seeds the global
    streams once and lets them run on, :172-174; per-race seeds keep races independent so they can
    shard over GPUs: rank r takes races r, r + world, ...; no collective on the data path, one
    all_gather_object of the per-race rows at the end).  Returns the reference's result dict plus
    per-race rows.
    """
    mine = shard_jobs(backtest_jobs(seasons, seed, fixtures_dir), rank, world)
    factory = predictor_factory or (lambda: F1Predictor(device=device))
    # At the reference's size (10 000 simulations per race, src/predictor.py:284) a launch is as long as one race of
    # one lane: this rank's races then go to the device in ONE launch (run_monte_carlo_batch; every race's histogram is
    # what its own launch would give).  Above BATCH_MAX_SIMULATIONS a race fills the device by itself.
    batched = {}
    if predictor_factory is None and 0 < n_simulations <= BATCH_MAX_SIMULATIONS and mine:
        from .predictor import pack_result
        from .simulation import run_monte_carlo_batch
        todo = [(i, job) for i, job in mine if job[3].get('drivers')]       # (a weekend without data raises below, as ever)
        inputs = [F1Predictor(device=device).simulator_inputs(fixture, entry['race'])
                  for _, (season, entry, race_seed, fixture) in todo]
        outs = run_monte_carlo_batch([dict(inp, seed=job[2]) for inp, (_, job) in zip(inputs, todo)], n_simulations,
                                     device=device)
        for (i, _), inp, (probs, _) in zip(todo, inputs, outs):
            batched[i] = pack_result(inp['drivers'], inp['grid_probs'], probs, inp['weather'], 'fp2', None)
    rows = []
    for i, (season, entry, race_seed, fixture) in mine:
        res = batched[i] if i in batched else factory().predict_weekend(
            season, entry['race'], fixture, n_simulations=n_simulations, seed=race_seed)
        rows.append((i, dict(race=entry['race'], season=season, laps=circuit_info(entry['race'])['laps'],
                             pole=res['pole_probabilities'], win=res['win_probabilities'],
                             podium_probabilities=res['podium_probabilities'], actual=entry, seed=race_seed,
                             fixture='synthetic' if fixture.get('synthetic') and not fixture.get('fixture_file')
                             else fixture.get('fixture_file', 'given'))))
    from .distributed import wants_process_group
    if wants_process_group(world):
        import torch.distributed as dist
        gathered = [None] * world
        dist.all_gather_object(gathered, rows)
        rows = [r for part in gathered for r in part]
    rows = [r for _, r in sorted(rows, key=lambda t: t[0])]
    preds = [dict(pole_probabilities=r['pole'], win_probabilities=r['win'],
                  podium_probabilities=r['podium_probabilities']) for r in rows]
    acts = [r['actual'] for r in rows]
    return {
        'pole_brier': float(brier_score([p['pole_probabilities'] for p in preds], [a['pole'] for a in acts])),
        'win_brier': float(brier_score([p['win_probabilities'] for p in preds], [a['winner'] for a in acts])),
        'podium_accuracy': podium_accuracy(preds, acts),
        'calibration_curve': calibration_analysis([dict(win_probabilities=r['win']) for r in rows], acts),
        'n_races': len(rows),
        'races': rows,
        # what these scores are NOT: the reference's backtest reads live FastF1 sessions and results; here the weekends
        # are fixtures and the outcomes a hand-entered file, so the numbers are not comparable with a reference run
        'reference_comparable': False,
    }


def cmd_backtest(args) -> int:
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    device = int(os.environ.get('LOCAL_RANK', str(args.device)))
    # Rehearsal on a one-GPU box (tests): MCGP_BENCH_SHARE_GPU=1 puts every rank on GPU 0 and gathers over
    # gloo (RCCL refuses two ranks on one device).  Never set in production launches.
    share = os.environ.get('MCGP_BENCH_SHARE_GPU') == '1'
    if share:
        device = args.device
    from .distributed import wants_process_group
    grouped = wants_process_group(world)
    if grouped:
        from . import _native
        _native.lib()                     # build / load once before any rank touches the GPU
        import torch
        import torch.distributed as dist
        if share:
            dist.init_process_group('gloo')
        else:
            torch.cuda.set_device(device)
            dist.init_process_group('nccl', device_id=torch.device('cuda', device))
    t0 = time.perf_counter()
    res = backtest(args.seasons, args.seed, args.simulations, device, rank, world, fixtures_dir=args.fixtures)
    dt = time.perf_counter() - t0
    if rank == 0:
        given = sum(1 for r in res['races'] if r['fixture'] != 'synthetic')
        print(f"\n{'=' * 60}\nBacktest (offline sweep: {given} race fixture(s) from --fixtures, the rest synthetic weekends with Elo\n"
              f"evolved race by race; hand-entered outcomes -- NOT comparable with the reference's live-data backtest)\n"
              f"Seasons: {args.seasons}   simulations per race: {args.simulations}\n{'=' * 60}\n")
        print(f"Races analyzed: {res['n_races']}   ({res['n_races'] * args.simulations / dt:,.0f} simulations/s overall)\n")
        print('BRIER SCORES (lower = better, 0 = perfect)\n' + '-' * 40)
        print(f"  Pole position: {res['pole_brier']:.4f}\n  Race winner:   {res['win_brier']:.4f}")
        print(f"  (Random baseline: {0.0475:.4f})\n")
        print('PODIUM ACCURACY\n' + '-' * 40 + f"\n  Correct podium picks: {res['podium_accuracy']:.1%}\n")
        cal = res['calibration_curve']
        if cal['prob_pred']:
            print('CALIBRATION (win probability: predicted -> observed)\n' + '-' * 40)
            for pp, pt in zip(cal['prob_pred'], cal['prob_true']):
                print(f"  {pp:6.1%} -> {pt:6.1%}")
            print()
        if args.json:
            with open(args.json, 'w') as f:
                json.dump(res, f)
    if grouped:
        dist.destroy_process_group()
    return 0


def cmd_export_fixtures(args) -> int:
    """One JSON file per race (fixture_file_name): the synthetic weekend with that race's Elo ratings -- a template
    to replace with real practice data (base_pace / tire_deg per driver, features, weather)."""
    os.makedirs(args.out, exist_ok=True)
    n = 0
    for season in args.seasons:
        entries = load_results(season)
        for idx, (entry, fx) in enumerate(zip(entries, season_fixtures(season, entries))):
            with open(os.path.join(args.out, fixture_file_name(season, idx, entry['race'])), 'w') as f:
                json.dump(fx, f, indent=1)
            n += 1
    print(f'{n} race fixtures written to {args.out}')
    return 0


FASTEST_LAP_POINT, FASTEST_LAP_WITHIN = 1, 10              # cli championship --fastest-lap-point


def championship_jobs(season, seed, from_round=1, fixtures_dir=None):
    """The races of a championship run: rounds from_round..end of results_<season>.json, each with backtest_jobs' inputs
    and per-race seed (the same seed gives the same race draws as `backtest`).  The results file does not mark sprint
    weekends, so every round is a Grand Prix (still so with --fastest-lap-point: sprints, which pay no fastest-lap point,
    are not in the file)."""
    jobs = backtest_jobs([season], seed, fixtures_dir)
    if not 1 <= from_round <= len(jobs):
        raise ValueError(f'--from-round must be in [1, {len(jobs)}], got {from_round}')
    return jobs[from_round - 1:]


def championship_races(jobs, device=0):
    """run_championship's race dicts for championship_jobs' rows (inputs from F1Predictor.simulator_inputs)."""
    races = []
    for season, entry, race_seed, fixture in jobs:
        inp = F1Predictor(device=device).simulator_inputs(fixture, entry['race'])
        races.append(dict(config=inp['config'], grid_probs=inp['grid_probs'], base_pace=inp['base_pace'],
                          tire_deg=inp['tire_deg'], driver_variance=inp['driver_variance'],
                          driver_dnf_rates=inp['driver_dnf_rates'], track_condition=inp['track_condition'],
                          seed=race_seed))
    return races


def cmd_championship(args) -> int:
    from .simulation import run_championship
    jobs = championship_jobs(args.season, args.seed, args.from_round, args.fixtures)
    standings = None
    if args.standings:
        with open(args.standings) as f:
            standings = json.load(f)
    races = championship_races(jobs, args.device)
    if args.fastest_lap_point:
        # the 2019-2024 rule: a point for the race's fastest lap, if classified in the top ten
        for race in races:
            race.update(fastest_lap_points=FASTEST_LAP_POINT, fastest_lap_within=FASTEST_LAP_WITHIN)
    live = {}
    state = None
    if args.state:
        # round --from-round is under way: it resumes from the state, in the field's own driver order
        state = load_state(args.state)
        live['drivers'] = [str(d) for d in races[0]['grid_probs']]
        races[0] = {k: v for k, v in races[0].items() if k not in ('grid_probs', 'fastest_lap_points', 'fastest_lap_within')}
        races[0]['state'] = state
    needs_round = args.from_round if args.needs_round is None else args.needs_round
    if args.needs:
        if not args.from_round <= needs_round < args.from_round + len(jobs):
            raise ValueError(f'--needs-round must be in [{args.from_round}, {args.from_round + len(jobs) - 1}], got '
                             f'{needs_round}')
        live['given_race'] = needs_round - args.from_round
    elif args.needs_round is not None:
        raise ValueError('--needs-round goes with --needs DRIVER')
    t0 = time.perf_counter()
    res = run_championship(races, args.simulations, standings=standings, device=args.device,
                           return_race_histograms=True, by_round=args.by_round, **live)
    dt = time.perf_counter() - t0
    for d in args.needs or []:
        if d not in res.drivers:
            raise ValueError(f'--needs {d}: not in the field {res.drivers}')
    partial = args.from_round > 1 and not standings
    what = f'points from round {args.from_round} on' if partial else 'season standings'
    print(f"\n{'=' * 60}\nChampionship {args.season}: rounds {args.from_round}-{args.from_round + len(jobs) - 1} "
          f"({len(jobs)} Grands Prix), {what}\nSimulations: {args.simulations}  seed: {args.seed}   "
          f"({args.simulations * len(jobs) / dt:,.0f} race simulations/s)\n{'=' * 60}\n")
    if state is not None:
        print(f"Round {args.from_round} ({jobs[0][1]['race']}) resumes from {args.state} (after lap {state.lap})\n")
    _bars(f"DRIVERS' TITLE PROBABILITIES ({what})", res.title_probabilities)
    print()
    _bars(f"CONSTRUCTORS' TITLE PROBABILITIES ({what})", res.constructor_title_probabilities)
    print()
    exp = res.expected_points
    print(f'EXPECTED POINTS ({what})\n' + '-' * 40)
    for i, (d, p) in enumerate(sorted(exp.items(), key=lambda kv: kv[1], reverse=True)[:10], 1):
        print(f'{i:2}. {d:4} {p:7.1f}')
    if args.fastest_lap_point:
        print(f'\nFASTEST-LAP POINT ({FASTEST_LAP_POINT} point within the top {FASTEST_LAP_WITHIN}, every round)\n' + '-' * 40)
        print(f"{'':2}  {'':4} {'expected':>8}  {'fastest laps':>12}")
        bonus, laps = res.expected_bonus_points, res.fastest_lap_counts.sum(axis=0)
        order = sorted(range(len(res.drivers)), key=lambda i: (-bonus[res.drivers[i]], res.drivers[i]))
        for k, i in enumerate(order[:10], 1):
            d = res.drivers[i]
            print(f'{k:2}. {d:4} {bonus[d]:8.2f}  {int(laps[i]) / max(res.n_simulations, 1):12.2f}')
    if args.by_round:
        print(f'\nBY ROUND ({what})\n' + '-' * 40)
        print(f"{'round':>5}  {'race':<22} {'decided':>8}  {'in contention':>13}  leaders")
        rows = zip(jobs, res.decided_by_round, res.leader_probabilities_by_round, res.contention_probabilities_by_round)
        for k, ((_, entry, _, _), decided, lead, cont) in enumerate(rows):
            top = sorted(lead.items(), key=lambda kv: kv[1], reverse=True)[:3]
            print(f"{args.from_round + k:>5}  {str(entry['race'])[:22]:<22} {decided * 100:7.1f}%  "
                  f"{sum(1 for v in cont.values() if v > 0.01):>13}  "
                  + '  '.join(f'{d} {v * 100:.1f}%' for d, v in top if v > 0))
    needs = {d: title_needs_table(res, d) for d in args.needs or []}
    for d, rows in needs.items():
        _print_title_needs(d, rows, needs_round, str(jobs[needs_round - args.from_round][1]['race']))
    if args.json:
        n = res.n_simulations
        out = dict(season=args.season, from_round=args.from_round, points_from_round_only=partial,
                   simulations=n, seed=args.seed, drivers=res.drivers, teams=res.teams,
                   title_probabilities=res.title_probabilities, position_probabilities=res.position_probabilities,
                   expected_points=exp, constructor_title_probabilities=res.constructor_title_probabilities,
                   constructor_position_probabilities=res.constructor_position_probabilities,
                   races=[dict(race=entry['race'], seed=race_seed,
                               win_probabilities={d: int(h[i, 0]) / n for i, d in enumerate(res.drivers)})
                          for (_, entry, race_seed, _), h in zip(jobs, res.race_histograms)])
        if args.by_round:
            # one entry per simulated round, in race order (index 0 = round --from-round)
            for key in ('decided_by_round', 'leader_probabilities_by_round', 'contention_probabilities_by_round',
                        'clinch_round_probabilities', 'constructor_decided_by_round',
                        'constructor_leader_probabilities_by_round', 'constructor_contention_probabilities_by_round',
                        'constructor_clinch_round_probabilities'):
                out[key] = getattr(res, key)
        if args.fastest_lap_point:
            out['fastest_lap_point'] = dict(
                points=FASTEST_LAP_POINT, within=FASTEST_LAP_WITHIN, expected_bonus_points=res.expected_bonus_points,
                expected_constructor_bonus_points=res.expected_constructor_bonus_points,
                bonus_probabilities_by_round=res.bonus_probabilities_by_round,
                fastest_lap_probabilities_by_round=[
                    {d: int(row[i]) / max(res.n_simulations, 1) for i, d in enumerate(res.drivers)}
                    for row in res.fastest_lap_counts])
        if state is not None:
            out['state_lap'] = int(state.lap)
        if args.needs:
            out['given_round'] = needs_round
            out['title_needs'] = {d: {str(pos): dict(p_finish=row['p_finish'], title=row['title'])
                                      for pos, row in rows.items()} for d, rows in needs.items()}
        with open(args.json, 'w') as f:
            json.dump(out, f)
    return 0


def title_needs_table(res, driver) -> dict:
    """{position: {'p_finish', 'count', 'title': {driver: P(that driver is champion | `driver` finishes there)}}} for the
    positions `driver` took in the given race of a run_championship(..., given_race=...) result; 'title' lists the
    drivers with a non-zero count, `driver` always."""
    table = res.title_given[res.drivers.index(driver)]
    rows = {}
    for p in np.nonzero(table.sum(axis=1))[0]:
        count = int(table[p].sum())
        title = {e: int(table[p, i]) / count for i, e in enumerate(res.drivers) if table[p, i] or e == driver}
        rows[int(p) + 1] = dict(p_finish=count / max(res.n_simulations, 1), count=count, title=title)
    return rows


def _print_title_needs(driver, rows, round_no, race):
    """One row per finishing position of `driver`: P(position), P(title | position) and the title odds of the two
    strongest rivals given that finish."""
    print(f'\nWHAT {driver} NEEDS (round {round_no}, {race})\n' + '-' * 60)
    print(f"{'finish':>6}  {'P(finish)':>9}  {'P(title | finish)':>17}  rivals' title odds given that finish")
    for pos, row in sorted(rows.items()):
        rivals = sorted(((e, v) for e, v in row['title'].items() if e != driver and v > 0), key=lambda kv: -kv[1])[:2]
        print(f"{'P' + str(pos):>6}  {row['p_finish'] * 100:8.1f}%  {row['title'][driver] * 100:16.1f}%  "
              + '  '.join(f'{e} {v * 100:.1f}%' for e, v in rivals))


def _add_race_arguments(p) -> None:
    p.add_argument('--season', type=int, default=2025)
    p.add_argument('--race', type=str, required=True)


def _add_run_arguments(p, simulations=100000) -> None:
    p.add_argument('--simulations', type=int, default=simulations)
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--offline', action='store_true', help='use the synthetic weekend fixture')
    p.add_argument('--fixture', type=str, default=None, help='race fixture JSON (see predictor.py)')
    p.add_argument('--device', type=int, default=0)
    p.add_argument('--json', type=str, default=None)


def _what_if_parser(sub, name, text):
    """The subparser of a what-if command (WHAT_IFS[name]) with the arguments in front of its own."""
    t = sub.add_parser(name, help=text)
    _add_race_arguments(t)
    t.set_defaults(fn=run_what_if)
    return t


def _add_what_if_arguments(t, state=True, single_compound='run plans that use one dry compound (the two-compound rule is '
                                                          'otherwise enforced)') -> None:
    """The arguments behind a what-if command's own."""
    if state:
        t.add_argument('--state', type=str, default=None, help='race state JSON (RaceState.to_json) to start from')
    t.add_argument('--allow-single-compound', action='store_true', help=single_compound)
    _add_run_arguments(t)


def _add_analysis_arguments(p) -> None:
    """The analysis flags predict and in-race share."""
    p.add_argument('--gaps', action='store_true',
                   help='also count time gaps: winning margin, gap to the winner at the flag, named pairs (and add them '
                        'to --json)')
    p.add_argument('--gap-edges', type=str, default=None,
                   help='with --gaps: the bin edges in seconds, comma-separated and increasing (default: 0.5 ... 120)')
    p.add_argument('--gap-pair', type=str, action='append', default=None,
                   help='with --gaps: a pair of drivers A:B whose gap is counted; repeat for more (at most 64)')
    p.add_argument('--if', dest='conditions', metavar='TEXT', type=str, action='append', default=None,
                   help="a condition evaluated inside every simulation, e.g. 'VER.wins & NOR.podium', 'sc>=1', 'LEC.pole': "
                        'its probability and the odds given it (and in --json); repeat for more (at most 64)')
    p.add_argument('--tyres', action='store_true',
                   help="also count the model's tyre stints: stop-count odds, first-stop window, most likely compound "
                        'sequence and win odds by stop count (and add them to --json)')
    p.add_argument('--moves', action='store_true',
                   help='also count how the field moves: expected places gained, start gain, passes made and lost per '
                        'driver, on-track passes per race and the commonest pairs (and add them to --json)')


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog='monte_carlo_gp_amd', description='F1 race prediction on MI355X')
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('predict', help='predict one race weekend (main.py of the reference)')
    _add_race_arguments(p)
    p.add_argument('--prediction-point', type=str, default='fp2', choices=['fp1', 'fp2', 'fp3', 'quali', 'sprint'])
    _add_run_arguments(p, simulations=10000)
    p.add_argument('--matchups', action='store_true',
                   help='also count teammate head-to-heads and the most likely podiums (and add them to --json)')
    p.add_argument('--trace', action='store_true',
                   help='also count the race lap by lap: leader, laps led, fastest lap, pit stops, safety cars '
                        '(and add them to --json)')
    _add_analysis_arguments(p)
    p.set_defaults(fn=cmd_predict)
    b = sub.add_parser('backtest', help='sweep a season and score it (backtest.py of the reference)')
    b.add_argument('--seasons', type=int, nargs='+', default=[2024])
    b.add_argument('--seed', type=int, default=42)
    b.add_argument('--simulations', type=int, default=10000)
    b.add_argument('--device', type=int, default=0)
    b.add_argument('--json', type=str, default=None)
    b.add_argument('--fixtures', type=str, default=None,
                   help='directory of per-race fixture files (see export-fixtures); races without a file use the synthetic weekend')
    b.set_defaults(fn=cmd_backtest)
    e = sub.add_parser('export-fixtures', help='write the per-race fixtures of the offline sweep as editable JSON files')
    e.add_argument('--seasons', type=int, nargs='+', default=[2024])
    e.add_argument('--out', type=str, required=True)
    e.set_defaults(fn=cmd_export_fixtures)
    c = sub.add_parser('championship', help="drivers' and constructors' title odds over the rest of a season")
    c.add_argument('--season', type=int, default=2024)
    c.add_argument('--from-round', type=int, default=1, help='first round simulated (1-based)')
    c.add_argument('--standings', type=str, default=None,
                   help='JSON {driver: points} or {driver: {"points": p, "finishes": [P1s, P2s, ...]}} before that round')
    c.add_argument('--fixtures', type=str, default=None, help='directory of per-race fixture files (as for backtest)')
    c.add_argument('--simulations', type=int, default=10000)
    c.add_argument('--seed', type=int, default=42)
    c.add_argument('--device', type=int, default=0)
    c.add_argument('--json', type=str, default=None)
    c.add_argument('--by-round', action='store_true',
                   help='also count the standings after every round: P(title decided by then), the likeliest leaders, '
                        'the drivers still in contention (and add the tables to --json)')
    c.add_argument('--fastest-lap-point', action='store_true',
                   help='score the 2019-2024 fastest-lap point: 1 point to the driver who sets the fastest lap of a round, '
                        'if classified in the top ten (every round then runs on the slower lap-time-tracking kernel)')
    c.add_argument('--state', type=str, default=None,
                   help='race state JSON (RaceState.to_json) of round --from-round, which then resumes from it (as in-race '
                        'does) instead of starting from the grid; --standings are those before that round')
    c.add_argument('--needs', metavar='DRIVER', type=str, action='append', default=None,
                   help="title odds by that driver's finishing position in one round: P(finish), P(title | finish) and the "
                        'two strongest rivals given that finish (and in --json); repeat for more drivers')
    c.add_argument('--needs-round', type=int, default=None,
                   help='with --needs: the round (absolute number) whose finishing positions are conditioned on; default '
                        '--from-round')
    c.set_defaults(fn=cmd_championship)
    r = sub.add_parser('in-race', help='win and podium odds from a mid-race state (one column per --state)')
    _add_race_arguments(r)
    r.add_argument('--state', type=str, action='append', required=True,
                   help='race state JSON (RaceState.to_json); repeat for scenarios run with common random numbers')
    _add_run_arguments(r)
    _add_analysis_arguments(r)
    r.set_defaults(fn=cmd_in_race)
    t = _what_if_parser(sub, 'strategy', "compare pit strategies for one driver against the model's own stops")
    t.add_argument('--driver', type=str, required=True)
    t.add_argument('--plan', type=str, action='append', default=[],
                   help='NAME=START:LAP/COMP,LAP/COMP (START empty: the model\'s start); repeat for more scenarios')
    t.add_argument('--window', type=str, default=None, help='A-B/COMP: one single-stop scenario per lap A..B')
    _add_what_if_arguments(t)
    t = _what_if_parser(sub, 'penalty', 'race odds under time penalties, served in the pits or added at the flag')
    t.add_argument('--give', type=str, action='append', default=[],
                   help="DRIVER:SECONDS[:serve|flag|lap][@LAP]: 'serve' (default) is served at the car's first stop from "
                        "LAP on, else added at the flag; 'flag' is added at the flag; 'lap' is lost on LAP; repeat for more")
    t.add_argument('--driver', type=str, default=None, help='the driver whose --plan scenarios are compared')
    t.add_argument('--plan', type=str, action='append', default=[],
                   help="NAME=START:LAP/COMP,LAP/COMP, as the strategy command's: one scenario 'penalised + NAME' each")
    _add_what_if_arguments(t)
    t = _what_if_parser(sub, 'events', 'race odds with a safety car, VSC, red flag or no event on chosen laps')
    t.add_argument('--event', type=str, action='append', default=[],
                   help="NAME=KIND@LAP[-LAP]: in scenario NAME the laps have KIND (sc, vsc, red, none) instead of their "
                        "draw; repeat for more; several of one NAME make one scenario")
    t.add_argument('--driver', type=str, default=None, help='the driver of the --plan scenarios, and the one shown')
    t.add_argument('--plan', type=str, action='append', default=[],
                   help="NAME=START:LAP/COMP,LAP/COMP, as the strategy command's; joins the --event scenario of that NAME")
    _add_what_if_arguments(t)
    t = _what_if_parser(sub, 'pace', "race odds under lap-time offsets on chosen laps or until a car's next stop")
    t.add_argument('--offset', type=str, action='append', default=[],
                   help="NAME=DRIVER:SECONDS@LAP-LAP or NAME=DRIVER:SECONDS@LAP+: in scenario NAME, SECONDS (negative = "
                        "faster) are added to DRIVER's base pace on the laps, or ('+') from LAP until the car's next stop; "
                        "repeat for more; several of one NAME make one scenario")
    t.add_argument('--driver', type=str, default=None, help='the driver of the --plan scenarios, and the one shown')
    t.add_argument('--plan', type=str, action='append', default=[],
                   help="NAME=START:LAP/COMP,LAP/COMP, as the strategy command's; joins the --offset scenario of that NAME")
    _add_what_if_arguments(t)
    t = _what_if_parser(sub, 'weather', 'race odds when the track condition changes on chosen laps')
    t.add_argument('--change', type=str, action='append', default=[],
                   help="NAME=CONDITION@LAP[-LAP]: in scenario NAME the laps have CONDITION (dry, damp, wet) instead of the "
                        "race's; repeat for more; several of one NAME make one scenario")
    t.add_argument('--driver', type=str, default=None, help='the driver of the --plan scenarios, and the one shown')
    t.add_argument('--plan', type=str, action='append', default=[],
                   help="NAME=START:LAP/COMP,LAP/COMP, as the strategy command's; joins the --change scenario of that NAME "
                        "(a plan without stops stays out)")
    t.add_argument('--wrong-tyre', type=str, action='append', default=[],
                   help="CONDITION:COMPOUND=SECONDS: seconds a lap on COMPOUND under CONDITION, replacing that cell of the "
                        "project's default table; repeat for more")
    _add_what_if_arguments(t, single_compound='run plans that use one dry compound (the rule is otherwise enforced where '
                                              'the track stays dry)')
    t = _what_if_parser(sub, 'grid', 'race odds under grid drops, pit-lane starts and pinned grid slots')
    t.add_argument('--drop', type=str, action='append', default=[],
                   help="NAME=DRIVER:PLACES: in scenario NAME the driver drops PLACES on the grid each simulation draws; PLACES "
                        "is a number, back, or a penalty name (engine, full_pu, gearbox, pitlane_start); repeat for more")
    t.add_argument('--pin', type=str, action='append', default=[],
                   help='NAME=DRIVER:SLOT: in scenario NAME the driver starts from SLOT in every simulation')
    t.add_argument('--pit-lane', type=str, action='append', default=[],
                   help="NAME=DRIVER[:SECONDS]: in scenario NAME the driver starts from the pit lane, behind the grid, and loses "
                        "SECONDS on lap 1 (default: the project's assumption)")
    t.add_argument('--driver', type=str, default=None, help='the driver shown (default: the five likeliest winners)')
    t.add_argument('--plan', type=str, action='append', default=[],
                   help="NAME=DRIVER:START[@AGE]:LAP/COMP,LAP/COMP: the strategy command's plan for DRIVER; joins the scenario "
                        "of that NAME")
    _add_what_if_arguments(t, state=False, single_compound='run plans that use one dry compound')
    t = _what_if_parser(sub, 'what-if', 'race odds under scenarios that mix pit plans, time penalties, race events and '
                                        'lap-time offsets')
    t.add_argument('--event', type=str, action='append', default=[],
                   help="NAME=KIND@LAP[-LAP], as the events command's; items of one NAME make one scenario")
    t.add_argument('--give', type=str, action='append', default=[],
                   help="NAME=DRIVER:SECONDS[:serve|flag|lap][@LAP]: the penalty command's grammar behind the scenario's NAME")
    t.add_argument('--offset', type=str, action='append', default=[],
                   help="NAME=DRIVER:SECONDS@LAP-LAP or NAME=DRIVER:SECONDS@LAP+, as the pace command's")
    t.add_argument('--driver', type=str, default=None,
                   help='the driver of the --plan and --window scenarios; shown with every driver an item names')
    t.add_argument('--plan', type=str, action='append', default=[],
                   help="NAME=START:LAP/COMP,LAP/COMP, as the strategy command's; joins the scenario of that NAME")
    t.add_argument('--window', type=str, default=None,
                   help='[NAME=]A-B/COMP: one scenario per lap A..B with the items of NAME and a single stop on that lap')
    _add_what_if_arguments(t)
    args = ap.parse_args(argv)
    return args.fn(args)


if __name__ == '__main__':
    sys.exit(main())
