"""Recorded command-line transcripts: the cases (argv lists run through cli.main with cli.F1Predictor replaced by a stand-in
that returns fixed result objects), the hand-made result objects the CLI tests share, and the runner that turns a case into
{'status', 'stdout', 'stderr', 'json'}.  The records under tests/golden/cli/ come from record(): it is run against the
commit BEFORE a change to cli.py / predictor.py (PYTHONPATH at that tree), so that test_cli_transcripts.py compares the new
code with the old code's own words:

    PYTHONPATH=<tree of the earlier commit> python tests/cli_cases.py tests/golden/cli

Every case runs in a directory of its own that holds state.json, state2.json and fixture.json and writes out.json, so no
path of the machine reaches a transcript."""
import argparse
import contextlib
import io
import json
import os
import re
import sys

import numpy as np

from monte_carlo_gp_amd import (CombinedResult, EventResult, GridResult, PaceResult, PenaltyResult, StrategyResult,
                                WeatherResult)


# ---------------------------------------------------------------- hand-made results: 3 drivers, 2 scenarios, 10 simulations
def _counts():
    hist = np.zeros((2, 3, 3), np.int64)
    hist[0] = [[5, 3, 2], [3, 4, 3], [2, 3, 5]]
    hist[1] = [[7, 2, 1], [2, 5, 3], [1, 3, 6]]
    delta = np.zeros((2, 3, 5), np.int64)
    delta[0, :, 2] = 10
    delta[1, 0] = [1, 3, 5, 1, 0]          # driver A: gains 2 once, 1 three times, same 5, loses 1 once
    delta[1, 1] = [0, 1, 6, 3, 0]
    delta[1, 2] = [0, 2, 7, 1, 0]
    return dict(drivers=['A', 'B', 'C'], n_simulations=10, hist=hist, delta=delta)


def strategy_result(names=('model', 'early')):
    return StrategyResult(names=list(names), **_counts())


def penalty_result(names=('none', 'penalised')):
    """strategy_result's counts, with fates."""
    fate = np.zeros((2, 3, 4), np.int64)
    fate[0, :, 0] = 10
    fate[1] = [[0, 6, 3, 1], [10, 0, 0, 0], [10, 0, 0, 0]]
    return PenaltyResult(names=list(names), fate=fate, **_counts())


def event_result(names=('as drawn', 'sc')):
    """strategy_result's counts, 4 laps, with event counts."""
    events = np.zeros((2, 3, 5), np.int64)
    events[0] = [[9, 1, 0, 0, 0], [6, 3, 1, 0, 0], [10, 0, 0, 0, 0]]
    events[1] = [[10, 0, 0, 0, 0], [0, 8, 2, 0, 0], [5, 5, 0, 0, 0]]
    return EventResult(names=list(names), events=events, **_counts())


def pace_result(names=('as is', 'damage')):
    """strategy_result's counts, 4 laps, with laps carried: A's until-stop offset of the second scenario begins on lap 2."""
    carried = np.zeros((2, 3, 5), np.int64)
    carried[:, :, 0] = 10
    carried[1, 0] = [1, 4, 3, 2, 0]
    return PaceResult(names=list(names), carried=carried, until_from={(names[1], 'A'): 2}, **_counts())


def weather_result(names):
    wrong = np.zeros((2, 3, 5), np.int64)
    wrong[:, :, 0] = 10
    wrong[1, 0] = [1, 4, 3, 2, 0]
    return WeatherResult(names=list(names), wrong_laps=wrong, **_counts())


def grid_result(names):
    c = _counts()
    c['hist'][1] = [[2, 3, 5], [5, 3, 2], [3, 4, 3]]
    c['delta'][1] = [[0, 0, 4, 4, 2], [0, 3, 7, 0, 0], [0, 2, 8, 0, 0]]
    start = np.zeros((2, 3, 3), np.int64)
    start[0] = [[6, 3, 1], [3, 5, 2], [1, 2, 7]]
    start[1] = [[0, 0, 10], [7, 3, 0], [3, 7, 0]]
    gain = np.zeros((2, 3, 5), np.int64)
    gain[0, :, 2] = 10
    gain[1, 0] = [0, 0, 5, 3, 2]
    gain[1, 1] = [0, 2, 8, 0, 0]
    gain[1, 2] = [1, 3, 6, 0, 0]
    return GridResult(names=list(names), start=start, gain=gain, **c)


def combined_result(names=('as drawn', 'sc')):
    """strategy_result's counts, 4 laps, with A's fates, event counts and B's laps carried from lap 2."""
    fate = np.zeros((2, 3, 4), np.int64)
    fate[:, :, 0] = 10
    fate[1, 0] = [0, 7, 2, 1]
    events = np.zeros((2, 3, 5), np.int64)
    events[0] = [[9, 1, 0, 0, 0], [6, 3, 1, 0, 0], [8, 2, 0, 0, 0]]
    events[1] = [[9, 1, 0, 0, 0], [0, 7, 2, 1, 0], [8, 2, 0, 0, 0]]
    carried = np.zeros((2, 3, 5), np.int64)
    carried[:, :, 0] = 10
    carried[1, 1] = [1, 4, 3, 2, 0]
    return CombinedResult(names=list(names), fate=fate, events=events, carried=carried,
                          until_from={(names[1], 'B'): 2}, **_counts())


# ---------------------------------------------------------------- the stand-in predictor
REFUSED_SEED = 13            # --seed 13: the stand-in raises the ValueError a library call would


def _refuse(seed):
    if seed == REFUSED_SEED:
        raise ValueError('the library refused these scenarios')


def _two(names):
    return list(names)[:2]


class StandInPredictor:
    """F1Predictor's nine entry points with the signatures the CLI tests' stand-ins have (predict_grids without a state,
    predict_weather with the model sixth); every result is fixed."""

    def __init__(self, device=0):
        pass

    def predict_strategies(self, season, race, fixture, strategies, state=None, n_simulations=0, seed=None,
                           allow_single_compound=False):
        _refuse(seed)
        return strategy_result(_two(strategies))

    def predict_penalties(self, season, race, fixture, penalties, strategies=None, state=None, n_simulations=0, seed=None,
                          allow_single_compound=False):
        _refuse(seed)
        return penalty_result(_two(penalties))

    def predict_events(self, season, race, fixture, events, strategies=None, state=None, n_simulations=0, seed=None,
                       allow_single_compound=False):
        _refuse(seed)
        return event_result(_two(events))

    def predict_paces(self, season, race, fixture, paces, strategies=None, state=None, n_simulations=0, seed=None,
                      allow_single_compound=False):
        _refuse(seed)
        return pace_result(_two(paces))

    def predict_weather(self, season, race, fixture, changes, strategies=None, model=None, state=None, n_simulations=0,
                        seed=None, allow_single_compound=False):
        _refuse(seed)
        assert model is not None
        return weather_result(_two(changes))

    def predict_grids(self, season, race, fixture, edits, strategies=None, n_simulations=0, seed=None,
                      prediction_point='fp2', allow_single_compound=False):
        _refuse(seed)
        return grid_result(_two(edits))

    def predict_combined(self, season, race, fixture, scenarios, state=None, n_simulations=0, seed=None,
                         allow_single_compound=False):
        _refuse(seed)
        return combined_result(_two(scenarios))

    def predict_weekend(self, season, race, fixture, prediction_point='fp2', n_simulations=0, seed=None, matchups=False,
                        **kw):
        d = list(fixture['drivers'])
        n = len(d)
        win = {x: (n - i) / (n * (n + 1) / 2) for i, x in enumerate(d)}
        res = dict(pole_probabilities=dict(reversed(list(win.items()))), win_probabilities=win,
                   podium_probabilities={x: min(1.0, 3 * p) for x, p in win.items()}, full_distributions={'dropped': 1},
                   weather={'rainfall': bool(fixture.get('weather', {}).get('rainfall'))},
                   prediction_point=prediction_point, confidence='moderate', grid_is_actual=False)
        if matchups:
            res.update(head_to_head={d[0]: {d[1]: 0.6}},
                       teammate_battles=[dict(team='Red Bull Racing Honda', drivers=[d[0], d[1]], probabilities=[0.6, 0.4])],
                       likely_podiums=[dict(podium=d[:3], probability=0.125), dict(podium=d[2::-1], probability=0.0625)])
        if kw.get('trace'):
            res.update(leader_by_lap={x: [win[x], 0.5 * win[x], 0.25 + 0.5 * win[x]] for x in d},
                       expected_laps_led={x: 3 * win[x] for x in d}, fastest_lap_probabilities=win,
                       pit_stop_distribution={x: [0.0, 0.75, 0.25] for x in d}, expected_pit_stops={x: 1.25 for x in d},
                       race_event_probabilities={k: dict(probability=p, expected=2 * p)
                                                 for k, p in (('safety_car', 0.5), ('vsc', 0.25), ('red_flag', 0.03125))})
        res.update(_blocks(d, kw, from_grid=True))
        return res

    def predict_from_state(self, season, race, fixture, states, n_simulations=0, seed=None, **kw):
        d = list(fixture['drivers'])
        out = []
        for k, st in enumerate(states):
            r = {'lap': st.lap, 'win_probabilities': {x: float(i == k) for i, x in enumerate(d)},
                 'podium_probabilities': {x: float(i < 3) for i, x in enumerate(d)}, 'points_probabilities': {},
                 'full_distributions': {'dropped': 1}}
            r.update(_blocks(d, kw, from_grid=False))
            out.append(r)
        return out


def _blocks(d, kw, from_grid):
    """The 'gaps', 'conditions', 'tyres' and 'moves' blocks of predictor.gap_keys and its like, written out by hand."""
    out, d = {}, d[:4]
    if kw.get('gaps'):
        opt = kw['gaps'] if isinstance(kw['gaps'], dict) else {}
        edges = opt.get('edges', [1.0, 5.0, 20.0])
        share = [1.0 / (len(edges) + 2)] * (len(edges) + 2)
        out['gaps'] = dict(
            edges=edges, first_lap=1 if from_grid else 4, winning_margin=[0.0] + share[1:-1] + [2 * share[0]],
            finishing_gap={x: share for x in d},
            within_at_flag={x: {str(e): (j + 1) / (len(edges) + i + 1) for j, e in enumerate(edges)} for i, x in enumerate(d)},
            pairs=[dict(a=a, b=b, a_ahead=0.75, b_ahead=0.125, either_out=0.125,
                        within_by_lap={str(e): [0.5, 0.25 + 0.0625 * j] for j, e in enumerate(edges)})
                   for a, b in opt.get('pairs', ())])
    if kw.get('conditions'):
        out['conditions'] = {}
        for k, name in enumerate(kw['conditions']):
            odds = lambda scale: {x: dict(given=scale / (i + 2) if k == 0 else None, unconditional=scale / (i + 3))
                                  for i, x in enumerate(d)}
            out['conditions'][name] = dict(probability=0.25 if k == 0 else 0.0, standard_error=0.015625 if k == 0 else 0.0,
                                           count=5 if k == 0 else 0, win=odds(1.0), podium=odds(2.0))
    if kw.get('tyres'):
        out['tyres'] = dict(first_lap=1 if from_grid else 4, drivers={
            x: dict(stops=[0.0, 0.5, 0.25, 0.125, 0.125], first_stop_window=[12 + i, 20 + i] if i != 1 else None,
                    strategy=dict(sequence='MEDIUM-HARD', probability=0.5),
                    win_by_stops=[None, 0.25 / (i + 1), 0.125, None, 0.0]) for i, x in enumerate(d)})
    if kw.get('moves'):
        out['moves'] = dict(first_lap=2 if from_grid else 4, drivers={
            x: dict(places_gained=0.5 - 0.25 * i, start_gain=0.125 * i if from_grid else None,
                    passes=dict(made_on_track=3.5, lost_on_track=2.25 + i, gained_in_pits=1.5, lost_in_pits=0.75))
            for i, x in enumerate(d)}, race_passes=dict(expected=21.0, p10=12, p90=31),
            pairs=[dict(a=d[0], b=d[1], per_race=1.5), dict(a=d[1], b=d[0], per_race=0.75)])
    return out


# ---------------------------------------------------------------- the cases
RUN = ['--race', 'Bahrain', '--season', '2024', '--simulations', '10']
OFF = RUN + ['--offline', '--seed', '3']
REFUSED = RUN + ['--offline', '--seed', str(REFUSED_SEED)]
JSON = ['--json', 'out.json']
STATE = ['--state', 'state.json']


def _what_if_cases(given, full, bad):
    """The cases every what-if command has: `given` the smallest valid items, `full` the --driver / --plan run, `bad`
    {case: items} that end with status 2."""
    cases = {'full': OFF + full + JSON, 'likeliest winners': OFF + given + JSON,
             'fixture file': RUN + ['--seed', '3', '--fixture', 'fixture.json'] + given, 'not offline': RUN + given,
             'nothing given': list(OFF), 'refused by the library': REFUSED + given}
    cases.update({name: OFF + items for name, items in bad.items()})
    return cases


CASES = {
    'strategy': {
        'full': OFF + ['--driver', 'A', '--plan', 'early=:15/HARD', '--plan', 'two=SOFT:15/MEDIUM,38/SOFT'] + JSON,
        'window': OFF + ['--driver', 'B', '--window', '18-19/HARD', '--allow-single-compound'] + JSON,
        'state': OFF + ['--driver', 'A', '--plan', 'early=:15/HARD'] + STATE + JSON,
        'fixture file': RUN + ['--fixture', 'fixture.json', '--driver', 'A', '--plan', 'early=:15/HARD'],
        'not offline': RUN + ['--driver', 'A', '--plan', 'early=:15/HARD'],
        'nothing given': OFF + ['--driver', 'A'],
        'bad plan': OFF + ['--driver', 'A', '--plan', 'bad'],
        'bad plan stop': OFF + ['--driver', 'A', '--plan', 'one=:25'],
        'bad plan compound': OFF + ['--driver', 'A', '--plan', 'one=:25/ULTRA'],
        'bad window': OFF + ['--driver', 'A', '--window', '20-18/HARD'],
        'plan twice': OFF + ['--driver', 'A', '--plan', 'one=:25/HARD', '--plan', 'one=:26/HARD'],
        'refused by the library': REFUSED + ['--driver', 'A', '--plan', 'early=:15/HARD'],
    },
    'penalty': dict(_what_if_cases(
        ['--give', 'A:5'], ['--give', 'A:5', '--give', 'B:5:flag', '--driver', 'A', '--plan', 'box=:30/HARD'],
        {'bad give': ['--give', 'A:five'], 'bad give kind': ['--give', 'A:5:grid'], 'bad give lap': ['--give', 'A:5:lap'],
         'plan without driver': ['--give', 'A:5', '--plan', 'x=:30/HARD'],
         'bad plan': ['--give', 'A:5', '--driver', 'A', '--plan', 'x=30/HARD'],
         'plan twice': ['--give', 'A:5', '--driver', 'A', '--plan', 'x=:30/HARD', '--plan', 'x=:31/HARD']}),
        state=OFF + ['--give', 'A:10:lap@3', '--driver', 'A', '--plan', 'box=:30/HARD'] + STATE + JSON),
    'events': dict(_what_if_cases(
        ['--event', 'sc=sc@3'],
        ['--event', 'sc=sc@3', '--event', 'sc=none@4-5', '--event', 'late red=red@50', '--driver', 'A', '--plan', 'sc=:3/HARD'],
        {'bad event': ['--event', 'sc=sc@x'], 'bad event kind': ['--event', 'x=yellow@3'], 'bad event name': ['--event', 'sc@3'],
         'event backwards': ['--event', 'x=sc@5-4'], 'plan without driver': ['--event', 'sc=sc@3', '--plan', 'x=:30/HARD'],
         'bad plan': ['--event', 'sc=sc@3', '--driver', 'A', '--plan', 'x=:30'],
         'plan twice': ['--event', 'sc=sc@3', '--driver', 'A', '--plan', 'x=:30/HARD', '--plan', 'x=:31/HARD']}),
        state=OFF + ['--event', 'as drawn=none@4-57', '--event', 'sc=sc@4'] + STATE + JSON),
    'pace': dict(_what_if_cases(
        ['--offset', 'damage=A:0.6@2+'],
        ['--offset', 'damage=A:0.6@2+', '--offset', 'push=B:-0.15@40-49', '--driver', 'A', '--plan', 'damage=:3/HARD'],
        {'bad offset': ['--offset', 'x=A:0.6@x'], 'bad offset seconds': ['--offset', 'x=A:fast@2+'],
         'offset backwards': ['--offset', 'x=A:0.6@12-11'], 'plan without driver': ['--offset', 'x=A:0.6@2+', '--plan', 'x=:30/HARD'],
         'bad plan': ['--offset', 'x=A:0.6@2+', '--driver', 'A', '--plan', '=:30/HARD'],
         'plan twice': ['--offset', 'x=A:0.6@2+', '--driver', 'A', '--plan', 'x=:30/HARD', '--plan', 'x=:31/HARD']}),
        state=OFF + ['--offset', 'damage=A:0.6@4+', '--driver', 'B'] + STATE + JSON),
    'weather': dict(_what_if_cases(
        ['--change', 'rain=damp@30-45'],
        ['--change', 'rain=damp@30-45', '--change', 'rain=wet@46-50', '--driver', 'A', '--plan', 'rain=:30/INTERMEDIATE',
         '--wrong-tyre', 'dry:INTERMEDIATE=3.5'],
        {'bad change': ['--change', 'x=damp@x'], 'bad change condition': ['--change', 'x=snow@30'],
         'bad change name': ['--change', '=damp@30'], 'change backwards': ['--change', 'x=damp@30-29'],
         'plan without driver': ['--change', 'x=damp@2', '--plan', 'x=:30/HARD'],
         'bad plan': ['--change', 'x=damp@2', '--driver', 'A', '--plan', 'x=Q:30/HARD'],
         'plan twice': ['--change', 'x=damp@2', '--driver', 'A', '--plan', 'x=:30/HARD', '--plan', 'x=:31/HARD'],
         'bad wrong tyre': ['--change', 'x=damp@2', '--wrong-tyre', 'dry:SOFT'],
         'wrong tyre out of range': ['--change', 'x=damp@2', '--wrong-tyre', 'dry:SOFT=99']}),
        state=OFF + ['--change', 'rain=damp@30-45', '--allow-single-compound'] + STATE + JSON),
    'grid': _what_if_cases(
        ['--drop', 'new engine=A:engine'],
        ['--driver', 'A', '--drop', 'new engine=A:engine', '--pit-lane', 'pit lane=A:2.5', '--plan',
         'pit lane=A:HARD@0:30/MEDIUM', '--pin', 'front row=B:1', '--pin', 'front row=A:2'],
        {'bad drop': ['--drop', 'x=A'], 'bad drop places': ['--drop', 'x=A:turbo'], 'bad pin': ['--pin', 'x=A:pole'],
         'bad pit lane': ['--pit-lane', 'x=A:slow'], 'bad plan': ['--drop', 'x=A:3', '--plan', 'x=A:HARD'],
         'bad plan age': ['--drop', 'x=A:3', '--plan', 'x=A:HARD@new:30/MEDIUM'],
         'plan alone': ['--plan', 'x=A::20/HARD'], 'edit twice': ['--drop', 'x=A:3', '--pin', 'x=A:2'],
         'plan twice': ['--drop', 'x=A:5', '--plan', 'x=A::20/HARD', '--plan', 'x=A::21/HARD']}),
    'what-if': dict(_what_if_cases(
        ['--event', 'sc=sc@3'],
        ['--driver', 'A', '--event', 'sc=sc@3', '--plan', 'sc=:3/HARD', '--give', 'sc=A:5', '--offset', 'sc=B:0.4@2+'],
        {'bad event': ['--event', 'x=sc'], 'give without name': ['--give', 'A:5'], 'bad give': ['--give', 'x=A'],
         'bad offset': ['--offset', 'x=A:0.6'], 'plan without driver': ['--plan', 'x=:30/HARD'],
         'window without driver': ['--window', '30-31/M'], 'bad plan': ['--driver', 'A', '--plan', 'x'],
         'bad window': ['--driver', 'A', '--window', '30/M'],
         'plan twice': ['--driver', 'A', '--plan', 'x=:31/HARD', '--plan', 'x=:32/HARD'],
         'window of no scenario': ['--driver', 'A', '--window', 'y=30-31/M', '--give', 'x=A:5'],
         'window over a plan': ['--driver', 'A', '--window', 'x=30-31/M', '--plan', 'x=:31/HARD']}),
        state=OFF + ['--driver', 'C', '--give', 'late=B:10:flag', '--offset', 'late=B:0.4@4+'] + STATE + JSON,
        window=OFF + ['--driver', 'A', '--give', 'sc=A:5', '--event', 'sc=sc@31', '--window', 'sc=30-32/H'] + JSON,
        named=OFF + ['--give', 'as drawn=B:5', '--offset', 'x=Z:0.1@2-3', '--offset', 'x=C:0.1@2+'] + JSON),
    'predict': {
        'plain': ['--race', 'Bahrain', '--offline', '--simulations', '20', '--seed', '1'],
        'every flag': ['--race', 'Bahrain', '--season', '2024', '--offline', '--simulations', '20', '--prediction-point', 'fp3',
                       '--matchups', '--trace', '--gaps', '--gap-edges', '0.8,4,30', '--gap-pair', 'VER:NOR', '--gap-pair',
                       'NOR : VER', '--if', 'VER.wins & NOR.podium', '--if', 'sc>=1', '--tyres', '--moves'] + JSON,
        'default gaps': ['--race', 'Bahrain', '--offline', '--gaps'] + JSON,
        'fixture file': ['--race', 'Bahrain', '--fixture', 'fixture.json', '--simulations', '20'] + JSON,
        'not offline': ['--race', 'Bahrain'],
        'bad gap edges': ['--race', 'Bahrain', '--offline', '--gaps', '--gap-edges', '1,x'],
        'bad gap pair': ['--race', 'Bahrain', '--offline', '--gaps', '--gap-pair', ':NOR'],
        'condition twice': ['--race', 'Bahrain', '--offline', '--if', 'sc>=1', '--if', ' sc>=1'],
    },
    'in-race': {
        'plain': ['--race', 'Bahrain', '--offline', '--simulations', '20', '--seed', '1'] + STATE,
        'every flag': ['--race', 'Bahrain', '--season', '2024', '--offline', '--simulations', '20', '--state', 'state.json',
                       '--state', 'state2.json', '--gaps', '--gap-edges', '0.8,4,30', '--gap-pair', 'VER:NOR', '--if',
                       'VER.wins & NOR.podium', '--if', 'sc>=1', '--tyres', '--moves'] + JSON,
        'one state every flag': ['--race', 'Bahrain', '--offline', '--gaps', '--if', 'sc>=1', '--tyres', '--moves'] + STATE + JSON,
        'fixture file': ['--race', 'Bahrain', '--fixture', 'fixture.json'] + STATE + JSON,
        'not offline': ['--race', 'Bahrain'] + STATE,
        'bad gap pair': ['--race', 'Bahrain', '--offline', '--gaps', '--gap-pair', 'VER'] + STATE,
    },
}


# ---------------------------------------------------------------- running a case
RATE = re.compile(r'\([\d,]+ simulations/s incl\. setup\)')          # a wall-clock rate


def _state(lap, drivers=('A', 'B', 'C')):
    return {'lap': lap, 'drs_disabled_until': 0, 'cars': [
        {'driver': d, 'cumulative_time': 90.0 * lap + i, 'last_lap_time': 90.0, 'tire_compound': 'SOFT', 'tire_age': lap,
         'used_compounds': ['SOFT'], 'retired_lap': 0} for i, d in enumerate(drivers)]}


def run_case(cli, command, argv, workdir) -> dict:
    """cli.main([command] + argv) in `workdir` with the stand-in predictor -> its status (an int, or what SystemExit
    carried), stdout with the rate masked, stderr, and out.json parsed (None where none was written)."""
    files = {'state.json': _state(3), 'state2.json': _state(5),
             'fixture.json': dict(cli.synthetic_fixture(['A', 'B', 'C']), synthetic=False, weather={'rainfall': True})}
    for name, doc in files.items():
        with open(os.path.join(workdir, name), 'w') as f:
            json.dump(doc, f)
    out_json = os.path.join(workdir, 'out.json')
    if os.path.exists(out_json):
        os.remove(out_json)
    stdout, stderr = io.StringIO(), io.StringIO()
    before, real = os.getcwd(), cli.F1Predictor
    os.chdir(workdir)
    cli.F1Predictor = StandInPredictor
    try:
        with contextlib.redirect_stdout(stdout), contextlib.redirect_stderr(stderr):
            try:
                status = cli.main([command] + argv)
            except SystemExit as e:
                status = e.code
    finally:
        cli.F1Predictor = real
        os.chdir(before)
    doc = None
    if os.path.exists(out_json):
        with open(out_json) as f:
            doc = json.load(f)
    return dict(status=status, stdout=RATE.sub('(# simulations/s incl. setup)', stdout.getvalue()), stderr=stderr.getvalue(),
                json=doc)


class _Parser(Exception):
    pass


def parser_shape(cli) -> dict:
    """{subcommand: [every action's option strings, dest, type name, default, nargs, required, choices, metavar, help and
    class name, in the order --help lists them]} of the parser cli.main builds."""
    def caught(self, argv=None):
        raise _Parser(self)
    real = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = caught
    try:
        cli.main([])
    except _Parser as e:
        ap = e.args[0]
    finally:
        argparse.ArgumentParser.parse_args = real
    sub = next(a for a in ap._actions if isinstance(a, argparse._SubParsersAction))
    return {name: [dict(option_strings=list(a.option_strings), dest=a.dest, type=getattr(a.type, '__name__', None),
                        default=a.default, nargs=a.nargs, required=a.required,
                        choices=list(a.choices) if a.choices is not None else None, metavar=a.metavar, help=a.help,
                        action=type(a).__name__) for a in p._actions]
            for name, p in sub.choices.items()}


def golden_path(directory, command):
    return os.path.join(directory, command.replace('-', '_') + '.json')


# The one record written by hand: `strategy` used to let the library's ValueError escape as a traceback and now reports it
# as the other six commands do.
HAND_WRITTEN = {('strategy', 'refused by the library'): dict(
    status=2, stdout='\n' + '=' * 60 + '\nF1 Pit Strategy: 2024 Bahrain, A\nSimulations: 10  seed: 13  data: synthetic fixture\n'
    + '=' * 60 + '\n\n', stderr='error: the library refused these scenarios\n', json=None)}


def record(directory) -> None:
    import tempfile
    from monte_carlo_gp_amd import cli
    os.makedirs(directory, exist_ok=True)
    for command, cases in CASES.items():
        doc = {}
        for name, argv in cases.items():
            if (command, name) in HAND_WRITTEN:
                doc[name] = HAND_WRITTEN[command, name]
                continue
            with tempfile.TemporaryDirectory() as tmp:
                doc[name] = run_case(cli, command, argv, tmp)
        with open(golden_path(directory, command), 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')
    with open(golden_path(directory, 'parser'), 'w') as f:
        json.dump(parser_shape(cli), f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    record(sys.argv[1])
