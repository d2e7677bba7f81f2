"""The `weather` command: flag parsing, scenario assembly, error messages and output with a stand-in predictor."""
import json

import numpy as np
import pytest

from cli_cases import weather_result as _result
from monte_carlo_gp_amd import PitPlan, TrackChange, WeatherModel, cli


def test_change_parsing():
    assert cli.parse_change('rain=damp@30-45') == ('rain', TrackChange(30, 45, 'damp'))
    assert cli.parse_change(' late shower = WET @ 50 ') == ('late shower', TrackChange(50, 50, 'wet'))
    assert cli.parse_change('dries=dry@12-57') == ('dries', TrackChange(12, 57, 'dry'))
    for bad, msg in (('damp@30-45', 'expected NAME=CONDITION'), ('=damp@30', 'expected NAME=CONDITION'),
                     ('x=snow@30', "CONDITION is 'dry', 'damp' or 'wet'"), ('x=damp', 'expected @LAP'),
                     ('x=damp@', 'expected @LAP'), ('x=damp@a', 'expected @LAP'), ('x=damp@30-', 'expected @LAP'),
                     ('x=damp@-30', 'expected @LAP'), ('x=damp@3.5', 'expected @LAP'), ('x=damp@30-29', 'runs backwards')):
        with pytest.raises(ValueError, match=msg):
            cli.parse_change(bad)


def test_wrong_tyre_parsing():
    default = WeatherModel().table()
    assert np.array_equal(cli.parse_wrong_tyre([]).table(), default)
    t = cli.parse_wrong_tyre(['dry:INTERMEDIATE=3.5', ' wet : soft = 20 ']).table()
    assert t[0, 3] == 3.5 and t[2, 0] == 20.0
    t[0, 3], t[2, 0] = default[0, 3], default[2, 0]
    assert np.array_equal(t, default)                       # every other cell is the default's
    for bad, msg in (('dry:INTERMEDIATE', 'expected CONDITION:COMPOUND=SECONDS'), ('INTERMEDIATE=3', 'expected CONDITION'),
                     ('snow:SOFT=3', "CONDITION is 'dry', 'damp' or 'wet'"), ('dry:SLICK=3', 'COMPOUND is one of'),
                     ('dry:SOFT=slow', 'SECONDS is a number'), ('dry:SOFT=61', 'finite and in'),
                     ('dry:SOFT=-1', 'finite and in'), ('dry:SOFT=nan', 'finite and in')):
        with pytest.raises(ValueError, match=msg):
            cli.parse_wrong_tyre([bad])


def test_scenario_assembly():
    changes, plans = cli.weather_scenarios(['rain=damp@30-45', 'storm=wet@30-57', 'rain=wet@46-50'], 'NOR',
                                           ['rain=:30/INTERMEDIATE'])
    assert list(changes) == ['as forecast', 'rain', 'storm'] and changes['as forecast'] == []
    assert changes['rain'] == [TrackChange(30, 45, 'damp'), TrackChange(46, 50, 'wet')]
    assert plans == {'rain': [PitPlan('NOR', [(30, 'INTERMEDIATE')])]}
    # a plan of a new name makes a scenario of its own (a plan without stops stays out); the user's baseline stays first
    changes, plans = cli.weather_scenarios(['as forecast=damp@30', 'x=damp@2-3'], 'NOR', ['out=:'])
    assert list(changes) == ['as forecast', 'x', 'out'] and changes['as forecast'] == [TrackChange(30, 30, 'damp')]
    assert changes['out'] == [] and plans == {'out': [PitPlan('NOR', [])]}
    with pytest.raises(ValueError, match='at least one --change'):
        cli.weather_scenarios([])
    with pytest.raises(ValueError, match='--driver'):
        cli.weather_scenarios(['x=damp@2-3'], None, ['x=:31/HARD'])
    with pytest.raises(ValueError, match='twice'):
        cli.weather_scenarios(['x=damp@2-3'], 'NOR', ['x=:31/HARD', 'x=:32/HARD'])


def test_weather_cli_with_a_stand_in_predictor(tmp_path, capsys, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, device=0):
            pass

        def predict_weather(self, season, race, fixture, changes, strategies=None, model=None, state=None, n_simulations=0,
                            seed=None, allow_single_compound=False):
            seen.update(changes=changes, strategies=strategies, model=model, n=n_simulations, seed=seed, state=state)
            if any(ch.first_lap < 2 for chs in changes.values() for ch in chs):
                raise ValueError("laps must be in [2, 57] (lap 1 has the configuration's condition)")
            return _result(list(changes)[:2])

    monkeypatch.setattr(cli, 'F1Predictor', Fake)
    out = tmp_path / 'w.json'
    rc = cli.main(['weather', '--race', 'Bahrain', '--offline', '--change', 'rain=damp@30-45', '--driver', 'A', '--plan',
                   'rain=:30/INTERMEDIATE', '--wrong-tyre', 'dry:INTERMEDIATE=3.5', '--simulations', '10', '--seed', '3',
                   '--json', str(out)])
    assert rc == 0
    assert list(seen['changes']) == ['as forecast', 'rain'] and seen['n'] == 10 and seen['seed'] == 3
    assert seen['changes']['rain'] == [TrackChange(30, 45, 'damp')]
    assert seen['strategies'] == {'rain': [PitPlan('A', [(30, 'INTERMEDIATE')])]}
    assert seen['model'].table()[0, 3] == 3.5
    text = capsys.readouterr().out
    assert 'scenario: as forecast' in text and 'scenario: rain' in text and '+20.0%' in text and '1.60' in text
    doc = json.load(open(out))
    assert doc['baseline'] == 'as forecast' and [r['scenario'] for r in doc['scenarios']] == ['as forecast', 'rain']
    assert doc['wrong_tyre_seconds'][0][3] == 3.5 and len(doc['wrong_tyre_seconds']) == 3
    a = doc['scenarios'][1]['drivers']['A']
    assert a['win'] == pytest.approx(0.7) and a['win_change'] == pytest.approx(0.2) and a['p_better'] == pytest.approx(0.4)
    assert a['wrong_tyre_laps'] == [0.1, 0.4, 0.3, 0.2, 0.0] and a['expected_wrong_tyre_laps'] == pytest.approx(1.6)
    assert doc['scenarios'][0]['drivers']['A']['expected_wrong_tyre_laps'] == 0.0
    for bad in ([], ['--change', 'x=damp@x'], ['--change', 'x=damp@2', '--plan', 'x=:30/HARD'],
                ['--change', 'x=damp@2', '--wrong-tyre', 'dry:SOFT=99'], ['--change', 'x=damp@1-5']):
        assert cli.main(['weather', '--race', 'Bahrain', '--offline'] + bad) == 2
    err = capsys.readouterr().err
    assert 'at least one --change' in err and '--plan needs --driver' in err and 'finite and in' in err and 'lap 1 has' in err
