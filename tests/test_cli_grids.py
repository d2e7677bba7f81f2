"""The `grid` command: flag parsing, scenario assembly, error messages and output with a stand-in predictor."""
import json

import pytest

from cli_cases import grid_result as _result
from monte_carlo_gp_amd import GridEdit, PitPlan, cli


def test_edit_parsing():
    assert cli.parse_drop('new engine=VER:engine') == ('new engine', GridEdit.drop('VER', 10))
    assert cli.parse_drop(' gearbox = NOR : 5 ') == ('gearbox', GridEdit('NOR', 'drop', 5))
    assert cli.parse_drop('x=VER:back') == ('x', GridEdit.back('VER')) and GridEdit.back('VER').value == 255
    assert cli.parse_drop('x=VER:FULL_PU')[1].value == 20
    assert cli.parse_pin('front row=NOR:1') == ('front row', GridEdit('NOR', 'pin', 1))
    assert cli.parse_pit_lane('pit lane=VER:2.5') == ('pit lane', GridEdit('VER', 'pit_lane', 0, 2.5))
    assert cli.parse_pit_lane('pit lane=VER') == ('pit lane', GridEdit.pit_lane('VER'))
    assert cli.parse_pit_lane('x=VER:0')[1].seconds == 0.0
    for parse, bad, msg in ((cli.parse_drop, 'VER:5', 'expected NAME=DRIVER:PLACES'),
                            (cli.parse_drop, '=VER:5', 'expected NAME=DRIVER:PLACES'),
                            (cli.parse_drop, 'x=:5', 'expected NAME=DRIVER:PLACES'),
                            (cli.parse_drop, 'x=VER', 'expected NAME=DRIVER:PLACES'),
                            (cli.parse_drop, 'x=VER:0', r'PLACES is in \[1, 255\]'),
                            (cli.parse_drop, 'x=VER:256', r'PLACES is in \[1, 255\]'),
                            (cli.parse_drop, 'x=VER:turbo', "PLACES is a number, 'back' or one of"),
                            (cli.parse_drop, 'x=VER:-3', "PLACES is a number, 'back' or one of"),
                            (cli.parse_pin, 'x=VER', 'SLOT is a grid slot'),
                            (cli.parse_pin, 'x=VER:0', 'SLOT is a grid slot'),
                            (cli.parse_pin, 'x=VER:pole', 'SLOT is a grid slot'),
                            (cli.parse_pin, 'VER:1', 'expected NAME=DRIVER:SLOT'),
                            (cli.parse_pit_lane, 'x=', r'expected NAME=DRIVER\[:SECONDS\]'),
                            (cli.parse_pit_lane, 'x=VER:slow', 'SECONDS is a number'),
                            (cli.parse_pit_lane, 'x=VER:-1', r'SECONDS is in \[0, 1e6\]'),
                            (cli.parse_pit_lane, 'x=VER:nan', r'SECONDS is in \[0, 1e6\]')):
        with pytest.raises(ValueError, match=msg):
            parse(bad)


def test_plan_parsing():
    assert cli.parse_grid_plan('pit lane=VER:HARD@0:30/MEDIUM') == ('pit lane', PitPlan('VER', [(30, 'MEDIUM')], start='HARD'))
    name, plan = cli.parse_grid_plan('x=NOR:soft@3:20/HARD,40/MEDIUM')
    assert (name, plan) == ('x', PitPlan('NOR', [(20, 'HARD'), (40, 'MEDIUM')], start='SOFT', start_age=3))
    assert cli.parse_grid_plan('x=NOR::25/HARD')[1] == PitPlan('NOR', [(25, 'HARD')])
    assert cli.parse_grid_plan('x=NOR:MEDIUM:')[1] == PitPlan('NOR', [], start='MEDIUM')
    for bad, msg in (('x=NOR', 'expected NAME=DRIVER:START'), ('x=NOR:HARD', 'expected NAME=DRIVER:START'),
                     ('NOR:HARD:30/MEDIUM', 'expected NAME=DRIVER:START'), ('x=NOR:@2:30/HARD', 'START@AGE needs'),
                     ('x=NOR:HARD@new:30/MEDIUM', 'START@AGE needs'), ('x=NOR:HARD:30', 'a stop is LAP/COMP')):
        with pytest.raises(ValueError, match=msg):
            cli.parse_grid_plan(bad)


def test_scenario_assembly():
    edits, plans = cli.grid_scenarios(['new engine=VER:engine'], ['front row=NOR:1', 'front row=VER:2'], ['pit lane=VER:2.5'],
                                      ['pit lane=VER:HARD@0:30/MEDIUM'])
    assert list(edits) == ['forecast grid', 'new engine', 'front row', 'pit lane'] and edits['forecast grid'] == []
    assert edits['new engine'] == [GridEdit.drop('VER', 10)]
    assert edits['front row'] == [GridEdit.pin('NOR', 1), GridEdit.pin('VER', 2)]
    assert edits['pit lane'] == [GridEdit.pit_lane('VER', 2.5)]
    assert plans == {'pit lane': [PitPlan('VER', [(30, 'MEDIUM')], start='HARD')]}
    # a plan of a new name makes a scenario of its own; the user's own baseline stays first; two drivers may plan
    edits, plans = cli.grid_scenarios(['forecast grid=VER:3'], plans=['tyres=NOR::20/HARD', 'tyres=VER::22/HARD'])
    assert list(edits) == ['forecast grid', 'tyres'] and edits['forecast grid'] == [GridEdit.drop('VER', 3)]
    assert edits['tyres'] == [] and [p.driver for p in plans['tyres']] == ['NOR', 'VER']
    with pytest.raises(ValueError, match='at least one --drop'):
        cli.grid_scenarios()
    with pytest.raises(ValueError, match='at least one --drop'):
        cli.grid_scenarios(plans=['x=NOR::20/HARD'])
    with pytest.raises(ValueError, match="--pit-lane 'x=VER': VER has an edit in scenario 'x' already"):
        cli.grid_scenarios(['x=VER:5'], [], ['x=VER'])
    with pytest.raises(ValueError, match="VER has a plan in scenario 'x' already"):
        cli.grid_scenarios(['x=VER:5'], plans=['x=VER::20/HARD', 'x=VER::21/HARD'])


def test_grid_cli_with_a_stand_in_predictor(tmp_path, capsys, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, device=0):
            pass

        def predict_grids(self, season, race, fixture, edits, strategies=None, n_simulations=0, seed=None,
                          prediction_point='fp2', allow_single_compound=False):
            seen.update(edits=edits, strategies=strategies, n=n_simulations, seed=seed)
            if any(e.kind == 'pin' and e.value > 20 for es in edits.values() for e in es):
                raise ValueError('the slot must be in [1, 20]')
            return _result(list(edits)[:2])

    monkeypatch.setattr(cli, 'F1Predictor', Fake)
    out = tmp_path / 'g.json'
    rc = cli.main(['grid', '--race', 'Bahrain', '--offline', '--driver', 'A', '--pit-lane', 'pit lane=A:2.5', '--plan',
                   'pit lane=A:HARD@0:30/MEDIUM', '--simulations', '10', '--seed', '3', '--json', str(out)])
    assert rc == 0
    assert list(seen['edits']) == ['forecast grid', 'pit lane'] and seen['n'] == 10 and seen['seed'] == 3
    assert seen['edits']['pit lane'] == [GridEdit.pit_lane('A', 2.5)]
    assert seen['strategies'] == {'pit lane': [PitPlan('A', [(30, 'MEDIUM')], start='HARD')]}
    text = capsys.readouterr().out
    assert 'scenario: forecast grid' in text and 'scenario: pit lane  [A:pit_lane+2.5s]' in text
    assert '-30.0%' in text and '3.00' in text and '+0.70' in text
    doc = json.load(open(out))
    assert doc['baseline'] == 'forecast grid' and [r['scenario'] for r in doc['scenarios']] == ['forecast grid', 'pit lane']
    a = doc['scenarios'][1]['drivers']['A']
    assert a['win'] == pytest.approx(0.2) and a['win_change'] == pytest.approx(-0.3) and a['p_worse'] == pytest.approx(0.6)
    assert a['expected_start'] == pytest.approx(3.0) and a['expected_places_gained'] == pytest.approx(0.7)
    assert doc['scenarios'][0]['drivers']['A']['expected_places_gained'] == 0.0
    assert doc['scenarios'][1]['expected_start'] == pytest.approx({'A': 3.0, 'B': 1.3, 'C': 1.7})
    for bad in ([], ['--drop', 'x=A'], ['--drop', 'x=A:3', '--pin', 'x=A:2'], ['--pin', 'x=A:21'],
                ['--pit-lane', 'x=A:slow'], ['--drop', 'x=A:3', '--plan', 'x=A:HARD']):
        assert cli.main(['grid', '--race', 'Bahrain', '--offline'] + bad) == 2
    err = capsys.readouterr().err
    assert 'at least one --drop' in err and 'expected NAME=DRIVER:PLACES' in err and 'has an edit in scenario' in err
    assert 'the slot must be in [1, 20]' in err and 'SECONDS is a number' in err and 'expected NAME=DRIVER:START' in err
