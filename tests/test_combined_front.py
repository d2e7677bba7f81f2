"""Combined what-if scenarios, front door: RaceSimulator.run_combined's packing, scenario naming, ValueErrors and
two-compound check (zero simulations need no device), CombinedResult's helpers on hand-made counts, and the `what-if`
CLI's argument grouping and output with a stand-in predictor."""
import ctypes as C
import json

import numpy as np
import pytest

import oracle_py as O
from cli_cases import combined_result as _result
from monte_carlo_gp_amd import (CombinedResult, EventResult, PaceOffset, PaceResult, PenaltyResult, PitPlan, RaceConfig,
                                RaceEvent, StrategyResult, TimePenalty, cli)
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, RaceSimulator


def _sim():
    c = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**c['config']), set_pop=DEFAULT_SET_POP)
    args = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    return c, sim, list(c['grid_probs']), args, dict(grid_probs=c['grid_probs'], seed=1)


def test_run_combined_names_shapes_and_value_errors():
    c, sim, d, args, kw = _sim()
    L = c['config']['total_laps']
    r = sim.run_combined(0, {
        'as drawn': {},
        'sc': {'events': [RaceEvent('sc', 31)], 'plans': [PitPlan(d[0], [(31, 'HARD')])],
               'penalties': [TimePenalty(d[0], 5.0)], 'paces': [PaceOffset(d[1], 0.4, until_stop_from=31)]},
        'upgrade': {'paces': [PaceOffset(d[2], -0.2, laps=(1, L))], 'events': [RaceEvent('none', 2, L)]},
        'flag': {'penalties': [TimePenalty(d[0], 5.0, 'flag')], 'plans': None},
    }, *args, **kw)
    assert isinstance(r, CombinedResult) and r.names == ['as drawn', 'sc', 'upgrade', 'flag'] and r.n_simulations == 0
    for cls in (StrategyResult, PenaltyResult, EventResult, PaceResult):
        assert isinstance(r, cls)
    assert r.hist.shape == (4, 20, 20) and r.delta.shape == (4, 20, 39) and r.fate.shape == (4, 20, 4)
    assert r.events.shape == (4, 3, L + 1) and r.carried.shape == (4, 20, L + 1) and r.orders is None
    assert r.until_from == {('sc', d[1]): 31}
    # each kind keeps its own call's checks, with the scenario's name
    bad = [
        ({'x': {'paces': [PaceOffset(d[0], 0.5, laps=(10, 12)), PaceOffset(d[0], 0.2, laps=(12, 20))]}}, "'x'.*two offsets on lap 12"),
        ({'x': {'paces': [PaceOffset(d[0], 0.5, laps=(0, 3))]}}, "'x'.*laps must be in"),
        ({'x': {'paces': [PaceOffset(d[0], 0.1, laps=(2, 2))] * 65}}, 'at most 64 offsets'),
        ({'x': {'events': [RaceEvent('sc', 1)]}}, "'x'.*lap 1 has no event"),
        ({'x': {'events': [RaceEvent('sc', 5, 9), RaceEvent('vsc', 9)]}}, "'x'.*lap 9 has two overrides"),
        ({'x': {'events': [RaceEvent('none', 2)] * 65}}, 'at most 64 overrides'),
        ({'x': {'penalties': [TimePenalty(d[0], 5.0), TimePenalty(d[0], 10.0)]}}, "'x'.*two penalties of kind 'serve'"),
        ({'x': {'penalties': [TimePenalty('NOBODY', 5.0)]}}, 'not one of the drivers'),
        ({'x': {'plans': [PitPlan('NOBODY', [(20, 'HARD')])]}}, 'not one of the drivers'),
        ({'x': {'plans': [PitPlan(d[0], [(20, 'SOFT')], start='SOFT')]}}, "'x'.*one dry compound"),
        ({'x': {'offsets': []}}, "'x'.*keys.*offsets"),
        ({'x': [PitPlan(d[0], [(20, 'HARD')])]}, "'x'.*a dict"),
        ({}, '1 to 64 scenarios'),
        ({str(k): {} for k in range(65)}, '1 to 64 scenarios'),
    ]
    for scen, match in bad:
        with pytest.raises(ValueError, match=match):
            sim.run_combined(0, scen, *args, **kw)
    with pytest.raises(ValueError, match='exactly one of'):
        sim.run_combined(0, {'x': {}}, *args, seed=1)
    # the two-compound rule can be waived, as for the siblings
    r = sim.run_combined(0, {'x': {'plans': [PitPlan(d[0], [(20, 'SOFT')], start='SOFT')]}}, *args,
                         allow_single_compound=True, **kw)
    assert r.names == ['x']


def test_run_combined_packs_each_table_behind_the_plans(monkeypatch):
    """The C call's arguments: per table a count per scenario, in scenario order, and the items concatenated."""
    c, sim, d, args, kw = _sim()
    seen = {}

    def fake_counted(n_simulations, drivers, alloc, call, orders_axis=None):
        class Lib:
            @staticmethod
            def mcgp_run_combined(*a):
                seen['args'] = a
                return 0
        call(Lib, 0, 0, 5, alloc(5))
        return {k: (None if v is None else v.astype(np.int64)) for k, v in alloc(0).items()}

    monkeypatch.setattr(sim, '_run_counted', fake_counted)
    sim.run_combined(5, {
        'a': {'penalties': [TimePenalty(d[3], 5.0, 'flag')]},
        'b': {'events': [RaceEvent('sc', 31), RaceEvent('none', 32, 40)], 'plans': [PitPlan(d[0], [(31, 'HARD')])],
              'paces': [PaceOffset(d[1], 0.4, until_stop_from=31)]},
        'c': {'penalties': [TimePenalty(d[0], 5.0, 'lap', 7), TimePenalty(d[1], 10.0)], 'paces': [PaceOffset(d[2], 0.1, laps=(1, 3))]},
    }, *args, **kw)
    a = seen['args']
    n, S, plan_count, plans, pen_count, pens, ev_count, evs, pace_count, offs = a[4:14]
    assert (n, S) == (20, 3) and a[14] == 5 and len(a) == 24
    assert list(plan_count) == [0, 1, 0] and (plans[0].driver, plans[0].n_stops, plans[0].stop_lap[0]) == (0, 1, 31)
    assert list(pen_count) == [1, 0, 2]
    assert [(p.driver, p.kind, p.lap, p.seconds) for p in pens] == [(3, N.PEN_AT_FLAG, 0, 5.0), (0, N.PEN_ON_LAP, 7, 5.0),
                                                                    (1, N.PEN_SERVE_AT_STOP, 2, 10.0)]
    assert list(ev_count) == [0, 2, 0] and [(e.first_lap, e.last_lap) for e in evs] == [(31, 31), (32, 40)]
    assert list(pace_count) == [0, 1, 1]
    assert [(o.driver, o.kind, o.first_lap, o.last_lap) for o in offs] == [(1, N.PACE_UNTIL_STOP, 31, 0), (2, N.PACE_LAPS, 1, 3)]


def test_combined_result_offers_what_its_three_siblings_offer():
    r = _result()
    assert r.win_probability('sc', 'A') == pytest.approx(0.7) and r.compare('sc', 'A')['p_better'] == pytest.approx(0.4)
    assert r.fate_probabilities('sc', 'A') == dict(none=0.0, served=0.7, at_flag=0.2, retired=0.1)
    assert r.expected_events('sc')['sc'] == pytest.approx(0.7 + 0.4 + 0.3) and r.probability_of('sc', 'sc') == pytest.approx(1.0)
    assert r.fate_probabilities('sc', 'B')['none'] == 1.0
    assert r.carried_distribution('sc', 'B').tolist() == [0.1, 0.4, 0.3, 0.2, 0.0]
    assert r.probability_cleared_by('sc', 'B', 2) == pytest.approx(0.5)
    # the methods are the siblings' own, not copies
    assert CombinedResult.fate_probabilities is PenaltyResult.fate_probabilities
    assert CombinedResult.expected_events is EventResult.expected_events
    assert CombinedResult.probability_cleared_by is PaceResult.probability_cleared_by


# ---------------------------------------------------------------- CLI
def test_what_if_groups_items_by_their_name():
    sc = cli.what_if_scenarios('NOR', ['sc=:31/HARD'], None, ['sc=NOR:5', 'late=VER:10:flag'], ['sc=sc@31', 'green=none@2-57'],
                               ['sc=VER:0.4@31+', 'green=NOR:-0.2@1-57'])
    assert list(sc) == ['as drawn', 'sc', 'green', 'late']
    assert sc['as drawn'] == dict(plans=[], penalties=[], events=[], paces=[])
    assert sc['sc'] == dict(plans=[PitPlan('NOR', [(31, 'HARD')])], penalties=[TimePenalty('NOR', 5.0, 'serve', None)],
                            events=[RaceEvent('sc', 31, None)], paces=[PaceOffset('VER', 0.4, until_stop_from=31)])
    assert sc['green'] == dict(plans=[], penalties=[], events=[RaceEvent('none', 2, 57)],
                               paces=[PaceOffset('NOR', -0.2, laps=(1, 57))])
    assert sc['late']['penalties'] == [TimePenalty('VER', 10.0, 'flag', None)]
    # the user's own 'as drawn' stays first; a lap penalty keeps its @LAP behind the name
    sc = cli.what_if_scenarios(None, gives=['x=NOR:20:lap@12', 'as drawn=VER:5'])
    assert list(sc) == ['as drawn', 'x'] and sc['as drawn']['penalties'] == [TimePenalty('VER', 5.0, 'serve', None)]
    assert sc['x']['penalties'] == [TimePenalty('NOR', 20.0, 'lap', 12)]
    # a window sweeps the stop lap of a named scenario, or of the race as drawn
    sc = cli.what_if_scenarios('NOR', window='sc=30-32/H', gives=['sc=NOR:5'], events=['sc=sc@31'])
    assert list(sc) == ['as drawn', 'sc', 'sc L30', 'sc L31', 'sc L32']
    assert sc['sc L31'] == dict(plans=[PitPlan('NOR', [(31, 'HARD')])], penalties=sc['sc']['penalties'],
                                events=sc['sc']['events'], paces=[])
    sc = cli.what_if_scenarios('NOR', window='30-31/M')
    assert list(sc) == ['as drawn', 'NOR L30', 'NOR L31'] and sc['NOR L30']['plans'] == [PitPlan('NOR', [(30, 'MEDIUM')])]
    for kw, match in [(dict(), 'at least one'), (dict(plans=['x=:31/HARD']), '--driver'), (dict(window='30-31/M'), '--driver'),
                      (dict(gives=['NOR:5']), 'NAME='), (dict(gives=['=NOR:5']), 'NAME='), (dict(gives=['x=NOR']), '--give'),
                      (dict(events=['x=sc']), '--event'), (dict(offsets=['x=NOR:0.6']), '--offset'),
                      (dict(driver='NOR', plans=['x=:31/HARD', 'x=:32/HARD']), 'twice'),
                      (dict(driver='NOR', window='y=30-31/M', gives=['x=NOR:5']), "no scenario 'y'"),
                      (dict(driver='NOR', window='x=30-31/M', plans=['x=:31/HARD']), 'has a --plan')]:
        with pytest.raises(ValueError, match=match):
            cli.what_if_scenarios(**kw)


def test_what_if_cli_with_a_stand_in_predictor(tmp_path, capsys, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, device=0):
            pass

        def predict_combined(self, season, race, fixture, scenarios, state=None, n_simulations=0, seed=None,
                             allow_single_compound=False):
            seen.update(scenarios=scenarios, n=n_simulations, seed=seed, state=state)
            if any(p.seconds > 60 for sc in scenarios.values() for p in sc['paces']):
                raise ValueError('seconds must be finite and in [-60, 60]')
            r = _result()
            r.names = list(scenarios)[:2]
            r.until_from = {(r.names[1], 'B'): 2}
            return r

    monkeypatch.setattr(cli, 'F1Predictor', Fake)
    out = tmp_path / 'w.json'
    rc = cli.main(['what-if', '--race', 'Bahrain', '--season', '2024', '--offline', '--driver', 'A', '--event', 'sc=sc@3',
                   '--plan', 'sc=:3/HARD', '--give', 'sc=A:5', '--offset', 'sc=B:0.4@2+', '--simulations', '10', '--seed',
                   '3', '--json', str(out)])
    assert rc == 0
    assert list(seen['scenarios']) == ['as drawn', 'sc'] and seen['n'] == 10 and seen['seed'] == 3 and seen['state'] is None
    assert seen['scenarios']['sc']['plans'] == [PitPlan('A', [(3, 'HARD')])]
    text = capsys.readouterr().out
    assert 'scenario: as drawn' in text and 'scenario: sc   (laps with: safety car 1.40' in text
    assert 'penalty served at a stop 70.0%, added at the flag 20.0%, retired unserved 10.0%' in text
    assert 'offset carried 1.60 laps on average' in text and '+20.0%' in text
    lines = [ln.split()[0] for ln in text.splitlines() if ln.startswith('  A ') or ln.startswith('  B ')]
    assert lines == ['A', 'B', 'A', 'B']                    # --driver and the driver an item names, in both scenarios
    doc = json.load(open(out))
    assert doc['baseline'] == 'as drawn' and [r['scenario'] for r in doc['scenarios']] == ['as drawn', 'sc']
    a, b = doc['scenarios'][1]['drivers']['A'], doc['scenarios'][1]['drivers']['B']
    assert a['win'] == pytest.approx(0.7) and a['win_change'] == pytest.approx(0.2) and a['fate']['served'] == pytest.approx(0.7)
    assert b['laps_carried'] == [0.1, 0.4, 0.3, 0.2, 0.0] and 'fate' not in b and 'laps_carried' not in a
    assert doc['scenarios'][1]['expected_events']['sc'] == pytest.approx(1.4) and 'expected_events' not in doc['scenarios'][0]
    assert cli.main(['what-if', '--race', 'Bahrain', '--offline']) == 2                         # nothing given
    assert cli.main(['what-if', '--race', 'Bahrain', '--offline', '--give', 'A:5']) == 2        # no NAME=
    assert cli.main(['what-if', '--race', 'Bahrain', '--offline', '--plan', 'x=:30/HARD']) == 2     # no --driver
    assert cli.main(['what-if', '--race', 'Bahrain', '--offline', '--offset', 'x=A:99@2+']) == 2    # the library's ValueError
