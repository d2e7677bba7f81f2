"""Race trace, host side: the C-ABI argument checks of mcgp_run_trace (no device needed), TraceResult's derived odds on
hand-made counts, the numpy restatement against the oracle's own finishing orders, and `predict --trace` with a stand-in
predictor."""
import ctypes as C
import json

import numpy as np
import pytest

import oracle_py as O
import trace_ref as TR
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, TraceResult, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import predictor as P
from monte_carlo_gp_amd.simulation import _Problem, DEFAULT_SET_POP


# ---------------------------------------------------------------- the C ABI without a device
def _abi_call(n=3, n_sims=100, device=0, deviates=32, laps=60, fill=0, null=(), config=None):
    lib = N.lib()
    c = O.load_case('S60')
    cfg = dict(c['config'], total_laps=laps, **(config or {}))
    m = max(n, 1)
    prob = _Problem(RaceConfig(**cfg), [f'D{i:02d}' for i in range(m)], {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)
    prob.cfg.total_laps = laps          # (RaceConfig does not check it: the library does)
    g = np.full((m, m), 1.0 / m)
    size = 1001 * 33 * 33
    bufs = {k: np.full(size, fill, np.uint64) for k in ('hist', 'lap_pos', 'laps_led', 'stops', 'fastest', 'events')}
    ptr = lambda k: None if k in null else bufs[k].ctypes.data_as(C.POINTER(C.c_uint64))
    rc = lib.mcgp_run_trace(C.byref(prob.cfg), C.byref(prob.drv),
                            None if 'grid_probs' in null else g.ctypes.data_as(C.POINTER(C.c_double)), n, n_sims, 0, 1,
                            device, ptr('hist'), ptr('lap_pos'), ptr('laps_led'), ptr('stops'), ptr('fastest'),
                            ptr('events'))
    return rc, lib.mcgp_last_error().decode(), bufs


def test_abi_version_matches_the_binding():
    L = N.lib()
    assert L.mcgp_abi_version() == N.ABI_VERSION == 6
    assert 'mcgp_run_trace' in N.EXPORTS and hasattr(L, 'mcgp_run_trace')


@pytest.mark.parametrize('kw,msg', [
    (dict(null=('hist',)), 'hist_out'),
    (dict(null=('lap_pos',)), 'lap_pos_out'),
    (dict(null=('grid_probs',)), 'grid_probs'),
    (dict(n=0), 'n must be in [1, 32]'),
    (dict(n=33), 'n must be in [1, 32]'),
    (dict(laps=0), 'total_laps must be in [1, 1000]'),
    (dict(laps=1001), 'total_laps must be in [1, 1000]'),
    (dict(deviates=53), 'MCGP_DEVIATES_32'),
], ids=['hist', 'lap_pos', 'grid_probs', 'n0', 'n33', 'laps0', 'laps1001', 'deviates53'])
def test_library_rejects_bad_arguments_before_any_device_lookup(kw, msg):
    """MCGP_E_BAD_ARG with a message that names the field, on a machine with or without a GPU (checks come first), and
    the outputs keep their values."""
    rc, err, bufs = _abi_call(fill=5, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert all((b == 5).all() for b in bufs.values())


def test_zero_simulations_need_no_device_and_limits_are_inclusive():
    for kw in (dict(n=1, laps=1), dict(n=32, laps=1000), dict(n=2, null=('laps_led', 'stops', 'fastest', 'events'))):
        rc, err, bufs = _abi_call(n_sims=0, fill=3, **kw)
        assert rc == 0, (kw, err)
        assert all((b == 3).all() for b in bufs.values())


def test_outputs_untouched_when_the_device_lookup_fails():
    """A device index no machine has: every argument passes, the device lookup fails, the buffers keep their values."""
    rc, err, bufs = _abi_call(n=4, device=999, fill=7)
    assert rc == -2 and 'device' in err
    assert all((b == 7).all() for b in bufs.values())


def test_run_trace_of_nothing_needs_no_device():
    case = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**case['config']))
    res = sim.run_trace(0, case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'])
    assert isinstance(res, TraceResult) and res.n_simulations == 0 and res.total_laps == 60
    assert res.lap_pos.shape == (60, 20, 21) and res.laps_led.shape == (20, 61) and res.events.shape == (3, 61)
    assert not res.lap_pos.any() and sim.last_drivers == list(case['grid_probs']) and not sim.last_histogram.any()
    assert res.event_probabilities['safety_car'] == {'probability': 0.0, 'expected': 0.0}


# ---------------------------------------------------------------- TraceResult on hand-made counts
def _hand_result():
    """3 laps, drivers A B, 4 simulations:
       sim 0: A leads laps 1-3; B pits on lap 2; fastest A;   one SC
       sim 1: A leads laps 1-3;                   fastest B;  one SC, one VSC
       sim 2: B leads laps 1-3; A pits on lap 2 and 3; fastest B;   two SCs
       sim 3: A leads lap 1, retires on lap 2; B leads laps 2-3; fastest B; a red flag"""
    L, n = 3, 2
    lap_pos = np.zeros((L, n, n + 1), np.int64)
    lap_pos[0] = [[3, 1, 0], [1, 3, 0]]
    lap_pos[1] = [[2, 1, 1], [2, 1, 0]]
    lap_pos[2] = [[2, 1, 1], [2, 1, 0]]
    hist = np.array([[2, 2], [2, 2]])
    laps_led = np.array([[1, 1, 0, 2], [2, 0, 1, 1]])       # A: 0 laps (sim 2), 1 (sim 3), 3 (sims 0, 1)
    stops = np.array([[3, 0, 1, 0], [3, 1, 0, 0]])
    fastest = np.array([1, 3])
    events = np.array([[3, 1, 0, 0], [1, 2, 1, 0], [3, 1, 0, 0]])
    return TraceResult(drivers=['A', 'B'], n_simulations=4, total_laps=L, hist=hist, lap_pos=lap_pos,
                       laps_led=laps_led, stops=stops, fastest=fastest, events=events)


def test_result_derivations():
    r = _hand_result()
    assert r.position_probabilities == {'A': {1: 0.5, 2: 0.5}, 'B': {1: 0.5, 2: 0.5}}
    assert r.leader_probabilities['A'].tolist() == [0.75, 0.5, 0.5]
    assert r.leader_probabilities['B'].tolist() == [0.25, 0.5, 0.5]
    assert r.retired_by_lap['A'].tolist() == [0.0, 0.25, 0.25] and r.retired_by_lap['B'].tolist() == [0.0, 0.0, 0.0]
    assert r.position_probabilities_by_lap['A'].shape == (3, 3)
    assert r.position_probabilities_by_lap['A'][1].tolist() == [0.5, 0.25, 0.25]
    assert r.laps_led_distribution['A'].tolist() == [0.25, 0.25, 0.0, 0.5]
    assert r.expected_laps_led == {'A': 1.75, 'B': 1.25}
    assert r.pit_stop_distribution['A'].tolist() == [0.75, 0.0, 0.25, 0.0]
    assert r.expected_pit_stops == {'A': 0.5, 'B': 0.25}
    assert r.fastest_lap_probabilities == {'A': 0.25, 'B': 0.75}
    ev = r.event_probabilities
    assert ev['red_flag'] == {'probability': 0.25, 'expected': 0.25}
    assert ev['safety_car'] == {'probability': 0.75, 'expected': 1.0}
    assert ev['vsc'] == {'probability': 0.25, 'expected': 0.25}
    keys = P.trace_keys(r)
    assert keys['leader_by_lap'] == {'A': [0.75, 0.5, 0.5], 'B': [0.25, 0.5, 0.5]}
    assert keys['pit_stop_distribution'] == {'A': [0.75, 0.0, 0.25], 'B': [0.75, 0.25, 0.0]}
    assert keys['fastest_lap_probabilities'] == {'A': 0.25, 'B': 0.75}
    assert keys['race_event_probabilities'] == ev
    json.dumps(keys)                                    # JSON-safe


# ---------------------------------------------------------------- the restatement against the oracle's own orders
@pytest.mark.parametrize('name', ['S60', 'EVT'])
def test_restatement_agrees_with_the_oracle_orders(name):
    """After lap L the running positions are the classified positions of the runners; laps led and lap-1 leaders agree
    with the per-lap counts; every simulation is counted once per row."""
    case = O.load_case(name)
    m, L = 96, case['config']['total_laps']
    t = TR.trace_counts(case, m, seed=11)
    n = t['hist'].shape[0]
    assert (t['lap_pos'].sum(axis=2) == m).all()
    assert (t['lap_pos'][L - 1][:, :n] <= t['hist']).all()
    assert (t['laps_led'] @ np.arange(L + 1) == t['lap_pos'][:, :, 0].sum(axis=0)).all()
    assert (t['laps_led'].sum(axis=1) == m).all() and (t['stops'].sum(axis=1) == m).all()
    assert t['fastest'].sum() <= m and (t['events'].sum(axis=1) == m).all()
    assert t['stops'][:, 1:].sum() > 0                  # somebody pits in 60 / 34 laps


def test_restatement_on_every_fuzz_configuration():
    """The 84 configurations of tests/golden/fuzz_cases.json: the sum identities of the counts, the number of fastest laps
    counted directly from the oracle's retirement trace, and hand values of the corner cases."""
    import resume_ref as RR
    with open(O.GOLDEN_DIR + '/fuzz_cases.json') as f:
        cases = json.load(f)
    m, counts = 32, {}
    for name, case in cases.items():
        L, seed = case['config']['total_laps'], case['seed']
        t = counts[name] = TR.trace_counts(case, m, seed)
        assert (t['lap_pos'].sum(axis=2) == m).all(), name
        assert (t['laps_led'].sum(axis=1) == m).all() and (t['stops'].sum(axis=1) == m).all(), name
        assert (t['events'].sum(axis=1) == m).all(), name
        assert (t['laps_led'] @ np.arange(L + 1) == t['lap_pos'][:, :, 0].sum(axis=0)).all(), name
        # a fastest lap exists where some car is running after some lap >= 2
        dnf = RR.traced_run(case, m, seed)['trace']['dnf']
        assert t['fastest'].sum() == (dnf[:, 1:, :] == 0).any(axis=(1, 2)).sum(), name
    assert len(counts) == 84
    one = counts['X_onelap']                            # no lap >= 2: no fastest lap, no event draw, no stop
    assert (one['fastest'] == 0).all() and (one['events'][:, 0] == m).all() and (one['stops'][:, 0] == m).all()
    for kind, name in ((TR.RED, 'X_always_red'), (TR.SC, 'X_always_sc'), (TR.VSC, 'X_always_vsc')):
        L = cases[name]['config']['total_laps']
        assert counts[name]['events'][kind, L - 1] == m, name       # laps 2 .. L
    assert (counts['X_all_out_lap1']['fastest'] == 0).all()


# ---------------------------------------------------------------- the CLI flag
class _FakePredictor:
    """predict_weekend's result shape from hand-made counts (no device)."""
    calls = []

    def __init__(self, device=0):
        pass

    def predict_weekend(self, season, race, fixture, prediction_point='fp2', n_simulations=0, seed=None, matchups=False,
                        **kw):
        _FakePredictor.calls.append(kw)
        drivers = list(fixture['drivers'])
        n = len(drivers)
        probs = {d: {1 + (i % n): 1.0} for i, d in enumerate(drivers)}
        res = P.pack_result(drivers, {d: [1.0 / n] * n for d in drivers}, probs, {}, prediction_point, None)
        if kw.get('trace'):
            L = 4
            r = TraceResult.empty(drivers, L, 2)
            r.lap_pos[:, :, 0] = 0
            r.lap_pos[:, 0, 0] = 2
            r.laps_led[:, 0] = 2
            r.laps_led[0] = [0, 0, 0, 0, 2]
            r.stops[:, 1] = 2
            r.fastest[1] = 2
            r.events[:, 0] = 2
            r.events[1] = [1, 1, 0, 0, 0]
            res.update(P.trace_keys(r))
        return res


def test_predict_trace_flag(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    plain, extra = tmp_path / 'plain.json', tmp_path / 'trace.json'
    base = ['predict', '--race', 'Bahrain', '--offline', '--simulations', '20', '--seed', '1']
    assert cli.main(base + ['--json', str(plain)]) == 0
    out_plain = capsys.readouterr().out
    assert 'LAP LEADER' not in out_plain and 'SAFETY CAR' not in out_plain
    assert cli.main(base + ['--trace', '--json', str(extra)]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [{}, {'trace': True}]          # the default call passes no new argument
    for title in ('LAP LEADER', 'LAPS LED', 'FASTEST LAP', 'PIT STOPS', 'SAFETY CAR'):
        assert title in out, title
    assert out.index('PODIUM PROBABILITIES') < out.index('LAP LEADER') < out.index('SAFETY CAR')
    a, b = json.loads(plain.read_text()), json.loads(extra.read_text())
    new = {'leader_by_lap', 'expected_laps_led', 'pit_stop_distribution', 'expected_pit_stops',
           'fastest_lap_probabilities', 'race_event_probabilities'}
    assert not new & set(a) and set(b) == set(a) | new
    assert {k: b[k] for k in a} == a
    first = list(b['leader_by_lap'])[0]
    assert b['leader_by_lap'][first] == [1.0] * 4 and b['expected_laps_led'][first] == 4.0
    assert b['race_event_probabilities']['safety_car'] == {'probability': 0.5, 'expected': 0.5}
    assert 'safety car' in out and '50.0%' in out
