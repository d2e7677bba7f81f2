"""Tyre stints, host side: the C-ABI argument checks of mcgp_run_stints (no device needed), the binding against the
header, the sequence codes, StintResult's readers on hand-made counts, the predictor's block, the CLI flags, and the two
references of the GPU tests pinned to each other: the numpy restatement over the oracle's trace
(stints_ref.stint_counts) and the wrapped Python restatement (stints_ref.restated_counts)."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import oracle_py as O
import resume_ref as RR
import stints_ref as SR
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, StintResult, cli, decode_stints, encode_stints
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import predictor as P
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, MANY_STINTS, _Problem, stint_string

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mcgp.h')
OUTS = ('hist', 'stop_lap', 'stops_pos', 'seq')


# ---------------------------------------------------------------- the C ABI without a device
def _state(n, lap=10, **over):
    a = dict(cumulative_time=np.arange(n, dtype=np.float64) + 900.0, last_lap_time=np.full(n, 90.0),
             grid_slot=np.arange(n, dtype=np.uint8), compound=np.zeros(n, np.uint8), used_compounds=np.ones(n, np.uint8),
             tire_age=np.full(n, 5, np.int16), retired_lap=np.zeros(n, np.int16))
    a.update(over)
    return a, lap, 0


def _abi_call(n=3, n_sims=100, device=0, deviates=32, laps=60, fill=0, null=(), state=None, both=False):
    lib = N.lib()
    c = O.load_case('S60')
    m = max(n, 1)
    prob = _Problem(RaceConfig(**dict(c['config'], total_laps=laps)), [f'D{i:02d}' for i in range(m)], {}, {}, {}, None,
                    'dry', DEFAULT_SET_POP, deviates)
    prob.cfg.total_laps = laps          # (RaceConfig does not check it: the library does)
    g = np.full((m, m), 1.0 / m)
    cs = RR.c_state(*state) if state is not None else None
    bufs = {k: np.full(1 << 18, fill, np.uint64) for k in OUTS}
    ptr = lambda k: None if k in null else bufs[k].ctypes.data_as(C.POINTER(C.c_uint64))
    use_grid = (state is None or both) and 'grid_probs' not in null
    rc = lib.mcgp_run_stints(C.byref(prob.cfg), C.byref(prob.drv),
                             g.ctypes.data_as(C.POINTER(C.c_double)) if use_grid else None,
                             C.byref(cs) if cs is not None else None, n, n_sims, 0, 1, device, ptr('hist'),
                             ptr('stop_lap'), ptr('stops_pos'), ptr('seq'))
    return rc, lib.mcgp_last_error().decode(), bufs


def test_binding_matches_the_header():
    L = N.lib()
    assert L.mcgp_abi_version() == N.ABI_VERSION == 6                 # an added entry point only: a caller tests for the symbol
    assert 'mcgp_run_stints' in N.EXPORTS and hasattr(L, 'mcgp_run_stints')
    with open(HEADER) as f:
        text = f.read()
    consts = dict(re.findall(r'#define (MCGP_STINT_\w+) (\d+)', text))
    assert consts == {'MCGP_STINT_STOPS': '4', 'MCGP_STINT_SEQ': '4', 'MCGP_STINT_SEQ_CODES': '1296'}
    assert (N.STINT_STOPS, N.STINT_SEQ, N.STINT_SEQ_CODES) == (4, 4, 6 ** 4)
    decl = re.search(r'int32_t mcgp_run_stints\((.*?)\);', text, re.S).group(1)
    params = [' '.join(p.split()) for p in decl.split(',')]
    ctype = {'const mcgp_config *': C.POINTER(N.McgpConfig), 'const mcgp_drivers *': C.POINTER(N.McgpDrivers),
             'const double *': C.POINTER(C.c_double), 'const mcgp_race_state *': C.POINTER(N.McgpRaceState),
             'uint32_t ': C.c_uint32, 'uint64_t ': C.c_uint64, 'int32_t ': C.c_int32, 'uint64_t *': C.POINTER(C.c_uint64)}
    want = [ctype[re.match(r'(.*?[ *])\w+$', p).group(1)] for p in params]
    assert len(want) == 13 and L.mcgp_run_stints.argtypes == want == N.STINTS_ARGTYPES
    assert L.mcgp_run_stints.restype is C.c_int32
    assert [p.split()[-1].lstrip('*') for p in params][-4:] == ['hist_out', 'stop_lap_out', 'stops_pos_out', 'seq_out']


_BAD = [
    ('hist', dict(null=('hist',)), 'hist_out'),
    ('stop_lap', dict(null=('stop_lap',)), 'stop_lap_out'),
    ('neither', dict(null=('grid_probs',)), 'grid_probs'),
    ('both', dict(state=_state(3), both=True), 'grid_probs'),
    ('n0', dict(n=0), 'n must be in [1, 32]'),
    ('n33', dict(n=33), 'n must be in [1, 32]'),
    ('laps0', dict(laps=0), 'total_laps must be in [1, 1000]'),
    ('laps1001', dict(laps=1001), 'total_laps must be in [1, 1000]'),
    ('deviates53', dict(deviates=53), 'MCGP_DEVIATES_32'),
    ('state_lap', dict(state=_state(3, lap=61)), 'lap'),
    ('state_slot', dict(state=_state(3, grid_slot=np.array([0, 0, 1], np.uint8))), 'grid_slot'),
    ('state_time', dict(state=_state(3, cumulative_time=np.array([1.0, math.nan, 2.0]))), 'cumulative_time'),
    ('state_compound', dict(state=_state(3, compound=np.array([0, 5, 0], np.uint8))), 'compound'),
]


@pytest.mark.parametrize('kw,msg', [(kw, msg) for _, kw, msg in _BAD], ids=[name for name, _, _ in _BAD])
def test_library_rejects_bad_arguments_before_any_device_lookup(kw, msg):
    """MCGP_E_BAD_ARG with a message that names the field, on a machine with or without a GPU (the checks come first: the
    device index is one no machine has), and the outputs keep their values."""
    rc, err, bufs = _abi_call(fill=5, device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert all((b == 5).all() for b in bufs.values())


def test_zero_simulations_need_no_device_and_limits_are_inclusive():
    for kw in (dict(n=1, laps=1), dict(n=32, laps=1000), dict(n=3, null=('stops_pos', 'seq')),
               dict(state=_state(3, lap=60)), dict(state=_state(3, lap=1))):
        rc, err, bufs = _abi_call(n_sims=0, fill=3, device=999, **kw)
        assert rc == 0, (kw, err)
        assert all((b == 3).all() for b in bufs.values())


def test_outputs_untouched_when_the_device_lookup_fails():
    """A device index no machine has: every argument passes, the device lookup fails, the buffers keep their values."""
    for kw in (dict(), dict(state=_state(4)), dict(null=('stops_pos', 'seq'))):
        rc, err, bufs = _abi_call(n=4, device=999, fill=7, **kw)
        assert rc == -2 and 'device' in err
        assert all((b == 7).all() for b in bufs.values())


def test_run_stints_of_nothing_needs_no_device_and_python_checks_its_arguments():
    case = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**case['config']))
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'])
    res = sim.run_stints(0, *args)
    assert isinstance(res, StintResult) and res.n_simulations == 0 and res.total_laps == 60 and res.first_lap == 2
    assert res.hist.shape == (20, 20) and res.stop_lap.shape == (20, 4, 61) and res.stops_pos.shape == (20, 5, 20)
    assert res.seq.shape == (20, 1296) and not res.seq.any()
    assert sim.last_drivers == list(case['grid_probs']) and not sim.last_histogram.any()
    with pytest.raises(ValueError, match='exactly one'):
        sim.run_stints(10, None, *args[1:])
    with pytest.raises(ValueError, match='keys of grid_probs'):
        sim.run_stints(10, *args, drivers=['VER'])


# ---------------------------------------------------------------- the sequence codes
def test_codes_round_trip_over_all_1296():
    valid = 0
    for code in range(1296):
        ids = decode_stints(code)
        if code == 0:
            assert ids == () and stint_string(0) == MANY_STINTS == '5+ stints'
            continue
        digits = [(code // 6 ** j) % 6 for j in range(4)]
        m = max(j for j in range(4) if digits[j]) + 1
        if 0 in digits[:m]:
            assert ids is None, code                   # a gap between stints: no car has this code
            with pytest.raises(ValueError):
                stint_string(code)
            continue
        assert ids == tuple(x - 1 for x in digits[:m]) and all(0 <= c <= 4 for c in ids)
        assert encode_stints(ids) == code
        assert encode_stints(stint_string(code)) == code
        assert encode_stints([N.COMPOUNDS[c] for c in ids]) == code
        valid += 1
    assert valid == 5 + 25 + 125 + 625
    assert encode_stints('M-H') == 2 + 3 * 6 and stint_string(encode_stints('S-H-S')) == 'S-H-S'
    assert encode_stints(['soft', 'Hard']) == encode_stints((0, 2)) == 1 + 3 * 6
    assert encode_stints('S-M-H-S-M') == 0 and encode_stints([0] * 12) == 0
    for bad in ([], ['X'], [5], [-1], 'S-Q'):
        with pytest.raises(ValueError):
            encode_stints(bad)
    for bad in (-1, 1296):
        with pytest.raises(ValueError):
            decode_stints(bad)


# ---------------------------------------------------------------- StintResult on hand-made counts
def _hand_result():
    """5 laps, drivers A B, 10 simulations.
    A: 6 x M-H, stop on lap 3 (4 of them, 3 wins) or lap 4 (2 of them, no win); 3 x M-H-S with stops on laps 2 and 4 (all
       win); 1 x no stop on M, second.
    B: 10 x S, never stops (a retirement or a long stint); it wins once and is second 9 times."""
    r = StintResult.empty(['A', 'B'], 5, n_simulations=10)
    r.hist[:] = [[6, 4], [4, 6]]
    r.stop_lap[0, 0] = [1, 0, 3, 4, 2, 0]
    r.stop_lap[0, 1] = [7, 0, 0, 0, 3, 0]
    r.stop_lap[0, 2:, 0] = 10
    r.stop_lap[1, :, 0] = 10
    r.stops_pos[0] = [[0, 1], [3, 3], [3, 0], [0, 0], [0, 0]]
    r.stops_pos[1, 0] = [4, 6]
    r.seq[0, encode_stints('M-H')] = 6
    r.seq[0, encode_stints('M-H-S')] = 3
    r.seq[0, encode_stints('M')] = 1
    r.seq[1, encode_stints('S')] = 10
    return r


def test_result_readers():
    r = _hand_result()
    assert r.position_probabilities() == {'A': {1: 0.6, 2: 0.4}, 'B': {1: 0.4, 2: 0.6}}
    assert r.stop_count_probabilities() == {'A': [0.1, 0.6, 0.3, 0.0, 0.0], 'B': [1.0, 0.0, 0.0, 0.0, 0.0]}
    assert r.stop_lap_distribution('A').tolist() == [0.1, 0.0, 0.3, 0.4, 0.2, 0.0]
    assert r.stop_lap_distribution('A', k=1).tolist() == [0.7, 0.0, 0.0, 0.0, 0.3, 0.0]
    # 9 simulations stop: laps 2 2 2 3 3 3 3 4 4; the 10 % quantile is the 1st of them, the 90 % quantile the 9th
    assert r.stop_window('A') == (2, 4) and r.stop_window('A', lo=0.5, hi=0.5) == (3, 3)
    assert r.stop_window('A', k=1) == (4, 4) and r.stop_window('A', k=2) is None and r.stop_window('B') is None
    assert r.stop_window('A', lo=0.0, hi=1.0) == (2, 4)
    assert r.strategy_probabilities('A') == [('M-H', 0.6), ('M-H-S', 0.3), ('M', 0.1)]
    assert r.strategy_probabilities('B') == [('S', 1.0)]
    by = r.position_probabilities_by_stops('A')
    assert by.tolist() == [[0.0, 1.0], [0.5, 0.5], [1.0, 0.0], [0.0, 0.0], [0.0, 0.0]]
    assert r.win_probability_given_stops('A', 1) == 0.5 and r.win_probability_given_stops('A', 2) == 1.0
    assert r.win_probability_given_stops('A', 0) == 0.0 and r.win_probability_given_stops('A', 3) is None
    assert r.win_probability_given_stops('B', 0) == 0.4
    r.seq[0, 0] = 2                                      # column 0 reads as '5+ stints'
    assert ('5+ stints', 0.2) in r.strategy_probabilities('A')
    for call in (lambda: r.stop_window('X'), lambda: r.stop_lap_distribution('A', k=4), lambda: r.stop_window('A', lo=0.9, hi=0.1),
                 lambda: r.win_probability_given_stops('A', 5)):
        with pytest.raises(ValueError):
            call()


def test_the_predictors_block():
    t = P.tyre_keys(_hand_result())
    assert t['first_lap'] == 2 and list(t['drivers']) == ['A', 'B']
    a, b = t['drivers']['A'], t['drivers']['B']
    assert a == {'stops': [0.1, 0.6, 0.3, 0.0, 0.0], 'first_stop_window': [2, 4],
                 'strategy': {'sequence': 'M-H', 'probability': 0.6}, 'win_by_stops': [0.0, 0.5, 1.0, None, None]}
    assert b['first_stop_window'] is None and b['strategy'] == {'sequence': 'S', 'probability': 1.0}
    json.dumps(t)


# ---------------------------------------------------------------- the CLI
class _FakePredictor:
    """Stands in for F1Predictor: records the keyword arguments the CLI passes and returns a hand-made block."""
    calls = []

    def __init__(self, device=0):
        pass

    @staticmethod
    def _tyres(drivers):
        r = _hand_result()
        r.drivers = list(drivers[:2])
        return P.tyre_keys(r)

    def predict_weekend(self, season, race, fixture, prediction_point='fp2', n_simulations=0, seed=None, matchups=False,
                        **kw):
        _FakePredictor.calls.append(kw)
        drivers = list(fixture['drivers'])
        n = len(drivers)
        res = P.pack_result(drivers, {d: [1.0 / n] * n for d in drivers}, {d: {1 + i: 1.0} for i, d in enumerate(drivers)},
                            {}, prediction_point, None)
        if kw.get('tyres'):
            res['tyres'] = self._tyres(drivers)
        return res

    def predict_from_state(self, season, race, fixture, states, n_simulations=0, seed=None, **kw):
        _FakePredictor.calls.append(kw)
        drivers = list(fixture['drivers'])
        out = []
        for st in states:
            r = {'lap': st.lap, 'win_probabilities': {d: float(i == 0) for i, d in enumerate(drivers)},
                 'podium_probabilities': {d: float(i < 3) for i, d in enumerate(drivers)}, 'points_probabilities': {},
                 'full_distributions': {}}
            if kw.get('tyres'):
                r['tyres'] = self._tyres(drivers)
            out.append(r)
        return out


def test_predict_tyres_flag(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    out_json = tmp_path / 'tyres.json'
    base = ['predict', '--race', 'Bahrain', '--offline', '--simulations', '20', '--seed', '1']
    assert cli.main(base) == 0
    assert 'TYRE STRATEGY' not in capsys.readouterr().out
    assert cli.main(base + ['--tyres', '--json', str(out_json)]) == 0
    text = capsys.readouterr().out
    assert _FakePredictor.calls == [{}, {'tyres': True}]
    assert text.index('PODIUM PROBABILITIES') < text.index('TYRE STRATEGY') < text.index('WIN ODDS BY STOP COUNT')
    for piece in ('(laps 2 on)', 'laps   2-4', 'M-H  60.0%', 'none', '1 stop  50.0%', '2 stops 100.0%', '0 stops  40.0%'):
        assert piece in text, (piece, text)
    block = json.loads(out_json.read_text())['tyres']
    a = list(cli.synthetic_fixture()['drivers'])[0]
    assert block['first_lap'] == 2 and block['drivers'][a]['win_by_stops'] == [0.0, 0.5, 1.0, None, None]


def test_in_race_tyres_flag(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    drivers = list(cli.synthetic_fixture()['drivers'])
    state = {'lap': 1, 'drs_disabled_until': 0, 'cars': [
        {'driver': d, 'cumulative_time': 90.0 + i, 'last_lap_time': 90.0, 'tire_compound': 'SOFT', 'tire_age': 1,
         'used_compounds': ['SOFT'], 'retired_lap': 0} for i, d in enumerate(drivers)]}
    path = tmp_path / 'state.json'
    path.write_text(json.dumps(state))
    base = ['in-race', '--race', 'Bahrain', '--offline', '--state', str(path), '--simulations', '20', '--seed', '1']
    assert cli.main(base) == 0
    assert 'TYRE STRATEGY' not in capsys.readouterr().out
    assert cli.main(base + ['--tyres', '--json', str(tmp_path / 'o.json')]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [{}, {'tyres': True}]
    assert 'TYRE STRATEGY' in out and 'WIN ODDS BY STOP COUNT' in out
    assert json.loads((tmp_path / 'o.json').read_text())[0]['tyres']['drivers'][drivers[1]]['first_stop_window'] is None


# ---------------------------------------------------------------- the two references agree
def test_the_restatement_equals_the_oracle_trace():
    """From the grid both references exist: the wrapped Python restatement gives the oracle trace's counts."""
    for name, m in (('S60', 6), ('EVT', 6), ('WET', 4)):
        case = O.load_case(name)
        a, b = SR.stint_counts(case, m, seed=5, sim_offset=20), SR.restated_counts(case, m, seed=5, sim_offset=20)
        for k in SR.KEYS:
            assert np.array_equal(a[k], b[k]), (name, k)
    # ... and from a state: one simulation continued as itself
    case = O.load_case('S60')
    ref = RR.traced_run(case, 3, 13)
    k = 31
    st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, 13, 2, k))
    a, b = SR.continued_counts(ref, [2], k, case, 13), SR.restated_counts(case, 1, 13, sim_offset=2, state=st)
    for key in SR.KEYS:
        assert np.array_equal(a[key], b[key]), key
