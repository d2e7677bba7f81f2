"""Race movement, host side: the C-ABI argument checks of mcgp_run_moves (no device needed), the binding against the
header, MoveResult's readers on hand-made counts, the predictor's block, the CLI flags, the reference's pair-by-pair
counting on a hand-made race, and the two references of the GPU tests pinned to each other: the numpy restatement over
the oracle's trace (moves_ref.move_counts) and the wrapped Python restatement (moves_ref.restated_counts)."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import moves_ref as MR
import oracle_py as O
import resume_ref as RR
from monte_carlo_gp_amd import MoveResult, RaceConfig, RaceSimulator, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import predictor as P
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, _Problem

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mcgp.h')
OUTS = MR.KEYS


# ---------------------------------------------------------------- the C ABI without a device
def _state(n, lap=10, **over):
    a = dict(cumulative_time=np.arange(n, dtype=np.float64) + 900.0, last_lap_time=np.full(n, 90.0),
             grid_slot=np.arange(n, dtype=np.uint8), compound=np.zeros(n, np.uint8), used_compounds=np.ones(n, np.uint8),
             tire_age=np.full(n, 5, np.int16), retired_lap=np.zeros(n, np.int16))
    a.update(over)
    return a, lap, 0


def _abi_call(n=3, n_sims=100, device=0, deviates=32, laps=60, fill=0, null=(), state=None, both=False, gain=False):
    """null: the outputs (or 'grid_probs') passed as NULL; with a state start_gain is NULL unless gain=True."""
    lib = N.lib()
    c = O.load_case('S60')
    m = max(n, 1)
    prob = _Problem(RaceConfig(**dict(c['config'], total_laps=laps)), [f'D{i:02d}' for i in range(m)], {}, {}, {}, None,
                    'dry', DEFAULT_SET_POP, deviates)
    prob.cfg.total_laps = laps          # (RaceConfig does not check it: the library does)
    g = np.full((m, m), 1.0 / m)
    cs = RR.c_state(*state) if state is not None else None
    null = set(null) | ({'start_gain'} if state is not None and not gain else set())
    bufs = {k: np.full(1 << 18, fill, np.uint64) for k in OUTS}
    ptr = lambda k: None if k in null else bufs[k].ctypes.data_as(C.POINTER(C.c_uint64))
    use_grid = (state is None or both) and 'grid_probs' not in null
    rc = lib.mcgp_run_moves(C.byref(prob.cfg), C.byref(prob.drv),
                            g.ctypes.data_as(C.POINTER(C.c_double)) if use_grid else None,
                            C.byref(cs) if cs is not None else None, n, n_sims, 0, 1, device, *[ptr(k) for k in OUTS])
    return rc, lib.mcgp_last_error().decode(), bufs


def test_binding_matches_the_header():
    L = N.lib()
    assert L.mcgp_abi_version() == N.ABI_VERSION == 6                 # an added entry point only: a caller tests for the symbol
    assert 'mcgp_run_moves' in N.EXPORTS and hasattr(L, 'mcgp_run_moves')
    with open(HEADER) as f:
        text = f.read()
    consts = dict(re.findall(r'#define (MCGP_MOVE_\w+) +(\d+)', text))
    assert consts == {'MCGP_MOVE_DRIVER_CAP': '127', 'MCGP_MOVE_RACE_CAP': '1023'}
    assert (N.MOVE_DRIVER_CAP, N.MOVE_RACE_CAP, len(N.MOVE_KINDS)) == (127, 1023, 4)
    decl = re.search(r'int32_t mcgp_run_moves\((.*?)\);', text, re.S).group(1)
    params = [' '.join(p.split()) for p in decl.split(',')]
    ctype = {'const mcgp_config *': C.POINTER(N.McgpConfig), 'const mcgp_drivers *': C.POINTER(N.McgpDrivers),
             'const double *': C.POINTER(C.c_double), 'const mcgp_race_state *': C.POINTER(N.McgpRaceState),
             'uint32_t ': C.c_uint32, 'uint64_t ': C.c_uint64, 'int32_t ': C.c_int32, 'uint64_t *': C.POINTER(C.c_uint64)}
    want = [ctype[re.match(r'(.*?[ *])\w+$', p).group(1)] for p in params]
    assert len(want) == 16 and L.mcgp_run_moves.argtypes == want == N.MOVES_ARGTYPES
    assert L.mcgp_run_moves.restype is C.c_int32
    assert [p.split()[-1].lstrip('*') for p in params][-7:] == [k + '_out' for k in OUTS]


_BAD = [
    ('hist', dict(null=('hist',)), 'hist_out'),
    ('grid_fin', dict(null=('grid_fin',)), 'grid_fin_out'),
    ('neither', dict(null=('grid_probs',)), 'grid_probs'),
    ('both', dict(state=_state(3), both=True), 'grid_probs'),
    ('start_gain_with_state', dict(state=_state(3), gain=True), 'start_gain_out'),
    ('n0', dict(n=0), 'n must be in [1, 32]'),
    ('n33', dict(n=33), 'n must be in [1, 32]'),
    ('laps0', dict(laps=0), 'total_laps must be in [1, 1000]'),
    ('laps1001', dict(laps=1001), 'total_laps must be in [1, 1000]'),
    ('deviates53', dict(deviates=53), 'MCGP_DEVIATES_32'),
    ('state_lap', dict(state=_state(3, lap=61)), 'lap'),
    ('state_slot', dict(state=_state(3, grid_slot=np.array([0, 0, 1], np.uint8))), 'grid_slot'),
    ('state_time', dict(state=_state(3, cumulative_time=np.array([1.0, math.nan, 2.0]))), 'cumulative_time'),
]


@pytest.mark.parametrize('kw,msg', [(kw, msg) for _, kw, msg in _BAD], ids=[name for name, _, _ in _BAD])
def test_library_rejects_bad_arguments_before_any_device_lookup(kw, msg):
    """MCGP_E_BAD_ARG with a message that names the field, on a machine with or without a GPU (the checks come first: the
    device index is one no machine has), and the outputs keep their values."""
    rc, err, bufs = _abi_call(fill=5, device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert all((b == 5).all() for b in bufs.values())


def test_zero_simulations_need_no_device_and_limits_are_inclusive():
    for kw in (dict(n=1, laps=1), dict(n=32, laps=1000), dict(n=3, null=MR.OPTIONAL),
               dict(state=_state(3, lap=60)), dict(state=_state(3, lap=1))):
        rc, err, bufs = _abi_call(n_sims=0, fill=3, device=999, **kw)
        assert rc == 0, (kw, err)
        assert all((b == 3).all() for b in bufs.values())


def test_outputs_untouched_when_the_device_lookup_fails():
    """A device index no machine has: every argument passes, the device lookup fails, the buffers keep their values."""
    for kw in (dict(), dict(state=_state(4)), dict(null=MR.OPTIONAL)):
        rc, err, bufs = _abi_call(n=4, device=999, fill=7, **kw)
        assert rc == -2 and 'device' in err
        assert all((b == 7).all() for b in bufs.values())


def test_run_moves_of_nothing_needs_no_device_and_python_checks_its_arguments():
    case = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**case['config']))
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'])
    res = sim.run_moves(0, *args)
    assert isinstance(res, MoveResult) and res.n_simulations == 0 and res.total_laps == 60 and res.first_lap == 2
    assert res.from_grid and res.hist.shape == (20, 20) and res.grid_fin.shape == (20, 20, 20)
    assert res.start_gain.shape == (20, 40) and res.passes.shape == (20, 4, 128) and res.race_passes.shape == (1024,)
    assert res.lap_passes.shape == (61, 2) and res.pair_passes.shape == (20, 20) and not res.passes.any()
    assert sim.last_drivers == list(case['grid_probs']) and not sim.last_histogram.any()
    with pytest.raises(ValueError, match='exactly one'):
        sim.run_moves(10, None, *args[1:])
    with pytest.raises(ValueError, match='keys of grid_probs'):
        sim.run_moves(10, *args, drivers=['VER'])


# ---------------------------------------------------------------- MoveResult on hand-made counts
def _hand_result(from_grid=True):
    """Two drivers, 10 simulations.  A starts on pole 6 times and wins 5 of those and 1 of the 4 from P2."""
    r = MoveResult.empty(['A', 'B'], 5, 10, 2 if from_grid else 4, from_grid)
    r.grid_fin[0] = [[5, 1], [1, 3]]
    r.grid_fin[1] = [[3, 1], [1, 5]]
    r.hist[:] = r.grid_fin.sum(axis=1)
    if from_grid:
        r.start_gain[0] = [2, 6, 1, 1]           # -1: 2, 0: 6, +1: 1, retired on lap 1: 1
        r.start_gain[1] = [1, 7, 2, 0]
    r.passes[:, :, 0] = 10
    r.passes[0, 0, 0], r.passes[0, 0, 2], r.passes[0, 0, 127] = 4, 5, 1          # made on track: 0 x4, 2 x5, 127+ x1
    r.passes[1, 1] = r.passes[0, 0]                                             # ... which B lost
    r.passes[1, 2, 0], r.passes[1, 2, 1] = 7, 3                                   # B gains through the pits 3 times
    r.passes[0, 3] = r.passes[1, 2]
    r.race_passes[0], r.race_passes[2], r.race_passes[200] = 4, 5, 1
    r.lap_passes[2] = [100, 1]
    r.lap_passes[4] = [110, 2]
    r.pair_passes[0, 1], r.pair_passes[1, 0] = 140, 70
    return r


def test_result_readers():
    r = _hand_result()
    assert r.position_probabilities()['A'][1] == 0.6
    assert r.finish_given_grid('A', 1).tolist() == [5 / 6, 1 / 6] and r.win_probability_from('A', 2) == 0.25
    assert r.win_probability_from('B', 1) == 0.75
    assert r.positions_gained_distribution('A').tolist() == [0.1, 0.8, 0.1]          # -1, 0, +1
    assert r.expected_positions_gained() == {'A': 0.0, 'B': 0.0}
    assert r.start_gain_distribution('A').tolist() == [0.2, 0.6, 0.1, 0.1]
    g = r.expected_start_gain()
    assert g['A'] == pytest.approx(-1 / 9) and g['B'] == pytest.approx(0.1)
    assert r.passes_distribution('A', 0)[2] == 0.5 and r.passes_distribution('A', 'made_on_track')[127] == 0.1
    e = r.expected_passes()
    assert e['A']['made_on_track'] == pytest.approx(13.7) and e['B']['lost_on_track'] == pytest.approx(13.7)
    assert e['B']['gained_in_pits'] == pytest.approx(0.3) and e['A']['gained_in_pits'] == 0.0
    assert r.race_passes_distribution()[200] == 0.1 and r.expected_race_passes() == 21.0
    assert (r.race_passes_quantile(0.1), r.race_passes_quantile(0.5), r.race_passes_quantile(0.9),
            r.race_passes_quantile(1.0)) == (0, 2, 2, 200)
    assert r.passes_by_lap()[4].tolist() == [11.0, 0.2] and not r.passes_by_lap()[:2].any()
    assert r.most_frequent_passes() == [('A', 'B', 14.0), ('B', 'A', 7.0)] and r.most_frequent_passes(1) == [('A', 'B', 14.0)]
    empty = MoveResult.empty(['A', 'B'], 5)
    assert empty.finish_given_grid('A', 1) is None and empty.win_probability_from('A', 1) is None
    assert empty.expected_start_gain() == {'A': None, 'B': None} and empty.most_frequent_passes() == []
    for call in (lambda: r.finish_given_grid('C', 1), lambda: r.finish_given_grid('A', 0), lambda: r.finish_given_grid('A', 3),
                 lambda: r.passes_distribution('A', 4), lambda: r.passes_distribution('A', 'overtakes'),
                 lambda: r.race_passes_quantile(1.5), lambda: _hand_result(False).start_gain_distribution('A'),
                 lambda: _hand_result(False).expected_start_gain()):
        with pytest.raises(ValueError):
            call()


def test_the_predictors_block():
    mv = P.move_keys(_hand_result())
    assert mv['first_lap'] == 2 and list(mv['drivers']) == ['A', 'B']
    a = mv['drivers']['A']
    assert a['places_gained'] == 0.0 and a['start_gain'] == pytest.approx(-1 / 9)
    assert a['passes']['made_on_track'] == pytest.approx(13.7) and set(a['passes']) == set(N.MOVE_KINDS)
    assert mv['race_passes'] == {'expected': 21.0, 'p10': 0, 'p90': 2}
    assert mv['pairs'] == [{'a': 'A', 'b': 'B', 'per_race': 14.0}, {'a': 'B', 'b': 'A', 'per_race': 7.0}]
    json.dumps(mv)
    st = P.move_keys(_hand_result(False))
    assert st['first_lap'] == 4 and st['drivers']['A']['start_gain'] is None


# ---------------------------------------------------------------- the CLI
class _FakePredictor:
    """Stands in for F1Predictor: records the keyword arguments the CLI passes and returns a hand-made block."""
    calls = []

    def __init__(self, device=0):
        pass

    @staticmethod
    def _moves(drivers, from_grid):
        r = _hand_result(from_grid)
        r.drivers = list(drivers[:2])
        return P.move_keys(r)

    def predict_weekend(self, season, race, fixture, prediction_point='fp2', n_simulations=0, seed=None, matchups=False,
                        **kw):
        _FakePredictor.calls.append(kw)
        drivers = list(fixture['drivers'])
        n = len(drivers)
        res = P.pack_result(drivers, {d: [1.0 / n] * n for d in drivers}, {d: {1 + i: 1.0} for i, d in enumerate(drivers)},
                            {}, prediction_point, None)
        if kw.get('moves'):
            res['moves'] = self._moves(drivers, True)
        return res

    def predict_from_state(self, season, race, fixture, states, n_simulations=0, seed=None, **kw):
        _FakePredictor.calls.append(kw)
        drivers = list(fixture['drivers'])
        out = []
        for st in states:
            r = {'lap': st.lap, 'win_probabilities': {d: float(i == 0) for i, d in enumerate(drivers)},
                 'podium_probabilities': {d: float(i < 3) for i, d in enumerate(drivers)}, 'points_probabilities': {},
                 'full_distributions': {}}
            if kw.get('moves'):
                r['moves'] = self._moves(drivers, False)
            out.append(r)
        return out


def test_predict_moves_flag(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    out_json = tmp_path / 'moves.json'
    base = ['predict', '--race', 'Bahrain', '--offline', '--simulations', '20', '--seed', '1']
    assert cli.main(base) == 0
    assert 'RACE MOVEMENT' not in capsys.readouterr().out
    assert cli.main(base + ['--moves', '--json', str(out_json)]) == 0
    text = capsys.readouterr().out
    assert _FakePredictor.calls == [{}, {'moves': True}]
    assert text.index('PODIUM PROBABILITIES') < text.index('RACE MOVEMENT')
    a, b = list(cli.synthetic_fixture()['drivers'])[:2]
    for piece in ('(passes on laps 2 on', 'order changes between lap ends', '-0.11', ' 13.7', '0.0 / 0.3',
                  'on-track passes per race: 21.0 (10-90 %: 0-2)', f'{a:4} on {b:4} 14.00 per race'):
        assert piece in text, (piece, text)
    block = json.loads(out_json.read_text())['moves']
    assert block['first_lap'] == 2 and block['pairs'][0] == {'a': a, 'b': b, 'per_race': 14.0}


def test_in_race_moves_flag(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    drivers = list(cli.synthetic_fixture()['drivers'])
    state = {'lap': 3, 'drs_disabled_until': 0, 'cars': [
        {'driver': d, 'cumulative_time': 270.0 + i, 'last_lap_time': 90.0, 'tire_compound': 'SOFT', 'tire_age': 3,
         'used_compounds': ['SOFT'], 'retired_lap': 0} for i, d in enumerate(drivers)]}
    path = tmp_path / 'state.json'
    path.write_text(json.dumps(state))
    base = ['in-race', '--race', 'Bahrain', '--offline', '--state', str(path), '--simulations', '20', '--seed', '1']
    assert cli.main(base) == 0
    assert 'RACE MOVEMENT' not in capsys.readouterr().out
    assert cli.main(base + ['--moves', '--json', str(tmp_path / 'o.json')]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [{}, {'moves': True}]
    assert 'RACE MOVEMENT' in out and '(passes on laps 4 on' in out
    assert json.loads((tmp_path / 'o.json').read_text())[0]['moves']['drivers'][drivers[0]]['start_gain'] is None


# ---------------------------------------------------------------- the reference itself
def test_the_reference_on_a_hand_made_race():
    """Three cars, four laps, slots 0 1 2.  Lap 2: car 2 passes car 1 on track.  Lap 3: car 0 retires and car 1 pits
    without losing a place, so car 2's step up to the lead is no pass.  Lap 4: car 1, at tyre age 0 again, comes out
    ahead of car 2: a place through the pits."""
    cum = np.array([[[1.0, 2.0, 3.0], [11.0, 13.0, 12.0], [11.0, 24.0, 22.0], [11.0, 31.0, 32.0]]])
    dnf = np.array([[[0, 0, 0], [0, 0, 0], [3, 0, 0], [3, 0, 0]]])
    age = np.array([[[1, 1, 1], [2, 2, 2], [3, 0, 3], [3, 0, 4]]])
    slot = np.array([[0, 1, 2]])
    t = MR.tallies(cum, dnf, age, slot, 1)
    assert t['kinds'][0].tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [1, 0, 0, 1]]
    assert t['race'].tolist() == [1] and t['lap'][0].tolist() == [[0, 0], [0, 0], [1, 0], [0, 0], [0, 1]]
    assert t['pair'][0].tolist() == [[0, 0, 0], [0, 0, 0], [0, 1, 0]]
    out = MR.counts_from_tallies(t, slot, np.array([[2, 0, 1]]), 4, True)
    assert out['grid_fin'][0, 0, 2] == out['grid_fin'][1, 1, 0] == out['grid_fin'][2, 2, 1] == 1
    assert out['start_gain'][:, 2].tolist() == [1, 1, 1] and out['race_passes'][1] == 1
    assert out['passes'][2, 0, 1] == 1 and out['passes'][1, 2, 1] == 1 and out['passes'][0, :, 0].tolist() == [1, 1, 1, 1]
    # from a state after lap 2 only laps 3 and 4 count
    t2 = MR.tallies(cum, dnf, age, slot, 2)
    assert t2['race'].tolist() == [0] and t2['kinds'][0].tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]


def test_the_restatement_equals_the_oracle_trace():
    """From the grid both references exist: the wrapped Python restatement gives the oracle trace's counts."""
    for name, m in (('S60', 6), ('EVT', 6), ('WET', 4)):
        case = O.load_case(name)
        a, b = MR.move_counts(case, m, seed=5, sim_offset=20), MR.restated_counts(case, m, seed=5, sim_offset=20)
        for k in MR.KEYS:
            assert np.array_equal(a[k], b[k]), (name, k)
    # ... and from a state: one simulation continued as itself
    case = O.load_case('S60')
    ref = RR.traced_run(case, 3, 13)
    k = 31
    st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, 13, 2, k))
    a, b = MR.continued_counts(ref, [2], k), MR.restated_counts(case, 1, 13, sim_offset=2, state=st)
    for key in MR.KEYS:
        assert np.array_equal(a[key], b[key]), key
