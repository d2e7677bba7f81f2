"""Pit windows, host side: the C-ABI argument checks of mcgp_run_pit_windows (no device needed), the binding against the
header, PitWindowResult's readers on hand-made counts, the command's parsing with its 64-window limit (and cli.main's
parser untouched), and the reference of the GPU tests (window_ref) checked on a hand-made race."""
import ctypes as C
import importlib
import json
import math
import os
import re

import numpy as np
import pytest

import oracle_py as O
import resume_ref as RR
import window_ref as WR
import monte_carlo_gp_amd
from monte_carlo_gp_amd import PitWindowResult, RaceConfig, RaceSimulator, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import predictor as P
from monte_carlo_gp_amd.simulation import DEFAULT_GAP_EDGES, DEFAULT_SET_POP, IN_THE_LEAD, _Problem
from monte_carlo_gp_amd.simulation import pit_window as strategy_windows

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mcgp.h')
OUTS = ('hist', 'rejoin', 'lost', 'ahead', 'gap_ahead', 'gap_behind')


def _command():
    return importlib.import_module('monte_carlo_gp_amd.pit_window')


# ---------------------------------------------------------------- the C ABI without a device
def _state(n, lap=10, **over):
    a = dict(cumulative_time=np.arange(n, dtype=np.float64) + 900.0, last_lap_time=np.full(n, 90.0),
             grid_slot=np.arange(n, dtype=np.uint8), compound=np.zeros(n, np.uint8), used_compounds=np.ones(n, np.uint8),
             tire_age=np.full(n, 5, np.int16), retired_lap=np.zeros(n, np.int16))
    a.update(over)
    return a, lap, 0


def _abi_call(n=3, n_sims=100, device=0, deviates=32, laps=60, fill=0, null=(), edges=(1.0, 5.0), windows=((0, 21.0),),
              state=None, both=False, n_edges=None, n_windows=None):
    lib = N.lib()
    c = O.load_case('S60')
    m = max(n, 1)
    prob = _Problem(RaceConfig(**dict(c['config'], total_laps=laps)), [f'D{i:02d}' for i in range(m)], {}, {}, {}, None,
                    'dry', DEFAULT_SET_POP, deviates)
    prob.cfg.total_laps = laps          # (RaceConfig does not check it: the library does)
    g = np.full((m, m), 1.0 / m)
    e = np.ascontiguousarray(edges, np.float64)
    wd = np.ascontiguousarray([w[0] for w in windows], np.uint8)
    wl = np.ascontiguousarray([w[1] for w in windows], np.float64)
    cs = RR.c_state(*state) if state is not None else None
    bufs = {k: np.full(1 << 17, fill, np.uint64) for k in OUTS}
    ptr = lambda k: None if k in null else bufs[k].ctypes.data_as(C.POINTER(C.c_uint64))
    use_grid = (state is None or both) and 'grid_probs' not in null
    rc = lib.mcgp_run_pit_windows(
        C.byref(prob.cfg), C.byref(prob.drv), g.ctypes.data_as(C.POINTER(C.c_double)) if use_grid else None,
        C.byref(cs) if cs is not None else None, n, len(e) if n_edges is None else n_edges,
        None if 'edges' in null else e.ctypes.data_as(C.POINTER(C.c_double)), len(wd) if n_windows is None else n_windows,
        None if 'window_drivers' in null or not len(wd) else wd.ctypes.data_as(C.POINTER(C.c_uint8)),
        None if 'window_losses' in null or not len(wl) else wl.ctypes.data_as(C.POINTER(C.c_double)),
        n_sims, 0, 1, device, *[ptr(k) for k in OUTS])
    return rc, lib.mcgp_last_error().decode(), bufs


def test_binding_matches_the_header():
    L = N.lib()
    assert L.mcgp_abi_version() == N.ABI_VERSION == 6                 # an added entry point only: a caller tests for the symbol
    assert 'mcgp_run_pit_windows' in N.EXPORTS and hasattr(L, 'mcgp_run_pit_windows')
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r'#define MCGP_ABI_VERSION 6\b', text)
    assert re.findall(r'#define MCGP_MAX_PIT_WINDOWS (\d+)', text) == [str(N.MAX_PIT_WINDOWS)] == ['64']
    decl = re.search(r'int32_t mcgp_run_pit_windows\((.*?)\);', text, re.S).group(1)
    params = [' '.join(p.split()) for p in decl.split(',')]
    ctype = {'const mcgp_config *': C.POINTER(N.McgpConfig), 'const mcgp_drivers *': C.POINTER(N.McgpDrivers),
             'const double *': C.POINTER(C.c_double), 'const mcgp_race_state *': C.POINTER(N.McgpRaceState),
             'uint32_t ': C.c_uint32, 'uint64_t ': C.c_uint64, 'int32_t ': C.c_int32,
             'const uint8_t *': C.POINTER(C.c_uint8), 'uint64_t *': C.POINTER(C.c_uint64)}
    want = [ctype[re.match(r'(.*?[ *])\w+$', p).group(1)] for p in params]
    assert len(want) == 20 and L.mcgp_run_pit_windows.argtypes == want == N.PIT_WINDOWS_ARGTYPES
    assert L.mcgp_run_pit_windows.restype is C.c_int32
    assert [p.split()[-1].lstrip('*') for p in params] == [
        'cfg', 'drv', 'grid_probs', 'state', 'n', 'n_edges', 'edges', 'n_windows', 'window_drivers', 'window_losses',
        'n_sims', 'sim_offset', 'seed', 'device', 'hist_out', 'rejoin_out', 'lost_out', 'ahead_out', 'gap_ahead_out',
        'gap_behind_out']
    # the header says what the call is not
    doc = text[text.index('/* Pit window:'):text.index('#define MCGP_MAX_PIT_WINDOWS')]
    assert 'NOTHING IS RE-SIMULATED' in doc and 'mcgp_run_strategies' in doc


_BAD = [
    ('hist', dict(null=('hist',)), 'hist_out is NULL'),
    ('rejoin', dict(null=('rejoin',)), 'rejoin_out is NULL'),
    ('lost', dict(null=('lost',)), 'lost_out is NULL'),
    ('ahead', dict(null=('ahead',)), 'ahead_out is NULL'),
    ('gap_ahead', dict(null=('gap_ahead',)), 'gap_ahead_out is NULL'),
    ('gap_behind', dict(null=('gap_behind',)), 'gap_behind_out is NULL'),
    ('neither', dict(null=('grid_probs',)), 'grid_probs'),
    ('both', dict(state=_state(3), both=True), 'grid_probs'),
    ('n0', dict(n=0), 'n must be in [1, 32]'),
    ('n33', dict(n=33), 'n must be in [1, 32]'),
    ('laps0', dict(laps=0), 'total_laps must be in [1, 1000]'),
    ('laps1001', dict(laps=1001), 'total_laps must be in [1, 1000]'),
    ('deviates53', dict(deviates=53), 'MCGP_DEVIATES_32'),
    ('edges0', dict(edges=()), 'n_edges must be in [1, 63]'),
    ('edges64', dict(edges=tuple(range(1, 65))), 'n_edges must be in [1, 63]'),
    ('edges_null', dict(null=('edges',)), 'edges is NULL'),
    ('edge_nan', dict(edges=(1.0, math.nan)), 'edges[1] is not finite'),
    ('edge_inf', dict(edges=(1.0, math.inf)), 'edges[1] is not finite'),
    ('edge_zero', dict(edges=(0.0, 1.0)), 'edges[0] must be > 0'),
    ('edge_negative', dict(edges=(-1.0, 1.0)), 'edges[0] must be > 0'),
    ('edge_equal', dict(edges=(1.0, 2.0, 2.0)), 'edges[2] must be above edges[1]'),
    ('edge_decreasing', dict(edges=(1.0, 3.0, 2.0)), 'edges[2] must be above edges[1]'),
    ('windows0', dict(windows=()), 'n_windows must be in [1, 64]'),
    ('windows65', dict(windows=tuple((i % 3, 20.0) for i in range(65))), 'n_windows must be in [1, 64]'),
    ('drivers_null', dict(null=('window_drivers',)), 'window_drivers is NULL'),
    ('losses_null', dict(null=('window_losses',)), 'window_losses is NULL'),
    ('driver_index', dict(windows=((0, 21.0), (3, 21.0))), 'window_drivers[1]: driver index must be below n'),
    ('loss_negative', dict(windows=((0, 21.0), (1, -0.5))), 'window_losses[1] must be finite and >= 0'),
    ('loss_nan', dict(windows=((0, math.nan),)), 'window_losses[0] must be finite and >= 0'),
    ('loss_inf', dict(windows=((0, 1.0), (1, 2.0), (2, math.inf))), 'window_losses[2] must be finite and >= 0'),
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
    for kw in (dict(n=1, laps=1), dict(n=32, laps=1000, edges=tuple(range(1, 64))),
               dict(n=2, windows=tuple((i % 2, float(i)) for i in range(64))), dict(windows=((2, 0.0), (2, 0.0), (2, 1e6))),
               dict(state=_state(3, lap=60)), dict(state=_state(3, lap=1))):
        rc, err, bufs = _abi_call(n_sims=0, fill=3, device=999, **kw)
        assert rc == 0, (kw, err)
        assert all((b == 3).all() for b in bufs.values())


def test_outputs_untouched_when_the_device_lookup_fails():
    """A device index no machine has: every argument passes, the device lookup fails, the buffers keep their values."""
    for kw in (dict(), dict(state=_state(4))):
        rc, err, bufs = _abi_call(n=4, device=999, fill=7, **kw)
        assert rc == -2 and 'device' in err
        assert all((b == 7).all() for b in bufs.values())


def test_run_pit_windows_of_nothing_needs_no_device_and_python_checks_its_arguments():
    case = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**case['config']))
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'])
    res = sim.run_pit_windows(0, *args, windows=[('VER', None), ('VER', 11), ('NOR', 0)])
    assert isinstance(res, PitWindowResult) and res.n_simulations == 0 and res.total_laps == 60 and res.first_lap == 1
    assert res.windows == [('VER', float(case['config']['pit_loss'])), ('VER', 11.0), ('NOR', 0.0)]      # None: pit_loss
    assert res.edges == tuple(float(x) for x in DEFAULT_GAP_EDGES) == tuple(float(x) for x in WR.DEFAULT_EDGES)
    assert res.rejoin.shape == res.lost.shape == (60, 3, 21) and res.ahead.shape == (60, 3, 22)
    assert res.gap_ahead.shape == res.gap_behind.shape == (60, 3, 16) and res.hist.shape == (20, 20)
    assert not res.rejoin.any() and sim.last_drivers == list(case['grid_probs']) and not sim.last_histogram.any()
    for kw, msg in ((dict(windows=[('XXX', None)]), 'not among the drivers'), (dict(windows=[('VER', -1)]), 'finite and >= 0'),
                    (dict(windows=[('VER', math.inf)]), 'finite and >= 0'), (dict(windows=[]), '1 to 64'),
                    (dict(windows=[('VER', float(i)) for i in range(65)]), '1 to 64'),
                    (dict(windows=[('VER', None)], edges=[2, 1]), 'increasing'),
                    (dict(windows=[('VER', None)], edges=list(range(1, 65))), 'edges')):
        with pytest.raises(ValueError, match=msg):
            sim.run_pit_windows(10, *args, **kw)
    with pytest.raises(ValueError, match='exactly one'):
        sim.run_pit_windows(10, None, *args[1:], windows=[('VER', None)])
    for doc in (RaceSimulator.run_pit_windows.__doc__, PitWindowResult.__doc__):          # the docstrings say what it is not
        assert 'Nothing is re-simulated' in ' '.join(doc.split())


# ---------------------------------------------------------------- PitWindowResult on hand-made counts
def _hand_result():
    """2 laps, drivers A B C, edges 1 s and 5 s (bins [0, 1), [1, 5), [5, inf)), windows (A, 20) and (A, 2), 4
    simulations.  Window (A, 20) after lap 2:
        sim 0: A leads and rejoins last: behind C by 0.5, nobody behind      sim 1: A second, rejoins second: behind B by 6, C 2 behind
        sim 2: A retired                                                   sim 3: A leads and stays in the lead, B 5 behind (on the edge: up)
    After lap 1 every stop is free and in the lead with B within 1 s behind; window (A, 2) is always free and in the
    lead with B at least 5 s behind."""
    r = PitWindowResult.empty(['A', 'B', 'C'], 2, (1.0, 5.0), [('A', 20.0), ('A', 2.0)], n_simulations=4)
    r.hist[:] = [[2, 1, 1], [1, 2, 1], [1, 1, 2]]
    for w in (0, 1):
        r.rejoin[0, w] = [4, 0, 0, 0]
        r.lost[0, w] = [4, 0, 0, 0]
        r.ahead[0, w] = [0, 0, 0, 4, 0]
        r.gap_ahead[0, w] = [0, 0, 0, 4]
    r.gap_behind[0, 0] = [4, 0, 0, 0]
    r.gap_behind[0, 1] = [0, 0, 4, 0]
    #                  positions 0, 1, 2 | retired
    r.rejoin[1, 0] = [1, 1, 1, 1]
    r.lost[1, 0] = [2, 0, 1, 1]                 # sim 0 loses two places, sims 1 and 3 none
    r.ahead[1, 0] = [0, 1, 1, 1, 1]             # behind B (sim 1), behind C (sim 0), in the lead (sim 3), retired (sim 2)
    r.gap_ahead[1, 0] = [1, 0, 1, 2]            # 0.5 | 6 | none (sim 3) and retired (sim 2)
    r.gap_behind[1, 0] = [0, 1, 1, 2]           # 2 | 5 | none (sim 0) and retired (sim 2)
    r.rejoin[1, 1] = [3, 0, 0, 1]
    r.lost[1, 1] = [3, 0, 0, 1]
    r.ahead[1, 1] = [0, 0, 0, 3, 1]
    r.gap_ahead[1, 1] = [0, 0, 0, 4]
    r.gap_behind[1, 1] = [0, 0, 3, 1]
    return r


def test_result_readers():
    r = _hand_result()
    assert r.position_probabilities()['A'] == {1: 0.5, 2: 0.25, 3: 0.25}
    assert r.running_probability(0).tolist() == [1.0, 0.75]
    third = 1.0 / 3.0
    assert r.rejoin_distribution(0, 1).tolist() == [1.0, 0.0, 0.0]
    assert np.allclose(r.rejoin_distribution(0, 2), [third] * 3)                          # given running: 3 simulations
    assert np.allclose(r.expected_rejoin_position(0), [1.0, 2.0]) and r.expected_rejoin_position(1).tolist() == [1.0, 1.0]
    assert np.allclose(r.places_lost_distribution(0, 2), [2 * third, 0.0, third])
    assert np.allclose(r.free_stop_probability(0), [1.0, 2 * third]) and r.free_stop_probability(1).tolist() == [1.0, 1.0]
    # clear air: gap ahead >= the edge, or no car ahead -- given running
    assert np.allclose(r.clear_air_probability(0, 1.0), [1.0, 2 * third]) and r.clear_air_probability(0, 1.0, lap=2) == \
        pytest.approx(2 * third)
    assert np.allclose(r.clear_air_probability(0, 5.0), [1.0, 2 * third])
    assert np.allclose(r.safe_from_behind_probability(0, 1.0), [0.0, 1.0])
    assert np.allclose(r.safe_from_behind_probability(0, 5.0), [0.0, 2 * third])          # 5 s is on the edge: it counts
    assert r.safe_from_behind_probability(1, 5.0, lap=1) == 1.0
    assert r.rejoins_behind(0, 1) == [(IN_THE_LEAD, 1.0)]
    assert [d for d, _ in r.rejoins_behind(0, 2)] == ['B', 'C', IN_THE_LEAD]                # equal odds: driver order, lead last
    assert r.rejoins_behind(0, 2, k=1) == [('B', pytest.approx(third))]
    assert r.median_rejoin_position(0, 2) == 2 and r.median_rejoin_position(1, 2) == 1
    assert r.open_laps(0) == [1, 2] and r.open_laps(0, p=0.7) == [1] and r.open_laps(1, p=1.0) == [1, 2]
    # a window by index, by (driver, loss), and by the driver alone where that is unambiguous
    assert r.free_stop_probability(('A', 2)).tolist() == [1.0, 1.0]
    s = PitWindowResult.empty(['A', 'B'], 5, (1.0,), [('B', 3.0)], first_lap=3)            # a run from a state after lap 2
    assert s._w('B') == 0 and np.isnan(s.free_stop_probability('B')).all() and s.open_laps('B') == []
    assert s.rejoins_behind('B', 4) == [] and s.median_rejoin_position('B', 3) is None


def test_result_refuses_what_the_counts_cannot_answer():
    r = _hand_result()
    for call in (lambda: r.clear_air_probability(0, 2.0), lambda: r.safe_from_behind_probability(0, 0.999999),
                 lambda: r.clear_air_probability(1, 0.5, lap=1)):
        with pytest.raises(ValueError, match='not one of the edges'):
            call()
    for call in (lambda: r.rejoin_distribution(2, 1), lambda: r.rejoin_distribution(-1, 1), lambda: r.free_stop_probability('A'),
                 lambda: r.free_stop_probability('B'), lambda: r.free_stop_probability(('A', 3.0)),
                 lambda: r.rejoin_distribution(0, 3), lambda: r.places_lost_distribution(0, 0),
                 lambda: r.rejoins_behind(0, 9)):
        with pytest.raises(ValueError):
            call()
    s = PitWindowResult.empty(['A', 'B'], 5, (1.0,), [('B', 3.0)], first_lap=3)
    with pytest.raises(ValueError, match=r'\[3, 5\]'):
        s.rejoin_distribution(0, 2)


def test_pit_window_keys_are_json_safe():
    keys = P.pit_window_keys(_hand_result(), clear_air_seconds=2.0)
    json.dumps(keys, allow_nan=False)
    assert keys['edges'] == [1.0, 5.0] and keys['clear_air_seconds'] == 1.0 and keys['first_lap'] == 1      # 1 is nearer 2 than 5
    w = keys['windows'][0]
    assert (w['driver'], w['loss']) == ('A', 20.0) and w['running'] == [1.0, 0.75]
    assert w['median_rejoin_position'] == [1, 2] and w['likeliest_ahead'][0] == [IN_THE_LEAD, 1.0]
    assert w['free_stop'][1] == pytest.approx(2 / 3) and w['open_laps'] == [1, 2]
    s = P.pit_window_keys(PitWindowResult.empty(['A', 'B'], 3, (1.0,), [('B', 3.0)], first_lap=3))
    json.dumps(s, allow_nan=False)
    assert s['windows'][0]['free_stop'] == [None] * 3 and s['windows'][0]['likeliest_ahead'] == [None] * 3
    assert P.pit_window_options([('A', None), ('A', 21.0), ('B', 5)], 21.0) == {'windows': [('A', 21.0), ('B', 5.0)]}
    assert P.pit_window_options({'windows': [('A', 1)], 'edges': [1, 2]}, 21.0) == {'windows': [('A', 1.0)], 'edges': [1.0, 2.0]}
    with pytest.raises(ValueError):
        P.pit_window_options({'window': []}, 21.0)


# ---------------------------------------------------------------- the command
class _FakePredictor:
    """predict_weekend's / predict_from_state's result shape from hand-made counts (no device)."""
    calls = []

    def __init__(self, device=0):
        pass

    def _block(self, drivers, pit_window, first_lap=1):
        opt = P.pit_window_options(pit_window, 21.0)
        r = PitWindowResult.empty(drivers, 6, opt.get('edges', DEFAULT_GAP_EDGES), opt['windows'], n_simulations=4,
                                  first_lap=first_lap)
        k = first_lap - 1
        r.rejoin[k:, :, 2] = 3
        r.rejoin[k:, :, -1] = 1
        r.lost[k:, :, 0] = 3
        r.lost[k:, :, -1] = 1
        r.ahead[k:, :, 1] = 3
        r.ahead[k:, :, -1] = 1
        r.gap_ahead[k:, :, 0] = 3
        r.gap_ahead[k:, :, -1] = 1
        r.gap_behind[k:, :, -1] = 4
        return P.pit_window_keys(r, 2.0)

    def predict_weekend(self, season, race, fixture, n_simulations=0, seed=None, **kw):
        _FakePredictor.calls.append(('weekend', kw))
        drivers = list(fixture['drivers'])
        n = len(drivers)
        res = P.pack_result(drivers, {d: [1.0 / n] * n for d in drivers}, {d: {1 + i: 1.0} for i, d in enumerate(drivers)},
                            {}, 'fp2', None)
        res['pit_window'] = self._block(drivers, kw['pit_window'])
        return res

    def predict_from_state(self, season, race, fixture, state, n_simulations=0, seed=None, **kw):
        _FakePredictor.calls.append(('state', kw))
        drivers = list(fixture['drivers'])
        return {'lap': state.lap, 'win_probabilities': {d: float(i == 0) for i, d in enumerate(drivers)},
                'podium_probabilities': {}, 'points_probabilities': {}, 'full_distributions': {},
                'pit_window': self._block(drivers, kw['pit_window'], state.lap + 1)}


def test_the_module_keeps_the_strategy_helper_of_its_name_callable():
    """monte_carlo_gp_amd.pit_window is the package's strategy helper; importing the command's module rebinds the
    attribute to the module, which answers a call as the helper does."""
    cmd = _command()
    want = strategy_windows('VER', range(18, 21), 'HARD', then=[(45, 'SOFT')], start='MEDIUM')
    assert monte_carlo_gp_amd.pit_window('VER', range(18, 21), 'HARD', then=[(45, 'SOFT')], start='MEDIUM') == want
    assert cmd('VER', range(18, 21), 'HARD', then=[(45, 'SOFT')], start='MEDIUM') == want and list(want) == [
        'VER L18', 'VER L19', 'VER L20']


def test_command_parsing_and_the_window_limit():
    cmd = _command()
    parse = lambda *a: cmd.build_parser().parse_args(['--race', 'Bahrain'] + list(a))
    args = parse('--driver', 'NOR', '--driver', 'VER', '--loss', '11', '--loss', '15.5', '--laps', '25-45', '--seed', '7')
    assert (args.season, args.simulations, args.seed, args.state, args.json) == (2025, 100000, 7, None, None)
    assert cmd.windows_argument(args) == [('NOR', None), ('NOR', 11.0), ('NOR', 15.5), ('VER', None), ('VER', 11.0),
                                          ('VER', 15.5)]
    assert cmd.windows_argument(parse('--driver', 'NOR', '--driver', 'NOR', '--loss', '3', '--loss', '3')) == [
        ('NOR', None), ('NOR', 3.0)]
    names = [f'D{i:02d}' for i in range(33)]
    flags = lambda ds: [x for d in ds for x in ('--driver', d)]
    assert len(cmd.windows_argument(parse(*flags(names[:32]), '--loss', '11'))) == 64          # 32 x 2: the limit itself
    assert len(cmd.windows_argument(parse('--driver', 'NOR', *[x for i in range(63) for x in ('--loss', str(i))]))) == 64
    for bad in (flags(names[:33]) + ['--loss', '11'], flags(names[:22]) + ['--loss', '1', '--loss', '2'],
                ['--driver', 'NOR'] + [x for i in range(64) for x in ('--loss', str(i))]):
        with pytest.raises(SystemExit, match='windows'):
            cmd.windows_argument(parse(*bad))
    for bad in (['--loss', '-1'], ['--loss', 'nan'], ['--loss', 'inf']):
        with pytest.raises(SystemExit, match='--loss'):
            cmd.windows_argument(parse('--driver', 'NOR', *bad))
    with pytest.raises(SystemExit):
        parse()                                                                               # --driver is required
    assert cmd.laps_argument(None, 31, 57) == list(range(31, 58)) and cmd.laps_argument('25-33', 31, 57) == [31, 32, 33]
    assert cmd.laps_argument('40', 1, 57) == [40] and cmd.laps_argument('58-60', 1, 57) == []
    for bad in ('x', '3-', '9-4', '1-2-3'):
        with pytest.raises(SystemExit, match='--laps'):
            cmd.laps_argument(bad, 1, 57)


def test_command_end_to_end_on_hand_made_counts(tmp_path, capsys, monkeypatch):
    cmd = _command()
    monkeypatch.setattr(cmd, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    drivers = list(cli.synthetic_fixture()['drivers'])
    a, b = drivers[0], drivers[1]
    out_json = tmp_path / 'w.json'
    base = ['--race', 'Bahrain', '--season', '2024', '--offline', '--simulations', '20', '--seed', '1']
    assert cmd.main(base + ['--driver', a, '--loss', '11', '--laps', '2-3', '--gap-edges', '0.8,1.9,4', '--json', str(out_json)]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [('weekend', {'pit_window': {'windows': [(a, None), (a, 11.0)], 'edges': [0.8, 1.9, 4.0]}})]
    assert f'PIT WINDOW: {a} losing 21 s' in out and f'PIT WINDOW: {a} losing 11 s' in out and 'nothing is re-simulated' in out
    assert 'clear air >= 1.9 s' in out                                # the edge nearest to the model's 2 s
    assert '100.0%' in out and f'{drivers[1]} (100%)' in out and out.count('\n   2 ') == 2 and '\n   4 ' not in out
    assert 'laps with P(free stop) >= 50%: 1, 2, 3, 4, 5, 6' in out
    saved = json.loads(out_json.read_text())
    assert saved['pit_window']['windows'][1]['loss'] == 11.0 and 'full_distributions' not in saved
    assert saved['pit_window']['windows'][0]['median_rejoin_position'] == [3] * 6
    # from a state: the laps after it
    state = {'lap': 4, 'drs_disabled_until': 0, 'cars': [
        {'driver': d, 'cumulative_time': 360.0 + i, 'last_lap_time': 90.0, 'tire_compound': 'SOFT', 'tire_age': 4,
         'used_compounds': ['SOFT'], 'retired_lap': 0} for i, d in enumerate(drivers)]}
    path = tmp_path / 'state.json'
    path.write_text(json.dumps(state))
    assert cmd.main(base + ['--state', str(path), '--driver', a, '--driver', b, '--json', str(out_json)]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls[1] == ('state', {'pit_window': {'windows': [(a, None), (b, None)]}})
    assert 'after lap 4' in out and '\n   5 ' in out and '\n   4 ' not in out
    assert json.loads(out_json.read_text())['state'] == str(path)
    for bad in (['--driver', a, '--laps', 'x'], ['--driver', a, '--gap-edges', '1,x']):
        with pytest.raises(SystemExit):
            cmd.main(base + bad)
    assert len(_FakePredictor.calls) == 2                             # both refused before any run


def test_cli_main_has_no_pit_window_argument(capsys):
    """The command adds nothing to cli.main's parser (tests/test_cli_transcripts.py pins it option by option)."""
    with pytest.raises(SystemExit):
        cli.main(['pit-window', '--race', 'Bahrain'])
    assert 'invalid choice' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(['predict', '--race', 'Bahrain', '--offline', '--pit-window', 'NOR'])
    assert 'unrecognized arguments' in capsys.readouterr().err


# ---------------------------------------------------------------- the reference
def test_the_reference_on_a_hand_made_race():
    """Three cars, one lap row each: the rejoin key among the others' keys, ties by grid slot, a retired car."""
    #                 lap 1: A 10, B 12, C 15      lap 2: A 20, B 20 (a tie: slot decides), C retired
    cum = np.array([[[10.0, 12.0, 15.0], [20.0, 20.0, 31.0]]])
    dnf = np.array([[[0, 0, 0], [0, 0, 2]]])
    slot = np.array([[1, 0, 2]])                         # B started ahead of A
    edges = (1.0, 5.0)
    v = WR.values_from_times(cum, dnf, slot, [(0, 2.0), (0, 0.0), (1, 0.0), (2, 1e6), (0, 5.0)], edges)
    # lap 1, (A, 2): t* = 12 ties with B, B's slot 0 < A's slot 1 -> B ahead: rejoins 1, lost 1, behind B by 0, C 3 behind
    assert v[0, 0, 0].tolist() == [1, 1, 1, 0, 1]
    assert v[0, 0, 1].tolist() == [0, 0, 3, 3, 1]        # (A, 0): in the lead, no car ahead, B 2 behind
    assert v[0, 0, 2].tolist() == [1, 0, 0, 1, 1]        # (B, 0): second as it is, A 2 ahead, C 3 behind
    assert v[0, 0, 3].tolist() == [2, 0, 1, 2, 3]        # (C, 1e6): last as it is, behind B, nobody behind
    assert v[0, 0, 4].tolist() == [1, 1, 1, 1, 0]        # (A, 5): t* = 15 ties with C, A's slot 1 < C's 2 -> C behind, by 0
    # lap 2: A and B tie at 20; B (slot 0) leads.  (A, 0): B ahead (tie, slot), rejoin 1, lost 0, gap 0; C is out
    assert v[0, 1, 1].tolist() == [1, 0, 1, 0, 3]
    assert v[0, 1, 2].tolist() == [0, 0, 3, 3, 0]        # (B, 0): leads, A right behind at 0
    assert v[0, 1, 3].tolist() == [3, 3, 4, 3, 3]        # C retired
    c = WR.counts_from_values(v, 3, len(edges))
    assert all((c[k].sum(axis=2) == 1).all() for k in WR.ROWS)
    assert WR.tie_cells(cum, dnf, 0.0) == 2 and WR.tie_cells(cum, dnf, 2.0, [0]) == 1 and WR.tie_cells(cum, dnf, 5.0) == 1
    assert WR.tie_cells(cum, dnf, 11.0) == 0             # (A + 11 = 31 is the retired C's frozen time: no cell)
