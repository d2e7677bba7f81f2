"""Race time gaps, host side: the C-ABI argument checks of mcgp_run_gaps (no device needed), the binding against the
header, GapResult's readers on hand-made counts, the CLI flags, and the two references of the GPU tests pinned to each
other: the numpy restatement over the oracle's trace (gaps_ref.gap_counts) and the wrapped Python restatement
(gaps_ref.restated_times)."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import gaps_ref as GR
import oracle_py as O
import resume_ref as RR
from monte_carlo_gp_amd import DEFAULT_GAP_EDGES, GapResult, RaceConfig, RaceSimulator, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import predictor as P
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, _Problem

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mcgp.h')


# ---------------------------------------------------------------- the C ABI without a device
def _state(n, lap=10, **over):
    a = dict(cumulative_time=np.arange(n, dtype=np.float64) + 900.0, last_lap_time=np.full(n, 90.0),
             grid_slot=np.arange(n, dtype=np.uint8), compound=np.zeros(n, np.uint8), used_compounds=np.ones(n, np.uint8),
             tire_age=np.full(n, 5, np.int16), retired_lap=np.zeros(n, np.int16))
    a.update(over)
    return a, lap, 0


def _abi_call(n=3, n_sims=100, device=0, deviates=32, laps=60, fill=0, null=(), edges=(1.0, 5.0), pairs=((0, 1),),
              state=None, both=False, n_edges=None, n_pairs=None, force_pair_out=False):
    lib = N.lib()
    c = O.load_case('S60')
    m = max(n, 1)
    prob = _Problem(RaceConfig(**dict(c['config'], total_laps=laps)), [f'D{i:02d}' for i in range(m)], {}, {}, {}, None,
                    'dry', DEFAULT_SET_POP, deviates)
    prob.cfg.total_laps = laps          # (RaceConfig does not check it: the library does)
    g = np.full((m, m), 1.0 / m)
    e = np.ascontiguousarray(edges, np.float64)
    pr = np.ascontiguousarray(np.asarray(pairs, np.uint8).reshape(-1, 2))
    cs = RR.c_state(*state) if state is not None else None
    bufs = {k: np.full(1 << 16, fill, np.uint64) for k in ('hist', 'lap_gap', 'lead', 'pair')}
    if not len(pr) and not force_pair_out:
        null = tuple(null) + ('pair',)              # pair_out goes with the pairs
    ptr = lambda k: None if k in null else bufs[k].ctypes.data_as(C.POINTER(C.c_uint64))
    use_grid = (state is None or both) and 'grid_probs' not in null
    rc = lib.mcgp_run_gaps(C.byref(prob.cfg), C.byref(prob.drv),
                           g.ctypes.data_as(C.POINTER(C.c_double)) if use_grid else None,
                           C.byref(cs) if cs is not None else None, n, len(e) if n_edges is None else n_edges,
                           None if 'edges' in null else e.ctypes.data_as(C.POINTER(C.c_double)),
                           len(pr) if n_pairs is None else n_pairs,
                           None if 'pairs' in null or not len(pr) else pr.ctypes.data_as(C.POINTER(C.c_uint8)),
                           n_sims, 0, 1, device, ptr('hist'), ptr('lap_gap'), ptr('lead'), ptr('pair'))
    return rc, lib.mcgp_last_error().decode(), bufs


def test_binding_matches_the_header():
    L = N.lib()
    assert L.mcgp_abi_version() == N.ABI_VERSION == 6                 # an added entry point only: a caller tests for the symbol
    assert 'mcgp_run_gaps' in N.EXPORTS and hasattr(L, 'mcgp_run_gaps')
    with open(HEADER) as f:
        text = f.read()
    consts = dict(re.findall(r'#define (MCGP_MAX_GAP_\w+) (\d+)', text))
    assert consts == {'MCGP_MAX_GAP_EDGES': str(N.MAX_GAP_EDGES), 'MCGP_MAX_GAP_PAIRS': str(N.MAX_GAP_PAIRS)}
    assert (N.MAX_GAP_EDGES, N.MAX_GAP_PAIRS) == (63, 64)
    decl = re.search(r'int32_t mcgp_run_gaps\((.*?)\);', text, re.S).group(1)
    params = [' '.join(p.split()) for p in decl.split(',')]
    ctype = {'const mcgp_config *': C.POINTER(N.McgpConfig), 'const mcgp_drivers *': C.POINTER(N.McgpDrivers),
             'const double *': C.POINTER(C.c_double), 'const mcgp_race_state *': C.POINTER(N.McgpRaceState),
             'uint32_t ': C.c_uint32, 'uint64_t ': C.c_uint64, 'int32_t ': C.c_int32,
             'const uint8_t *': C.POINTER(C.c_uint8), 'uint64_t *': C.POINTER(C.c_uint64)}
    want = [ctype[re.match(r'(.*?[ *])\w+$', p).group(1)] for p in params]
    assert len(want) == 17 and L.mcgp_run_gaps.argtypes == want == N.GAPS_ARGTYPES
    assert L.mcgp_run_gaps.restype is C.c_int32
    assert [p.split()[-1].lstrip('*') for p in params][-4:] == ['hist_out', 'lap_gap_out', 'lead_out', 'pair_out']


_BAD = [
    ('hist', dict(null=('hist',)), 'hist_out'),
    ('lap_gap', dict(null=('lap_gap',)), 'lap_gap_out'),
    ('neither', dict(null=('grid_probs',)), 'grid_probs'),
    ('both', dict(state=_state(3), both=True), 'grid_probs'),
    ('n0', dict(n=0, pairs=()), 'n must be in [1, 32]'),
    ('n33', dict(n=33, pairs=()), 'n must be in [1, 32]'),
    ('laps0', dict(laps=0), 'total_laps must be in [1, 1000]'),
    ('laps1001', dict(laps=1001), 'total_laps must be in [1, 1000]'),
    ('deviates53', dict(deviates=53), 'MCGP_DEVIATES_32'),
    ('edges0', dict(edges=(), pairs=()), 'n_edges'),
    ('edges64', dict(edges=tuple(range(1, 65)), pairs=()), 'n_edges'),
    ('edges_null', dict(null=('edges',)), 'edges'),
    ('edge_nan', dict(edges=(1.0, math.nan)), 'edges[1]'),
    ('edge_inf', dict(edges=(1.0, math.inf)), 'edges[1]'),
    ('edge_zero', dict(edges=(0.0, 1.0)), 'edges[0]'),
    ('edge_negative', dict(edges=(-1.0, 1.0)), 'edges[0]'),
    ('edge_equal', dict(edges=(1.0, 2.0, 2.0)), 'edges[2]'),
    ('edge_decreasing', dict(edges=(1.0, 3.0, 2.0)), 'edges[2]'),
    ('pairs65', dict(n=4, pairs=tuple((0, 1) for _ in range(65))), 'n_pairs'),
    ('pair_index', dict(pairs=((0, 1), (1, 3))), 'pairs[1]'),
    ('pair_same', dict(pairs=((2, 2),)), 'pairs[0]'),
    ('pairs_null', dict(null=('pairs',), n_pairs=1), 'pairs is NULL'),
    ('pair_out_null', dict(null=('pair',)), 'pair_out'),
    ('pair_out_given', dict(pairs=(), force_pair_out=True), 'pair_out'),
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
    for kw in (dict(n=1, laps=1, pairs=()), dict(n=32, laps=1000, edges=tuple(range(1, 64))),
               dict(n=2, pairs=tuple((i % 2, 1 - i % 2) for i in range(64))),
               dict(n=3, null=('lead',), pairs=()), dict(state=_state(3, lap=60)), dict(state=_state(3, lap=1))):
        rc, err, bufs = _abi_call(n_sims=0, fill=3, device=999, **kw)
        assert rc == 0, (kw, err)
        assert all((b == 3).all() for b in bufs.values())


def test_outputs_untouched_when_the_device_lookup_fails():
    """A device index no machine has: every argument passes, the device lookup fails, the buffers keep their values."""
    for kw in (dict(), dict(state=_state(4))):
        rc, err, bufs = _abi_call(n=4, device=999, fill=7, **kw)
        assert rc == -2 and 'device' in err
        assert all((b == 7).all() for b in bufs.values())


def test_run_gaps_of_nothing_needs_no_device_and_python_checks_its_arguments():
    case = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**case['config']))
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'])
    res = sim.run_gaps(0, *args, pairs=[('VER', 'NOR')])
    assert isinstance(res, GapResult) and res.n_simulations == 0 and res.total_laps == 60 and res.first_lap == 1
    assert res.edges == tuple(float(x) for x in DEFAULT_GAP_EDGES) == tuple(float(x) for x in GR.DEFAULT_EDGES)
    assert res.lap_gap.shape == (60, 20, 16) and res.lead.shape == (60, 16) and res.pair.shape == (60, 1, 31)
    assert not res.lap_gap.any() and sim.last_drivers == list(case['grid_probs']) and not sim.last_histogram.any()
    for kw, msg in ((dict(pairs=[('VER', 'XXX')]), 'not among the drivers'), (dict(pairs=[('VER', 'VER')]), 'different'),
                    (dict(edges=[2, 1]), 'increasing'), (dict(edges=[0, 1]), 'positive'), (dict(edges=[]), 'edges'),
                    (dict(edges=list(range(1, 65))), 'edges'), (dict(pairs=[('VER', 'NOR')] * 65), 'at most 64')):
        with pytest.raises(ValueError, match=msg):
            sim.run_gaps(10, *args, **kw)
    with pytest.raises(ValueError, match='exactly one'):
        sim.run_gaps(10, None, *args[1:])


# ---------------------------------------------------------------- GapResult on hand-made counts
def _hand_result():
    """2 laps, drivers A B C, edges 1 s and 5 s (bins [0, 1), [1, 5), [5, inf)), pairs (A, B) and (C, A), 4 simulations.
    After lap 2:  sim 0: A leads, B +0.4, C +6     sim 1: B leads, A +2, C retired
                  sim 2: A leads, B +1 (on the edge: up), C +3     sim 3: C alone (A and B retired)
    After lap 1 everybody runs within 1 s behind A."""
    r = GapResult.empty(['A', 'B', 'C'], 2, (1.0, 5.0), [('A', 'B'), ('C', 'A')], n_simulations=4)
    r.hist[:] = [[2, 1, 1], [1, 2, 1], [1, 1, 2]]
    r.lap_gap[0] = [[4, 0, 0, 0]] * 3
    r.lead[0] = [4, 0, 0, 0]
    r.pair[0] = [[4, 0, 0, 0, 0, 0, 0], [0, 0, 0, 4, 0, 0, 0]]
    r.lap_gap[1] = [[2, 1, 0, 1], [2, 1, 0, 1], [1, 1, 1, 1]]
    r.lead[1] = [1, 2, 0, 1]
    #           (A, B): a ahead 0.4, 1 | b ahead 2 | out          (C, A): a (= C) never ahead; A ahead by 6 and 3; out twice
    r.pair[1] = [[1, 1, 0, 0, 1, 0, 1], [0, 0, 0, 0, 1, 1, 2]]
    return r


def test_result_readers():
    r = _hand_result()
    assert r.n_bins == 3 and r.bin_bounds(0) == (0.0, 1.0) and r.bin_bounds(2) == (5.0, math.inf)
    assert r.position_probabilities['A'] == {1: 0.5, 2: 0.25, 3: 0.25}
    assert r.gap_distribution('A').tolist() == [0.5, 0.25, 0.0, 0.25]
    assert r.gap_distribution('C', lap=1).tolist() == [1.0, 0.0, 0.0, 0.0]
    assert set(r.finishing_gap_distributions) == {'A', 'B', 'C'}
    assert r.within('B', 1.0) == 0.5 and r.within('B', 5.0) == 0.75 and r.within('C', 5, lap=1) == 1.0
    assert r.winning_margin_distribution.tolist() == [0.25, 0.5, 0.0, 0.25]
    assert r.winning_margin_under(5.0) == 0.75 and r.winning_margin_under(1) == 0.25
    assert r.lead_by_lap.shape == (2, 4) and r.lead_by_lap[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert r.median_gap_bin_by_lap('A') == [(0.0, 1.0), (0.0, 1.0)]           # running 3 times: bins 0, 0, 1
    assert r.median_gap_bin_by_lap('C') == [(0.0, 1.0), (1.0, 5.0)]           # running 3 times: bins 0, 1, 2
    assert r.pair_summary('A', 'B') == {'a_ahead': 0.5, 'b_ahead': 0.25, 'either_out': 0.25}
    assert r.pair_summary('B', 'A') == {'a_ahead': 0.25, 'b_ahead': 0.5, 'either_out': 0.25}      # the mirror image
    assert r.pair_summary('C', 'A') == {'a_ahead': 0.0, 'b_ahead': 0.5, 'either_out': 0.5}
    assert r.pair_summary('C', 'A', lap=1) == {'a_ahead': 0.0, 'b_ahead': 1.0, 'either_out': 0.0}
    assert r.pair_within_by_lap('A', 'B', 1.0).tolist() == [1.0, 0.25]
    assert r.pair_within_by_lap('A', 'B', 5.0).tolist() == [1.0, 0.75]


def test_result_refuses_what_the_counts_cannot_answer():
    r = _hand_result()
    for call in (lambda: r.within('A', 2.0), lambda: r.within('A', 0.999999), lambda: r.winning_margin_under(3),
                 lambda: r.pair_within_by_lap('A', 'B', 4.0), lambda: r.within('A', 0.5, lap=1)):
        with pytest.raises(ValueError, match='not one of the edges'):
            call()
    for call in (lambda: r.within('X', 1.0), lambda: r.gap_distribution('A', lap=3), lambda: r.gap_distribution('A', lap=0),
                 lambda: r.pair_summary('B', 'C'), lambda: r.bin_bounds(3)):
        with pytest.raises(ValueError):
            call()
    s = GapResult.empty(['A', 'B'], 5, (1.0,), first_lap=3)           # a run from a state after lap 2
    with pytest.raises(ValueError, match=r'\[3, 5\]'):
        s.within('A', 1.0, lap=2)
    assert s.median_gap_bin_by_lap('A') == [None] * 5


def test_gap_keys_are_json_safe():
    keys = P.gap_keys(_hand_result())
    json.dumps(keys)
    assert keys['edges'] == [1.0, 5.0] and keys['winning_margin'] == [0.25, 0.5, 0.0, 0.25]
    assert keys['within_at_flag']['B'] == {'1.0': 0.5, '5.0': 0.75}
    assert keys['pairs'][0]['a'] == 'A' and keys['pairs'][0]['within_by_lap']['5.0'] == [1.0, 0.75]
    assert P.gap_options(True) == {} and P.gap_options({'edges': [1, 2], 'pairs': [('A', 'B')]}) == {
        'edges': [1.0, 2.0], 'pairs': [('A', 'B')]}
    with pytest.raises(ValueError):
        P.gap_options({'edge': [1]})


# ---------------------------------------------------------------- the CLI flags
class _FakePredictor:
    """predict_weekend's / predict_from_state's result shape from hand-made counts (no device)."""
    calls = []

    def __init__(self, device=0):
        pass

    def _gaps(self, drivers, gaps):
        opt = P.gap_options(gaps)
        edges = opt.get('edges', DEFAULT_GAP_EDGES)
        r = GapResult.empty(drivers, 3, edges, opt.get('pairs', ()), n_simulations=4)
        r.lap_gap[2, :, 1] = 4
        r.lap_gap[2, 0] = 0
        r.lap_gap[2, 0, 0] = 4
        r.lead[2, 1] = 3
        r.lead[2, -1] = 1
        if len(r.pairs):
            r.pair[2, :, 0] = 3
            r.pair[2, :, -1] = 1
        return P.gap_keys(r)

    def predict_weekend(self, season, race, fixture, prediction_point='fp2', n_simulations=0, seed=None, matchups=False,
                        **kw):
        _FakePredictor.calls.append(kw)
        drivers = list(fixture['drivers'])
        n = len(drivers)
        res = P.pack_result(drivers, {d: [1.0 / n] * n for d in drivers}, {d: {1 + i: 1.0} for i, d in enumerate(drivers)},
                            {}, prediction_point, None)
        if kw.get('gaps'):
            res['gaps'] = self._gaps(drivers, kw['gaps'])
        return res

    def predict_from_state(self, season, race, fixture, states, n_simulations=0, seed=None, **kw):
        _FakePredictor.calls.append(kw)
        drivers = list(fixture['drivers'])
        out = []
        for st in states:
            r = {'lap': st.lap, 'win_probabilities': {d: float(i == 0) for i, d in enumerate(drivers)},
                 'podium_probabilities': {d: float(i < 3) for i, d in enumerate(drivers)}, 'points_probabilities': {},
                 'full_distributions': {}}
            if kw.get('gaps'):
                r['gaps'] = self._gaps(drivers, kw['gaps'])
            out.append(r)
        return out


def test_predict_gaps_flags(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    plain, extra = tmp_path / 'plain.json', tmp_path / 'gaps.json'
    base = ['predict', '--race', 'Bahrain', '--offline', '--simulations', '20', '--seed', '1']
    assert cli.main(base + ['--json', str(plain)]) == 0
    out_plain = capsys.readouterr().out
    assert 'WINNING MARGIN' not in out_plain
    assert cli.main(base + ['--gaps']) == 0
    out_default = capsys.readouterr().out
    assert '< 1 s' in out_default and '< 5 s' in out_default and '< 20 s' in out_default and 'PAIR GAPS' not in out_default
    drivers = list(cli.synthetic_fixture()['drivers'])
    a, b = drivers[0], drivers[1]
    assert cli.main(base + ['--gaps', '--gap-edges', '0.8,4,30', '--gap-pair', f'{a}:{b}', '--gap-pair', f'{b} : {a}',
                            '--json', str(extra)]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [{}, {'gaps': True},
                                    {'gaps': {'edges': [0.8, 4.0, 30.0], 'pairs': [(a, b), (b, a)]}}]
    for title in ('WINNING MARGIN', 'WITHIN OF THE WINNER AT THE FLAG', 'PAIR GAPS AT THE FLAG'):
        assert title in out, title
    assert out.index('PODIUM PROBABILITIES') < out.index('WINNING MARGIN')
    assert '< 0.8 s' in out and '< 4 s' in out and '< 30 s' in out             # the nearest edges to 1, 5 and 20 s
    assert '75.0%' in out and 'fewer than two finish' in out and f'{a:4} ahead  75.0%' in out
    pa, pb = json.loads(plain.read_text()), json.loads(extra.read_text())
    assert 'gaps' not in pa and set(pb) == set(pa) | {'gaps'} and {k: pb[k] for k in pa} == pa
    assert pb['gaps']['edges'] == [0.8, 4.0, 30.0] and pb['gaps']['winning_margin'] == [0.0, 0.75, 0.0, 0.0, 0.25]
    for bad in (['--gap-edges', '1,x'], ['--gap-pair', 'VER'], ['--gap-pair', ':NOR']):
        with pytest.raises(SystemExit):
            cli.main(base + ['--gaps'] + bad)


def test_in_race_gaps_flags(tmp_path, capsys, monkeypatch):
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
    assert 'WINNING MARGIN' not in capsys.readouterr().out
    assert cli.main(base + ['--gaps', '--gap-pair', f'{drivers[0]}:{drivers[1]}', '--json', str(tmp_path / 'o.json')]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [{}, {'gaps': {'pairs': [(drivers[0], drivers[1])]}}]
    assert 'WINNING MARGIN' in out and 'PAIR GAPS AT THE FLAG' in out and '< 20 s' in out
    assert json.loads((tmp_path / 'o.json').read_text())[0]['gaps']['edges'] == [float(x) for x in DEFAULT_GAP_EDGES]


# ---------------------------------------------------------------- the references
def test_bin_rule_of_the_reference():
    e = (0.5, 1.0, 2.0)
    x = np.array([0.0, 0.49999, 0.5, np.nextafter(0.5, 0), 1.0, 1.5, 2.0, 1e9])
    assert GR.bin_of(x, e).tolist() == [0, 0, 1, 0, 2, 2, 3, 3]           # a value equal to an edge goes up


@pytest.mark.parametrize('name', ['S60', 'EVT', 'N10'])
def test_the_two_references_agree(name):
    """The wrapped restatement (the reference for many simulations from one state) against the oracle's trace: the times
    of the running cars after every lap are the oracle's bit for bit, so are the retirements and the finishing orders;
    hence so are the counts.  12 simulations, every lap; then from a mid-race state of one of them."""
    case = O.load_case(name)
    m, seed, L = 12, 42, case['config']['total_laps']
    ref = RR.traced_run(case, m, seed)
    tr = ref['trace']
    cum, dnf, slot, orders = GR.restated_times(case, m, seed, grids=ref['grids'])
    running = tr['dnf'] == 0
    assert ((dnf == 0) == running).all() and (orders == ref['orders']).all() and (slot == GR.slots_of(ref['grids'])).all()
    assert (cum[running].view(np.uint64) == tr['cum'][running].view(np.uint64)).all()         # 0 cells differ
    pairs = [(0, 1), (1, 0), (2, 5)]
    a = GR.gap_counts(case, m, seed, pairs=pairs, ref=ref)
    b = GR.counts_from_times(cum, dnf, slot, pairs=pairs)
    assert all((a[k] == b[k]).all() for k in ('lap_gap', 'lead', 'pair'))
    assert (a['lap_gap'].sum(axis=2) == m).all() and (a['lead'].sum(axis=1) == m).all() and (a['pair'].sum(axis=2) == m).all()
    # from the state of simulation 3 after lap L // 2, continued as simulation 3: the oracle trace's later laps
    i, k = 3, L // 2
    st = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, i, k))
    c = GR.restated_counts(case, 1, seed, sim_offset=i, state=st, pairs=pairs)
    d = GR.continued_counts(ref, [i], k, pairs=pairs)
    assert all((c[key] == d[key]).all() for key in ('hist', 'lap_gap', 'lead', 'pair'))
    assert not c['lap_gap'][:k].any() and (c['lap_gap'][k:].sum(axis=2) == 1).all()
