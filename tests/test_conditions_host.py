"""Combination and conditional odds, host side: the C-ABI argument checks of mcgp_run_conditions (no device needed), the
binding and the structs against the header, the condition parser (every subject, operator, shorthand and error),
ConditionResult's arithmetic on hand-made counts, the predictor's and the CLI's plumbing with fakes, and the reference's
own evaluation on a hand-made table of facts."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import conditions_ref as CR
import oracle_py as O
import resume_ref as RR
from monte_carlo_gp_amd import Condition, ConditionResult, RaceConfig, RaceSimulator, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import conditions as CD
from monte_carlo_gp_amd import predictor as P
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, _Problem

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mcgp.h')
HI, LO = CD.INT_MAX, CD.INT_MIN
WIN0 = [(CR.POSITION, 0, 0, 1, 1, 0)]


# ---------------------------------------------------------------- the C ABI without a device
def _state(n, lap=10, **over):
    a = dict(cumulative_time=np.arange(n, dtype=np.float64) + 900.0, last_lap_time=np.full(n, 90.0),
             grid_slot=np.arange(n, dtype=np.uint8), compound=np.zeros(n, np.uint8), used_compounds=np.ones(n, np.uint8),
             tire_age=np.full(n, 5, np.int16), retired_lap=np.zeros(n, np.int16))
    a.update(over)
    return a, lap, 0


def _abi_call(n=3, n_sims=100, device=0, deviates=32, laps=60, fill=0, null=(), conds=(WIN0,), state=None, both=False,
              n_conditions=None, n_atoms=None):
    lib = N.lib()
    c = O.load_case('S60')
    m = max(n, 1)
    prob = _Problem(RaceConfig(**dict(c['config'], total_laps=laps)), [f'D{i:02d}' for i in range(m)], {}, {}, {}, None,
                    'dry', DEFAULT_SET_POP, deviates)
    prob.cfg.total_laps = laps          # (RaceConfig does not check it: the library does)
    g = np.full((m, m), 1.0 / m)
    table = CR.c_conditions(list(conds))
    if n_atoms is not None:
        table[n_atoms[0]].n_atoms = n_atoms[1]
    cs = RR.c_state(*state) if state is not None else None
    bufs = {k: np.full(1 << 17, fill, np.uint64) for k in ('hist', 'count', 'cond_hist')}
    ptr = lambda k: None if k in null else bufs[k].ctypes.data_as(C.POINTER(C.c_uint64))
    use_grid = (state is None or both) and 'grid_probs' not in null
    rc = lib.mcgp_run_conditions(C.byref(prob.cfg), C.byref(prob.drv),
                                 g.ctypes.data_as(C.POINTER(C.c_double)) if use_grid else None,
                                 C.byref(cs) if cs is not None else None, n,
                                 len(conds) if n_conditions is None else n_conditions,
                                 None if 'conditions' in null else table, n_sims, 0, 1, device, ptr('hist'), ptr('count'),
                                 ptr('cond_hist'))
    return rc, lib.mcgp_last_error().decode(), bufs


def _fields(struct):
    return [(f, getattr(struct, f).offset, getattr(struct, f).size) for f, _ in struct._fields_]


def test_binding_and_structs_match_the_header():
    L = N.lib()
    assert L.mcgp_abi_version() == N.ABI_VERSION == 6                 # an added entry point only: a caller tests for the symbol
    assert 'mcgp_run_conditions' in N.EXPORTS and hasattr(L, 'mcgp_run_conditions')
    with open(HEADER) as f:
        text = f.read()
    consts = dict(re.findall(r'#define (MCGP_MAX_CONDITION\w*) (\d+)', text))
    assert consts == {'MCGP_MAX_CONDITIONS': '64', 'MCGP_MAX_CONDITION_ATOMS': '8'}
    assert (N.MAX_CONDITIONS, N.MAX_CONDITION_ATOMS) == (64, 8)
    facts = dict(re.findall(r'(MCGP_FACT_\w+) = (\d+)', text))
    assert facts == {'MCGP_FACT_POSITION': '0', 'MCGP_FACT_GRID': '1', 'MCGP_FACT_RETIRED_LAP': '2',
                     'MCGP_FACT_AHEAD_BY': '3', 'MCGP_FACT_GAINED': '4', 'MCGP_FACT_FINISHERS': '5',
                     'MCGP_FACT_RED_FLAGS': '6', 'MCGP_FACT_SAFETY_CARS': '7', 'MCGP_FACT_VSCS': '8'}
    assert [getattr(N, 'FACT_' + k[10:]) for k in facts] == list(range(9))
    assert (CR.POSITION, CR.GRID, CR.RETIRED_LAP, CR.AHEAD_BY, CR.GAINED, CR.FINISHERS, CR.RED_FLAGS, CR.SAFETY_CARS,
            CR.VSCS) == tuple(range(9))
    # typedef struct mcgp_condition_atom { int32_t fact, a, b, lo, hi, negate; }
    atom = re.search(r'typedef struct mcgp_condition_atom \{ int32_t (.*?); \}', text).group(1)
    assert [x.strip() for x in atom.split(',')] == [f for f, _ in N.McgpConditionAtom._fields_]
    assert _fields(N.McgpConditionAtom) == [('fact', 0, 4), ('a', 4, 4), ('b', 8, 4), ('lo', 12, 4), ('hi', 16, 4),
                                            ('negate', 20, 4)]
    assert C.sizeof(N.McgpConditionAtom) == 24
    assert re.search(r'typedef struct mcgp_condition \{ uint32_t n_atoms; mcgp_condition_atom atom\[MCGP_MAX_CONDITION_ATOMS\]; \}',
                     text)
    assert _fields(N.McgpCondition) == [('n_atoms', 0, 4), ('atom', 4, 192)] and C.sizeof(N.McgpCondition) == 196
    decl = re.search(r'int32_t mcgp_run_conditions\((.*?)\);', text, re.S).group(1)
    params = [' '.join(p.split()) for p in decl.split(',')]
    ctype = {'const mcgp_config *': C.POINTER(N.McgpConfig), 'const mcgp_drivers *': C.POINTER(N.McgpDrivers),
             'const double *': C.POINTER(C.c_double), 'const mcgp_race_state *': C.POINTER(N.McgpRaceState),
             'const mcgp_condition *': C.POINTER(N.McgpCondition), 'uint32_t ': C.c_uint32, 'uint64_t ': C.c_uint64,
             'int32_t ': C.c_int32, 'uint64_t *': C.POINTER(C.c_uint64)}
    want = [ctype[re.match(r'(.*?[ *])\w+$', p).group(1)] for p in params]
    assert len(want) == 14 and L.mcgp_run_conditions.argtypes == want == N.CONDITIONS_ARGTYPES
    assert L.mcgp_run_conditions.restype is C.c_int32
    assert [p.split()[-1].lstrip('*') for p in params][-3:] == ['hist_out', 'count_out', 'cond_hist_out']


_BAD = [
    ('hist', dict(null=('hist',)), 'hist_out'),
    ('count', dict(null=('count',)), 'count_out'),
    ('neither', dict(null=('grid_probs',)), 'grid_probs'),
    ('both', dict(state=_state(3), both=True), 'grid_probs'),
    ('n0', dict(n=0), 'n must be in [1, 32]'),
    ('n33', dict(n=33), 'n must be in [1, 32]'),
    ('laps0', dict(laps=0), 'total_laps must be in [1, 1000]'),
    ('laps1001', dict(laps=1001), 'total_laps must be in [1, 1000]'),
    ('deviates53', dict(deviates=53), 'MCGP_DEVIATES_32'),
    ('conditions0', dict(n_conditions=0), 'n_conditions must be in [1, 64]'),
    ('conditions65', dict(conds=(WIN0,) * 65), 'n_conditions must be in [1, 64]'),
    ('conditions_null', dict(null=('conditions',)), 'conditions is NULL'),
    ('atoms9', dict(conds=(WIN0, WIN0), n_atoms=(1, 9)), 'conditions[1].n_atoms'),
    ('fact_unknown', dict(conds=(WIN0, [WIN0[0], (9, 0, 0, 0, 1, 0)])), 'conditions[1].atom[1].fact'),
    ('fact_negative', dict(conds=([(-1, 0, 0, 0, 1, 0)],)), 'conditions[0].atom[0].fact'),
    ('a_high', dict(conds=([(CR.GRID, 3, 0, 1, 1, 0)],)), 'conditions[0].atom[0].a'),
    ('a_negative', dict(conds=([(CR.RETIRED_LAP, -1, 0, 1, 1, 0)],)), 'conditions[0].atom[0].a'),
    ('a_high_gained', dict(conds=(WIN0, WIN0, [WIN0[0], WIN0[0], (CR.GAINED, 7, 0, 1, 1, 0)])), 'conditions[2].atom[2].a'),
    ('b_high', dict(conds=([(CR.AHEAD_BY, 0, 3, 1, 1, 0)],)), 'conditions[0].atom[0].b'),
    ('b_negative', dict(conds=([(CR.AHEAD_BY, 0, -2, 1, 1, 0)],)), 'conditions[0].atom[0].b'),
    ('a_is_b', dict(conds=([(CR.AHEAD_BY, 2, 2, 1, 1, 0)],)), 'two different drivers'),
    ('lo_above_hi', dict(conds=([(CR.FINISHERS, 0, 0, 2, 1, 0)],)), 'conditions[0].atom[0].lo'),
    ('state_lap', dict(state=_state(3, lap=61)), 'lap'),
    ('state_slot', dict(state=_state(3, grid_slot=np.array([0, 0, 1], np.uint8))), 'grid_slot'),
    ('state_time', dict(state=_state(3, cumulative_time=np.array([1.0, math.nan, 2.0]))), 'cumulative_time'),
]


@pytest.mark.parametrize('kw,msg', [(kw, msg) for _, kw, msg in _BAD], ids=[name for name, _, _ in _BAD])
def test_library_rejects_bad_arguments_before_any_device_lookup(kw, msg):
    """MCGP_E_BAD_ARG with a message that names the condition, the atom and the field, on a machine with or without a GPU
    (the checks come first: the device index is one no machine has), and the outputs keep their values."""
    rc, err, bufs = _abi_call(fill=5, device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert all((b == 5).all() for b in bufs.values())


def test_zero_simulations_need_no_device_and_limits_are_inclusive():
    eight = [(CR.POSITION, 0, 0, 1, 1, 0)] * 8
    for kw in (dict(n=1, laps=1), dict(n=32, laps=1000, conds=(eight,) * 64), dict(conds=(CR.EMPTY,)),
               dict(n=3, null=('cond_hist',)), dict(state=_state(3, lap=60)), dict(state=_state(3, lap=1)),
               # bounds beyond a fact's range are legal; a / b are ignored for the race-wide facts
               dict(conds=([(CR.POSITION, 0, 0, LO, HI, 1)], [(CR.FINISHERS, 99, -5, -7, -7, 0)],
                           [(CR.VSCS, -1, 99, 100000, HI, 0)], [(CR.AHEAD_BY, 0, 2, LO, LO, 0)]))):
        rc, err, bufs = _abi_call(n_sims=0, fill=3, device=999, **kw)
        assert rc == 0, (kw, err)
        assert all((b == 3).all() for b in bufs.values())


def test_outputs_untouched_when_the_device_lookup_fails():
    """A device index no machine has: every argument passes, the device lookup fails, the buffers keep their values."""
    for kw in (dict(), dict(state=_state(4))):
        rc, err, bufs = _abi_call(n=4, device=999, fill=7, **kw)
        assert rc == -2 and 'device' in err
        assert all((b == 7).all() for b in bufs.values())


# ---------------------------------------------------------------- the parser
D = ['VER', 'NOR', 'LEC', 'PIA']


def _atoms(text):
    return [(a.fact, a.a, a.b, a.lo, a.hi, int(a.negate)) for a in CD.parse(text, D).atoms]


@pytest.mark.parametrize('text,want', [
    ('VER.pos=1', [(0, 0, 0, 1, 1, 0)]),
    ('NOR.pos != 2', [(0, 1, 0, 2, 2, 1)]),
    ('LEC.pos<4', [(0, 2, 0, LO, 3, 0)]),
    ('LEC.pos <= 4', [(0, 2, 0, LO, 4, 0)]),
    ('PIA.grid>2', [(1, 3, 0, 3, HI, 0)]),
    ('PIA.grid >=2', [(1, 3, 0, 2, HI, 0)]),
    ('VER.out in 2..30', [(2, 0, 0, 2, 30, 0)]),
    ('VER.gain>=3', [(4, 0, 0, 3, HI, 0)]),
    ('VER.gain in -5..-1', [(4, 0, 0, -5, -1, 0)]),
    ('NOR.ahead_of.PIA > 0', [(3, 1, 3, 1, HI, 0)]),
    ('NOR.ahead_of.PIA in -1 .. 1', [(3, 1, 3, -1, 1, 0)]),
    ('finishers<16', [(5, 0, 0, LO, 15, 0)]),
    ('red=0', [(6, 0, 0, 0, 0, 0)]),
    ('sc>=1', [(7, 0, 0, 1, HI, 0)]),
    ('vsc in 1..2', [(8, 0, 0, 1, 2, 0)]),
    ('VER.wins', [(0, 0, 0, 1, 1, 0)]),
    ('NOR.podium', [(0, 1, 0, 1, 3, 0)]),
    ('LEC.points', [(0, 2, 0, 1, 10, 0)]),
    ('LEC.pole', [(1, 2, 0, 1, 1, 0)]),
    ('NOR.dnf', [(2, 1, 0, 1, HI, 0)]),
    ('NOR.finishes', [(2, 1, 0, 0, 0, 0)]),
    ('VER.beats.NOR', [(3, 0, 1, 1, HI, 0)]),
    ('!VER.wins', [(0, 0, 0, 1, 1, 1)]),
    ('! sc >= 1', [(7, 0, 0, 1, HI, 1)]),
    ('!NOR.pos != 2', [(0, 1, 0, 2, 2, 0)]),
    ('  VER.wins&NOR.podium ', [(0, 0, 0, 1, 1, 0), (0, 1, 0, 1, 3, 0)]),
    ('NOR.points & PIA.points', [(0, 1, 0, 1, 10, 0), (0, 3, 0, 1, 10, 0)]),
    ('sc>=1 & !LEC.dnf & LEC.gain >= 3 & finishers < 4', [(7, 0, 0, 1, HI, 0), (2, 2, 0, 1, HI, 1), (4, 2, 0, 3, HI, 0),
                                                           (5, 0, 0, LO, 3, 0)]),
])
def test_parser_reads_every_subject_operator_and_shorthand(text, want):
    assert _atoms(text) == want
    c = CD.parse(text, D)
    assert isinstance(c, Condition) and c.text == text.strip() and CD.parse(c, D) is c
    s = c.c_struct()
    assert s.n_atoms == len(want)
    assert [(s.atom[k].fact, s.atom[k].a, s.atom[k].b, s.atom[k].lo, s.atom[k].hi, s.atom[k].negate)
            for k in range(s.n_atoms)] == want


@pytest.mark.parametrize('text,token,why', [
    ('HAM.wins', 'HAM', 'not among the drivers'),
    ('VER.beats.HAM', 'HAM', 'not among the drivers'),
    ('VER.wins & HAM.pos=1', 'HAM', 'not among the drivers'),
    ('VER.ahead_of.XXX>0', 'XXX', 'not among the drivers'),
    ('VER.pos', 'VER.pos', 'needs a comparison'),
    ('sc', 'sc', 'needs a comparison'),
    ('VER.ahead_of.NOR', 'VER.ahead_of.NOR', 'needs a comparison'),
    ('VER.wins=1', 'VER.wins', 'takes no comparison'),
    ('VER.beats.NOR>0', 'VER.beats.NOR', 'takes no comparison'),
    ('VER.speed>3', 'VER.speed', 'unknown subject'),
    ('laps>3', 'laps', 'unknown subject'),
    ('VER.winz', 'VER.winz', 'unknown shorthand'),
    ('VER', 'VER', 'unknown shorthand'),
    ('VER.pos<=x', 'x', 'not an integer'),
    ('VER.pos<=1.5', '1.5', 'not an integer'),
    ('VER.pos<', '', 'not an integer'),
    ('sc in 1..x', 'x', 'not an integer'),
    ('sc in 3..1', 'sc in 3..1', 'empty'),
    ('VER.pos < 99999999999', '99999999999', 'beyond'),
    ('VER.beats.VER', 'VER.beats.VER', 'two different drivers'),
    ('VER.ahead_of.VER>0', 'VER.ahead_of.VER', 'two different drivers'),
    ('VER.wins &', '', 'empty atom'),
    ('VER.wins && NOR.wins', '', 'empty atom'),
    ('!', '!', 'empty atom'),
    ('VER wins', 'VER wins', 'expected SUBJECT OP VALUE'),
])
def test_parser_errors_name_the_text_and_the_token(text, token, why):
    with pytest.raises(ValueError) as e:
        CD.parse(text, D)
    msg = str(e.value)
    assert repr(text) in msg and repr(token) in msg and why in msg, msg


def test_parser_limits():
    with pytest.raises(ValueError, match='empty'):
        CD.parse('   ', D)
    with pytest.raises(ValueError, match='9 atoms, at most 8'):
        CD.parse(' & '.join(['VER.wins'] * 9), D)
    assert len(CD.parse(' & '.join(['VER.wins'] * 8), D).atoms) == 8
    with pytest.raises(ValueError, match='string or a Condition'):
        CD.parse(5, D)
    with pytest.raises(ValueError, match='1 to 64'):
        CD.parse_all({}, D)
    with pytest.raises(ValueError, match='1 to 64'):
        CD.parse_all({str(i): 'VER.wins' for i in range(65)}, D)
    with pytest.raises(ValueError, match='dict'):
        CD.parse_all(['VER.wins'], D)
    parsed = CD.parse_all({'w': 'VER.wins', 'all': Condition(())}, D)
    arr = CD.c_array(parsed)
    assert len(arr) == 2 and arr[0].n_atoms == 1 and arr[1].n_atoms == 0


def test_parser_agrees_with_the_reference_evaluation():
    """The texts of the issue's examples, evaluated by the reference on a hand-made table of facts."""
    #            orders (driver classified p-th)   slot by driver   retired lap by driver   red sc vsc
    facts = CR.facts_of([[0, 1, 2, 3], [1, 3, 0, 2], [2, 0, 3, 1], [3, 2, 1, 0]],
                        [[0, 1, 2, 3], [3, 0, 1, 2], [1, 2, 0, 3], [0, 1, 2, 3]],
                        [[0, 0, 0, 0], [0, 0, 7, 0], [0, 1, 0, 0], [9, 5, 0, 0]], [[0, 0, 0], [0, 1, 0], [1, 2, 0], [0, 0, 3]])
    want = {'VER.wins & NOR.podium': [1, 0, 0, 0], 'NOR.points & PIA.points': [1, 1, 1, 1], 'sc>=1': [0, 1, 1, 0],
            'LEC.pole': [0, 0, 1, 0], 'NOR.dnf': [0, 0, 1, 1], 'VER.gain>=1': [0, 1, 0, 0], 'finishers<3': [0, 0, 0, 1],
            'NOR.out=1': [0, 0, 1, 0], '!VER.finishes': [0, 0, 0, 1], 'PIA.beats.VER & vsc=0': [0, 1, 0, 0],
            'VER.ahead_of.LEC in 1..2': [1, 1, 0, 0], 'red != 0': [0, 0, 1, 0]}
    for text, col in want.items():
        assert CR.holds(facts, _atoms(text)).astype(int).tolist() == col, text
    conds = [_atoms(t) for t in want]
    assert CR.masks(facts, conds).tolist() == [sum(col[i] << c for c, col in enumerate(want.values())) for i in range(4)]
    got = CR.counts(facts, conds)
    assert got['count'].tolist() == [sum(col) for col in want.values()]
    assert got['cond_hist'][2].tolist() == [[0, 1, 1, 0], [1, 0, 0, 1], [1, 0, 0, 1], [0, 1, 1, 0]]       # given sc>=1
    assert facts['finishers'].tolist() == [4, 3, 3, 2] and CR.holds(facts, CR.EMPTY).all()
    assert CR.holds(facts, CR.ALWAYS).all() and not CR.holds(facts, CR.NEVER).any()


# ---------------------------------------------------------------- ConditionResult on hand-made counts
def _hand_result():
    """Drivers A B C, 10 simulations; 'x' met in 4 of them, 'never' in none, 'all' in all."""
    hist = np.array([[5, 3, 2], [3, 4, 3], [2, 3, 5]])
    cond = np.array([[[3, 1, 0], [1, 2, 1], [0, 1, 3]], np.zeros((3, 3), int), hist])
    return ConditionResult(drivers=['A', 'B', 'C'], names=['x', 'never', 'all'], n_simulations=10, hist=hist,
                           counts={'x': 4, 'never': 0, 'all': 10}, cond_hist=cond)


def test_result_arithmetic():
    r = _hand_result()
    assert r.probability('x') == 0.4 and r.probability('never') == 0.0 and r.probability('all') == 1.0
    assert r.standard_error('x') == math.sqrt(0.4 * 0.6 / 10) and r.standard_error('all') == 0.0
    assert r.position_probabilities() == {'A': {1: 0.5, 2: 0.3, 3: 0.2}, 'B': {1: 0.3, 2: 0.4, 3: 0.3},
                                          'C': {1: 0.2, 2: 0.3, 3: 0.5}}
    assert r.position_probabilities('x') == {'A': {1: 0.75, 2: 0.25}, 'B': {1: 0.25, 2: 0.5, 3: 0.25}, 'C': {2: 0.25, 3: 0.75}}
    assert r.position_probabilities('all') == r.position_probabilities()
    assert r.win_probability('x', 'A') == 0.75 and r.win_probability(None, 'A') == 0.5
    assert r.podium_probability('x', 'C') == 1.0 and r.win_probability('x', 'C') == 0.0
    assert r.counts == {'x': 4, 'never': 0, 'all': 10} and r.n_simulations == 10
    for call in (lambda: r.win_probability('never', 'A'), lambda: r.podium_probability('never', 'A'),
                 lambda: r.position_probabilities('never')):
        with pytest.raises(ValueError, match="'never'"):
            call()
    with pytest.raises(KeyError):
        r.probability('nope')
    with pytest.raises(KeyError):
        r.win_probability('x', 'Z')
    s = r.summary()
    assert s['x']['count'] == 4 and s['x']['win']['A'] == {'given': 0.75, 'unconditional': 0.5}
    assert s['never']['win']['A'] == {'given': None, 'unconditional': 0.5} and s['never']['probability'] == 0.0
    assert s['x']['podium']['B'] == {'given': 1.0, 'unconditional': 1.0}
    json.dumps(s)
    # a run without the histograms has probabilities and counts, and says so when asked for more
    light = _hand_result()
    light.cond_hist = None
    assert light.probability('x') == 0.4 and light.standard_error('x') == r.standard_error('x')
    assert light.position_probabilities() == r.position_probabilities() and light.win_probability(None, 'A') == 0.5
    for call in (lambda: light.win_probability('x', 'A'), lambda: light.podium_probability('all', 'A'),
                 lambda: light.position_probabilities('x')):
        with pytest.raises(ValueError, match='not collected'):
            call()
    ls = light.summary()
    assert ls['x']['probability'] == 0.4 and ls['x']['win']['A'] == {'given': None, 'unconditional': 0.5}


def test_run_conditions_of_nothing_needs_no_device_and_python_checks_its_arguments():
    case = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**case['config']))
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'])
    res = sim.run_conditions(0, {'double': 'VER.wins & NOR.podium', 'sc': 'sc>=1'}, *args)
    assert isinstance(res, ConditionResult) and res.n_simulations == 0 and res.names == ['double', 'sc']
    assert res.counts == {'double': 0, 'sc': 0} and res.cond_hist.shape == (2, 20, 20) and res.probability('sc') == 0.0
    assert sim.run_conditions(0, {'sc': 'sc>=1'}, *args, histograms=False).cond_hist is None
    assert sim.last_drivers == list(case['grid_probs']) and not sim.last_histogram.any()
    for conds, msg in (({'x': 'XXX.wins'}, 'not among the drivers'), ({}, '1 to 64'), ({'x': 'VER.pos'}, 'comparison'),
                       (['VER.wins'], 'dict')):
        with pytest.raises(ValueError, match=msg):
            sim.run_conditions(10, conds, *args)
    with pytest.raises(ValueError, match='exactly one'):
        sim.run_conditions(10, {'x': 'VER.wins'}, None, *args[1:])


# ---------------------------------------------------------------- the predictor and the CLI with fakes
class _FakeSimulator:
    """RaceSimulator's run_conditions from hand-made counts (no device)."""
    def __init__(self):
        self.calls = []

    def _resolve_seed(self, seed):
        return 77 if seed is None else seed

    def run_conditions(self, n_simulations, conditions, grid_probs, *args, **kw):
        self.calls.append((n_simulations, dict(conditions), grid_probs, kw))
        r = _hand_result()
        r.names = list(conditions)
        r.counts = dict(zip(r.names, [4, 0, 10]))
        return r


def test_predictor_adds_the_conditions_block():
    sim = _FakeSimulator()
    drivers = ['A', 'B', 'C']
    inp = dict(drivers=drivers, base_pace={}, tire_deg={}, driver_variance={}, driver_dnf_rates={}, track_condition='dry',
               weather={})
    grid = {d: [1 / 3] * 3 for d in drivers}
    conds = {'x': 'A.wins', 'never': 'finishers<0', 'all': 'finishers>=0'}
    res = P.F1Predictor._with_counts(sim, inp, grid, 10, None, 'fp2', None, False, False, None, conds)
    assert sim.calls == [(10, conds, grid, {'seed': 77, 'track_condition': 'dry'})]
    assert res['win_probabilities'] == {'A': 0.5, 'B': 0.3, 'C': 0.2}
    block = res['conditions']
    assert list(block) == ['x', 'never', 'all'] and block == P.condition_keys(_hand_result())
    assert block['x']['probability'] == 0.4 and block['x']['standard_error'] == math.sqrt(0.024)
    assert block['x']['win']['A'] == {'given': 0.75, 'unconditional': 0.5}
    assert block['never']['podium']['A']['given'] is None


class _FakePredictor:
    """predict_weekend's / predict_from_state's result shape from hand-made counts (no device)."""
    calls = []

    def __init__(self, device=0):
        pass

    @staticmethod
    def _block(drivers, conditions):
        n = len(drivers)
        hist = np.zeros((n, n), int)
        hist[np.arange(n), np.arange(n)] = 8
        cond = np.zeros((len(conditions), n, n), int)
        cond[:, np.arange(n), np.arange(n)] = 2
        counts = {name: 2 for name in conditions}
        if 'finishers<0' in counts:
            counts['finishers<0'] = 0
        return P.condition_keys(ConditionResult(drivers=drivers, names=list(conditions), n_simulations=8, hist=hist,
                                                counts=counts, cond_hist=cond))

    def predict_weekend(self, season, race, fixture, prediction_point='fp2', n_simulations=0, seed=None, matchups=False,
                        **kw):
        _FakePredictor.calls.append(kw)
        drivers = list(fixture['drivers'])
        n = len(drivers)
        res = P.pack_result(drivers, {d: [1.0 / n] * n for d in drivers}, {d: {1 + i: 1.0} for i, d in enumerate(drivers)},
                            {}, prediction_point, None)
        if kw.get('conditions'):
            res['conditions'] = self._block(drivers, kw['conditions'])
        return res

    def predict_from_state(self, season, race, fixture, states, n_simulations=0, seed=None, **kw):
        _FakePredictor.calls.append(kw)
        drivers = list(fixture['drivers'])
        out = []
        for st in states:
            r = {'lap': st.lap, 'win_probabilities': {d: float(i == 0) for i, d in enumerate(drivers)},
                 'podium_probabilities': {d: float(i < 3) for i, d in enumerate(drivers)}, 'points_probabilities': {},
                 'full_distributions': {}}
            if kw.get('conditions'):
                r['conditions'] = self._block(drivers, kw['conditions'])
            out.append(r)
        return out


def test_predict_if_flags(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    plain, extra = tmp_path / 'plain.json', tmp_path / 'cond.json'
    base = ['predict', '--race', 'Bahrain', '--offline', '--simulations', '20', '--seed', '1']
    assert cli.main(base + ['--json', str(plain)]) == 0
    assert 'CONDITIONS' not in capsys.readouterr().out
    drivers = list(cli.synthetic_fixture()['drivers'])
    a, b = drivers[0], drivers[1]
    texts = [f'{a}.wins & {b}.podium', ' sc>=1 ', 'finishers<0']
    argv = list(base)
    for t in texts:
        argv += ['--if', t]
    assert cli.main(argv + ['--json', str(extra)]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [{}, {'conditions': {t.strip(): t for t in texts}}]
    assert out.index('PODIUM PROBABILITIES') < out.index('CONDITIONS')
    assert f'{a}.wins & {b}.podium:  25.0%' in out and 'sc>=1:  25.0%' in out and '(2 simulations)' in out
    assert 'never met: no conditional odds' in out and f'{a:4} wins 100.0% if so (overall 100.0%)' in out
    pa, pb = json.loads(plain.read_text()), json.loads(extra.read_text())
    assert 'conditions' not in pa and set(pb) == set(pa) | {'conditions'} and {k: pb[k] for k in pa} == pa
    assert list(pb['conditions']) == [t.strip() for t in texts] and pb['conditions']['sc>=1']['probability'] == 0.25
    with pytest.raises(SystemExit):
        cli.main(base + ['--if', 'sc>=1', '--if', 'sc>=1 '])


def test_in_race_if_flags(tmp_path, capsys, monkeypatch):
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
    assert 'CONDITIONS' not in capsys.readouterr().out
    assert cli.main(base + ['--if', f'{drivers[1]}.dnf', '--json', str(tmp_path / 'o.json')]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [{}, {'conditions': {f'{drivers[1]}.dnf': f'{drivers[1]}.dnf'}}]
    assert 'CONDITIONS' in out and f'{drivers[1]}.dnf:  25.0%' in out
    assert json.loads((tmp_path / 'o.json').read_text())[0]['conditions'][f'{drivers[1]}.dnf']['count'] == 2
