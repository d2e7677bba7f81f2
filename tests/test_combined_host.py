"""Combined what-if scenarios, host side: the Python restatement (combined_ref) against the four restatements it is built
beside, and the C-ABI argument checks of mcgp_run_combined, which are made before any device lookup and so need no
device."""
import ctypes as C

import numpy as np
import pytest

import combined_ref as CR
import events_ref as ER
import oracle_py as O
import paces_ref as PR
import penalties_ref as NR
import resume_ref as RR
import strategy_ref as SR
from monte_carlo_gp_amd import RaceConfig
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, _Problem

M, SEED, OFFSET = 24, 47, 300
H = 2
inf = float('inf')


# ---------------------------------------------------------------- the restatement against its siblings
_traced = {}


def _ref(name):
    if name not in _traced:
        _traced[name] = RR.traced_run(O.load_case(name), 40, SEED, OFFSET)
    return _traced[name]


def _starts(name):
    """(label, first lap with a pit step, keyword arguments of the restatements' orders())."""
    case, ref = O.load_case(name), _ref(name)
    k = case['config']['total_laps'] // 2
    state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFFSET + 3, k))
    return [('grid', 2, dict(grids=ref['grids'])), ('state', k + 1, dict(state=state))]


@pytest.mark.parametrize('name', ['S60', 'EVT'])
def test_the_restatement_with_one_table_is_the_restatement_of_that_call(name):
    case = O.load_case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    zeros = np.zeros((M, n), np.int64)
    for label, first, kw in _starts(name):
        # no table: strategy_ref, and events_ref's counts of the drawn events
        for plans in ({}, {0: (-1, 0, [(first + 3, 2)])}):
            o, f, e, c = CR.orders(case, M, SEED, OFFSET, plans=plans, **kw)
            assert np.array_equal(o, SR.orders(case, M, SEED, OFFSET, plans=plans, **kw)), label
            assert np.array_equal(e, ER.orders(case, M, SEED, OFFSET, plans=plans, **kw)[1])
            assert not f.any() and not c.any()
        if label == 'grid':                                 # ... and, without plans, the pinned oracle
            assert np.array_equal(CR.orders(case, M, SEED, OFFSET, **kw)[0], _ref(name)['orders'][:M])
        drawn = ER.orders(case, M, SEED, OFFSET, **kw)[1]
        changed = 0
        for pens, plans in NR.scenarios(first, L, n):
            o, f, e, c = CR.orders(case, M, SEED, OFFSET, plans=plans, penalties=pens, **kw)
            want_o, want_f = NR.orders(case, M, SEED, OFFSET, plans=plans, penalties=pens, **kw)
            assert np.array_equal(o, want_o) and np.array_equal(f, want_f), (label, pens)
            assert np.array_equal(c, zeros) and (plans or np.array_equal(e, drawn))
            changed += bool(f.any())
        assert changed
        for evs, plans in ER.scenarios(first, L, n):
            o, f, e, c = CR.orders(case, M, SEED, OFFSET, plans=plans, overrides=evs, **kw)
            want_o, want_e = ER.orders(case, M, SEED, OFFSET, plans=plans, overrides=evs, **kw)
            assert np.array_equal(o, want_o) and np.array_equal(e, want_e), (label, evs)
            assert not f.any() and not c.any()
        for offs, plans in PR.scenarios(1 if label == 'grid' else first, L, n):
            o, f, e, c = CR.orders(case, M, SEED, OFFSET, plans=plans, offsets=offs, **kw)
            want_o, want_c = PR.orders(case, M, SEED, OFFSET, plans=plans, offsets=offs, **kw)
            assert np.array_equal(o, want_o) and np.array_equal(c, want_c), (label, offs)
            assert not f.any()


# ---------------------------------------------------------------- the C ABI without a device
def _prob(n=3, laps=60, deviates=32):
    c = O.load_case('S60')
    cfg = dict(c['config'], total_laps=laps)
    return _Problem(RaceConfig(**cfg), [f'D{i:02d}' for i in range(n)], {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)


def _call(scen=None, n=3, laps=60, state=None, grid=True, n_sims=100, deviates=32, null=(), n_scenarios=None, fill=5,
          device=0):
    """mcgp_run_combined on scenario() dicts -> (rc, message, whether every output kept its fill).  null: the arguments
    passed as NULL, by name."""
    scen = [CR.scenario()] if scen is None else list(scen)
    prob = _prob(n, laps, deviates)
    counts, c_plans = SR.c_plans([sc['plans'] for sc in scen])
    ncounts, c_pens = NR.c_penalties([sc['penalties'] for sc in scen])
    ecounts, c_evs = ER.c_events([sc['events'] for sc in scen])
    pcounts, c_offs = PR.c_paces([sc['paces'] for sc in scen])
    S = len(scen) if n_scenarios is None else n_scenarios
    g = np.full((max(n, 1), max(n, 1)), 1.0 / max(n, 1))
    cs = RR.c_state(*state) if state is not None else None
    rows = max(S, 1) * n
    outs = [np.full(rows * n, fill, np.uint64), np.full(rows * (2 * n - 1), fill, np.uint64),
            np.full(rows * 4, fill, np.uint64), np.full(max(S, 1) * 3 * (laps + 1), fill, np.uint64),
            np.full(rows * (laps + 1), fill, np.uint64)]
    o = np.full(rows * max(n_sims, 1), fill, np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    arg = lambda name, value: None if name in null else value
    rc = N.lib().mcgp_run_combined(
        arg('cfg', C.byref(prob.cfg)), C.byref(prob.drv), g.ctypes.data_as(C.POINTER(C.c_double)) if grid else None,
        C.byref(cs) if cs is not None else None, n, S, arg('plan_count', counts), arg('plans', c_plans),
        arg('penalty_count', ncounts), arg('penalties', c_pens), arg('event_count', ecounts), arg('events', c_evs),
        arg('pace_count', pcounts), arg('paces', c_offs), n_sims, 0, 1, device, arg('hist', u64(outs[0])),
        *[u64(a) for a in outs[1:]], o.ctypes.data_as(C.POINTER(C.c_uint8)))
    untouched = all((a == fill).all() for a in outs) and (o == fill).all()
    return rc, N.lib().mcgp_last_error().decode(), untouched


def _state(n=3, lap=10):
    a = dict(cumulative_time=np.array([100.0 * lap + d for d in range(n)], np.float64),
             last_lap_time=np.full(n, 91.5, np.float64), grid_slot=np.arange(n, dtype=np.uint8),
             compound=np.full(n, 1, np.uint8), used_compounds=np.full(n, 0b011, np.uint8),
             tire_age=np.full(n, 7, np.int16), retired_lap=np.zeros(n, np.int16))
    return (a, lap, 0)


sc = CR.scenario
SERVE, FLAG, LAP, LAPS, UNTIL = CR.SERVE, CR.FLAG, CR.LAP, CR.LAPS, CR.UNTIL_STOP
FROM20 = dict(state=_state(lap=20), grid=False)

BAD = [
    (dict(scen=(), n_scenarios=0), 'n_scenarios must be in [1, 64]'),
    (dict(scen=(sc(),) * 65), 'n_scenarios must be in [1, 64]'),
    # an items pointer missing with a non-zero count, per table
    (dict(scen=(sc(penalties=[(0, FLAG, 0, 5.0)]),), null=('penalties',)), 'penalties is NULL'),
    (dict(scen=(sc(events=[(5, 5, 2)]),), null=('events',)), 'events is NULL'),
    (dict(scen=(sc(paces=[(0, LAPS, 5, 5, 0.5)]),), null=('paces',)), 'paces is NULL'),
    (dict(scen=(sc({0: (-1, 0, [(20, H)])}),), null=('plans',)), 'plans is NULL'),
    # each kind's limit, with its table's name
    (dict(scen=(sc(), sc(penalties=[(k % 3, LAP, 2 + k // 3, 1.0) for k in range(257)]))),
     'scenario 1: penalty_count must be in [0, 256]'),
    (dict(scen=(sc(events=[(2, 2, 0)] * 65),)), 'scenario 0: event_count must be in [0, 64]'),
    (dict(scen=(sc(), sc(), sc(paces=[(k % 3, LAPS, 1 + k // 3, 1 + k // 3, 0.1) for k in range(65)]))),
     'scenario 2: pace_count must be in [0, 64]'),
    # the item is named by its table, so "lap" and "first_lap" are never ambiguous
    (dict(scen=(sc(penalties=[(0, SERVE, 1, 5.0)]),)),
     'scenario 0, penalty 0: lap must be in [2, total_laps] (lap 1 has no pit step)'),
    (dict(scen=(sc(events=[(1, 5, 2)]),)), 'scenario 0, event 0: first_lap must be in [2, total_laps] (lap 1 has no event)'),
    (dict(scen=(sc(paces=[(0, LAPS, 0, 5, 0.5)]),)), 'scenario 0, offset 0: first_lap must be in [1, total_laps]'),
    (dict(scen=(sc(penalties=[(0, LAP, 20, 5.0)]),), **FROM20),
     "scenario 0, penalty 0: lap must be in [21, total_laps] (after the state's lap)"),
    (dict(scen=(sc(events=[(20, 25, 3)]),), **FROM20),
     "scenario 0, event 0: first_lap must be in [21, total_laps] (after the state's lap)"),
    (dict(scen=(sc(paces=[(0, UNTIL, 20, 0, 0.5)]),), **FROM20),
     "scenario 0, offset 0: first_lap must be in [21, total_laps] (after the state's lap)"),
    # the tables are checked in the order penalties, events, offsets; a good table does not hide a bad one
    (dict(scen=(sc(penalties=[(0, FLAG, 0, 5.0)], events=[(5, 5, 2)], paces=[(3, LAPS, 5, 5, 0.5)]),)),
     'scenario 0, offset 0: driver must be in [0, n)'),
    (dict(scen=(sc(), sc(penalties=[(0, FLAG, 0, 5.0), (0, FLAG, 0, 5.0)], events=[(5, 5, 9)]))),
     'scenario 1, penalty 1: driver 0 has two MCGP_PEN_AT_FLAG penalties'),
    (dict(scen=(sc(events=[(5, 9, 2), (9, 9, 1)], paces=[(0, LAPS, 5, 5, inf)]),)),
     'scenario 0, event 1: first_lap..last_lap: lap 9 has two overrides'),
    (dict(scen=(sc(paces=[(1, UNTIL, 5, 0, 0.5), (1, UNTIL, 30, 0, 0.5)]),)),
     'scenario 0, offset 1: driver 1 has two MCGP_PACE_UNTIL_STOP offsets in this scenario'),
    (dict(scen=(sc({1: (-1, 0, [(61, H)])}, penalties=[(0, FLAG, 0, 5.0)]),)),
     'scenario 0, plan 0: stop 0: stop_lap must be in [2, total_laps]'),
    (dict(deviates=53), 'MCGP_DEVIATES_32'),
    (dict(null=('hist',)), 'hist_out is NULL'),
    (dict(null=('plan_count',)), 'plan_count is NULL'),
    (dict(null=('cfg',)), 'cfg / drv is NULL'),
    (dict(grid=False), 'grid_probs is NULL'),
    (dict(state=_state()), 'grid_probs must be NULL when a state is given'),
    (dict(n=0), 'n must be in [1, 32]'),
    (dict(laps=1001), 'total_laps must be in [1, 1000]'),
]


@pytest.mark.parametrize('kw,msg', BAD, ids=[f'{i}: {m}' for i, (_, m) in enumerate(BAD)])
def test_library_rejects_bad_arguments_before_any_device_lookup(kw, msg):
    """MCGP_E_BAD_ARG naming the scenario, the item by its table and the field, on a machine with or without a GPU
    (device 999 is never looked up: the checks come first), and the outputs keep their values."""
    rc, err, untouched = _call(device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert untouched


def test_null_count_arrays_limits_and_zero_simulations_need_no_device():
    full = sc({0: (-1, 0, [(30, H)])}, [(0, SERVE, 2, 5.0), (1, FLAG, 0, 10.0), (2, LAP, 60, 3.0)],
              [(2, 2, 2), (60, 60, 1)], [(0, LAPS, 1, 60, 60.0), (0, UNTIL, 1, 0, -60.0)])
    ok = [
        dict(null=('penalty_count', 'penalties', 'event_count', 'events', 'pace_count', 'paces', 'plans')),
        dict(null=('penalty_count', 'event_count', 'pace_count')),          # the item pointers are then not read
        dict(scen=(sc(), full), null=('event_count', 'events')),
        dict(scen=(sc(), full), null=('penalty_count',)),                   # its penalties are then nobody's
        dict(scen=(sc(), full)),
        dict(scen=(sc(),) * 64),
        dict(null=('penalties', 'events', 'paces', 'plans')),               # every count is 0
        dict(scen=(sc(penalties=[(0, SERVE, 11, 5.0)], events=[(11, 11, 1)], paces=[(0, UNTIL, 11, 0, 0.3)]),),
             state=_state(lap=10), grid=False),
        dict(scen=(sc(),), state=_state(lap=60), grid=False),               # nothing left to run
    ]
    for kw in ok:
        rc, err, untouched = _call(n_sims=0, device=999, **kw)
        assert rc == 0 and untouched, (kw, err)
    # every table at its limit in each of 64 scenarios, 32 cars, 1000 laps
    big = sc({d: (-1, 0, []) for d in range(32)}, [(k % 32, LAP, 2 + k // 32, 1.0) for k in range(256)],
             [(2 + k, 2 + k, k % 4) for k in range(64)],
             [(k // 2, k % 2, 1 + 15 * k, (10 + 15 * k) * (1 - k % 2), 0.01 * k) for k in range(64)])
    rc, err, untouched = _call(scen=(big,) * 64, n=32, laps=1000, n_sims=0, device=999)
    assert rc == 0 and untouched, err
    # with simulations, a valid call gets past the checks to the device lookup
    rc, err, untouched = _call(scen=(sc(), full), n_sims=10, device=999)
    assert rc == -2 and untouched, err


def test_the_header_declares_the_entry_point_and_the_abi_version_stays():
    with open(O.ROOT + '/include/mcgp.h') as f:
        header = f.read()
    assert 'int32_t mcgp_run_combined(const mcgp_config *cfg' in header and '#define MCGP_ABI_VERSION 6' in header
    assert 'mcgp_run_combined' in N.EXPORTS and hasattr(N.lib(), 'mcgp_run_combined')
    assert N.lib().mcgp_abi_version() == 6
