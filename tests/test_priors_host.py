"""Pace uncertainty, host side: the C-ABI argument checks of mcgp_run_priors (no device needed), the struct layout,
PacePrior's constructors and run_priors' ValueErrors, the scenario names, PriorResult's helpers on hand-made counts, the
`uncertainty` command's parsing and the JSON safety of the predictor's block."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import oracle_py as O
import priors_ref as QR
import strategy_ref as SR
from monte_carlo_gp_amd import PacePrior, PriorResult, RaceConfig, StrategyResult
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, RaceSimulator, _Problem

D, G = QR.DRIVER, QR.GROUP
H = 2
inf, nan = float('inf'), float('nan')


# ---------------------------------------------------------------- the C ABI without a device
def _prob(n=3, laps=60, deviates=32):
    c = O.load_case('S60')
    cfg = dict(c['config'], total_laps=laps)
    return _Problem(RaceConfig(**cfg), [f'D{i:02d}' for i in range(n)], {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)


def _items(scenarios):
    """[[(kind, driver, members, sigma), ...], ...] raw, so that any field may be wrong."""
    flat = [N.McgpPacePrior(kind=int(k), driver=int(d), members=int(mem), pad=0, sigma=float(s))
            for sc in scenarios for k, d, mem, s in sc]
    counts = [len(sc) for sc in scenarios]
    return (C.c_uint32 * max(len(counts), 1))(*counts), (N.McgpPacePrior * max(len(flat), 1))(*flat)


def _call(items=((),), plans=None, edges=(-0.1, 0.1), n=3, laps=60, grid=True, n_sims=100, deviates=32, null=(),
          n_scenarios=None, n_edges=None, fill=5, device=0):
    prob = _prob(n, laps, deviates)
    items = list(items)
    plans = list(plans) if plans is not None else [{}] * len(items)
    counts, c_plans = SR.c_plans(plans)
    pcounts, c_it = _items(items)
    S = len(items) if n_scenarios is None else n_scenarios
    B = 16
    e = np.ascontiguousarray(list(edges) + [0.0], np.float64)
    g = np.full((max(n, 1), max(n, 1)), 1.0 / max(n, 1))
    h = np.full(max(S, 1) * n * n, fill, np.uint64)
    dl = np.full(max(S, 1) * n * (2 * n - 1), fill, np.uint64)
    dr = np.full(max(S, 1) * n * B * n, fill, np.uint64)
    xo = np.full(max(S, 1) * max(n_sims, 1) * n, fill, np.float32)
    o = np.full(max(S, 1) * max(n_sims, 1) * n, fill, np.uint8)
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_priors(
        None if 'cfg' in null else C.byref(prob.cfg), C.byref(prob.drv),
        g.ctypes.data_as(C.POINTER(C.c_double)) if grid else None, None, n, S,
        None if 'plan_count' in null else counts, None if 'plans' in null else c_plans,
        None if 'prior_count' in null else pcounts, None if 'priors' in null else c_it,
        len(edges) if n_edges is None else n_edges, None if 'edges' in null else e.ctypes.data_as(C.POINTER(C.c_double)),
        n_sims, 0, 1, device, None if 'hist' in null else u64(h), u64(dl), u64(dr),
        xo.ctypes.data_as(C.POINTER(C.c_float)), o.ctypes.data_as(C.POINTER(C.c_uint8)))
    untouched = all((a == fill).all() for a in (h, dl, dr, xo, o))
    return rc, N.lib().mcgp_last_error().decode(), untouched


BAD = [
    (dict(items=(), n_scenarios=0), 'n_scenarios must be in [1, 64]'),
    (dict(items=([],) * 65), 'n_scenarios must be in [1, 64]'),
    (dict(null=('prior_count',)), 'prior_count is NULL'),
    (dict(items=([], [(D, 0, 0, 0.1)] * 65)), 'scenario 1: prior_count must be in [0, 64]'),
    (dict(items=([(D, 0, 0, 0.1)],), null=('priors',)), 'priors is NULL'),
    (dict(n_edges=16), 'n_edges must be in [0, 15]'),
    (dict(null=('edges',)), 'edges is NULL'),
    (dict(edges=(0.1, nan)), 'edges[1] must be finite'),
    (dict(edges=(inf,)), 'edges[0] must be finite'),
    (dict(edges=(0.1, 0.1)), 'edges[1] must be above edges[0]'),
    (dict(edges=(0.0, 0.2, 0.1)), 'edges[2] must be above edges[1]'),
    (dict(items=([], [(2, 0, 0, 0.1)])), 'scenario 1, item 0: kind must be MCGP_PRIOR_DRIVER or MCGP_PRIOR_GROUP'),
    (dict(items=([(-1, 0, 0, 0.1)],)), 'scenario 0, item 0: kind must be'),
    (dict(items=([(D, 0, 0, 0.1), (D, 1, 0, nan)],)), 'scenario 0, item 1: sigma must be finite and in [0, 10]'),
    (dict(items=([(D, 0, 0, inf)],)), 'sigma must be finite and in [0, 10]'),
    (dict(items=([(D, 0, 0, -0.001)],)), 'sigma must be finite and in [0, 10]'),
    (dict(items=([(G, 0, 3, 10.001)],)), 'sigma must be finite and in [0, 10]'),
    (dict(items=([(D, 3, 0, 0.1)],)), 'scenario 0, item 0: driver must be in [0, n)'),
    (dict(items=([(D, -1, 0, 0.1)],)), 'driver must be in [0, n)'),
    (dict(items=([(D, 1, 2, 0.1)],)), 'scenario 0, item 0: members must be 0 for MCGP_PRIOR_DRIVER'),
    (dict(items=([(G, 1, 3, 0.1)],)), 'scenario 0, item 0: driver must be 0 for MCGP_PRIOR_GROUP'),
    (dict(items=([(G, 0, 0, 0.1)],)), 'scenario 0, item 0: members must have at least one bit'),
    (dict(items=([(G, 0, 8, 0.1)],)), 'scenario 0, item 0: members must have no bit at or above n'),
    (dict(items=([(G, 0, 1 << 31, 0.1)],)), 'members must have no bit at or above n'),
    (dict(items=([], [(D, 1, 0, 0.1), (G, 0, 3, 0.1), (D, 1, 0, 0.2)])),
     'scenario 1, item 2: driver 1 has two MCGP_PRIOR_DRIVER items in this scenario'),
    (dict(items=([(G, 0, 3, 0.1), (G, 0, 6, 0.1)],)), 'scenario 0, item 1: members: driver 1 is in two groups in this scenario'),
    (dict(plans=({1: (-1, 0, [(61, H)])},)), 'scenario 0, plan 0: stop 0: stop_lap must be in [2, total_laps]'),
    (dict(deviates=53), 'MCGP_DEVIATES_32'),
    (dict(null=('hist',)), 'hist_out is NULL'),
    (dict(null=('plan_count',)), 'plan_count is NULL'),
    (dict(plans=({0: (-1, 0, [(20, H)])},), null=('plans',)), 'plans is NULL'),
    (dict(null=('cfg',)), 'cfg / drv is NULL'),
    (dict(grid=False), 'grid_probs is NULL'),
    (dict(n=0), 'n must be in [1, 32]'),
    (dict(n=33), 'n must be in [1, 32]'),
]


@pytest.mark.parametrize('kw,msg', BAD, ids=[f'{i}: {m}' for i, (_, m) in enumerate(BAD)])
def test_library_rejects_bad_arguments_before_any_device_lookup(kw, msg):
    """MCGP_E_BAD_ARG naming the scenario, the item and the field, on a machine with or without a GPU (device 999 is never
    looked up: the checks come first), and the outputs keep their values."""
    rc, err, untouched = _call(device=999, **kw)
    assert rc == -1 and msg in err, (kw, rc, err)
    assert untouched


def test_limits_are_inclusive_and_zero_simulations_need_no_device():
    ok = [
        dict(items=([],) * 64),
        dict(items=([(D, 0, 0, 0.0), (D, 1, 0, 10.0), (G, 0, 7, 10.0)],)),
        dict(items=([(G, 0, 1, 0.1), (G, 0, 2, 0.1), (G, 0, 4, 0.1)],)),              # groups of one
        dict(items=([(D, 0, 0, -0.0)],)),
        dict(edges=()), dict(edges=(), null=('edges',)),
        dict(edges=tuple(0.01 * i for i in range(15))),
        dict(items=([(D, 2, 0, 0.1)],), plans=({2: (H, 0, [(30, 1)])},)),
        dict(null=('plans', 'priors')),                     # every count is 0
    ]
    for kw in ok:
        rc, err, untouched = _call(n_sims=0, device=999, **kw)
        assert rc == 0 and untouched, (kw, err)
    # 64 items in each of 64 scenarios, 32 cars
    full = [(D, d, 0, 0.1) for d in range(32)] + [(G, 0, 1 << d, 0.2) for d in range(32)]
    rc, err, untouched = _call(items=(full,) * 64, n=32, n_sims=0, device=999)
    assert rc == 0 and untouched, err
    # with simulations, a valid call gets past the checks to the device lookup
    rc, err, untouched = _call(items=([(D, 0, 0, 0.2)],), n_sims=10, device=999)
    assert rc == -2 and untouched, err


def test_struct_matches_the_header():
    assert C.sizeof(N.McgpPacePrior) == 24
    assert [(f, getattr(N.McgpPacePrior, f).offset) for f, _ in N.McgpPacePrior._fields_] == [
        ('kind', 0), ('driver', 4), ('members', 8), ('pad', 12), ('sigma', 16)]
    with open(O.ROOT + '/include/mcgp.h') as f:
        header = f.read()
    assert 'enum { MCGP_PRIOR_DRIVER = 0, MCGP_PRIOR_GROUP = 1 };' in header
    assert 'typedef struct mcgp_pace_prior {' in header and '#define MCGP_ABI_VERSION 6' in header
    assert '#define MCGP_MAX_SCENARIO_PRIORS 64' in header and '#define MCGP_MAX_PRIOR_EDGES 15' in header
    assert (N.PRIOR_DRIVER, N.PRIOR_GROUP, N.MAX_SCENARIO_PRIORS, N.MAX_PRIOR_EDGES, N.MAX_PRIOR_SIGMA) == (0, 1, 64, 15, 10.0)
    assert 'mcgp_run_priors' in N.EXPORTS and hasattr(N.lib(), 'mcgp_run_priors')


# ---------------------------------------------------------------- Python layer
def test_pace_prior_constructors():
    index = {'VER': 0, 'NOR': 1, 'LEC': 2}
    c = PacePrior.driver('NOR', 0.15).c_struct(index)
    assert (c.kind, c.driver, c.members, c.sigma) == (N.PRIOR_DRIVER, 1, 0, 0.15)
    c = PacePrior.group(['LEC', 'VER'], 0.2).c_struct(index)
    assert (c.kind, c.driver, c.members, c.sigma) == (N.PRIOR_GROUP, 0, 0b101, 0.2)
    for bad in (PacePrior.driver('VER', -0.1), PacePrior.driver('VER', 10.5), PacePrior.driver('VER', nan),
                PacePrior.group([], 0.1), PacePrior.group(['VER', 'VER'], 0.1)):
        with pytest.raises(ValueError):
            bad.c_struct(index)


def _sim():
    c = O.load_case('S60')
    return RaceSimulator(RaceConfig(**c['config'])), c


def _kw(c):
    return dict(grid_probs=c['grid_probs'], base_pace=c['base_pace'], tire_deg=c['tire_deg'],
                driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'])


def test_run_priors_raises_before_the_library_is_asked():
    sim, c = _sim()
    names = list(c['grid_probs'])
    a, b = names[0], names[1]
    bad = [
        (dict(priors={'x': [PacePrior.driver('NOBODY', 0.1)]}), 'is not one of the drivers'),
        (dict(priors={'x': [PacePrior.group([a, 'NOBODY'], 0.1)]}), 'is not one of the drivers'),
        (dict(priors={'x': [PacePrior.driver(a, 0.1), PacePrior.driver(a, 0.2)]}), 'has two own priors'),
        (dict(priors={'x': [PacePrior.group([a, b], 0.1), PacePrior.group([b], 0.2)]}), 'is in two groups'),
        (dict(priors={'x': [PacePrior.driver(a, 11.0)]}), "scenario 'x'"),
        (dict(priors={'x': [PacePrior.driver(a, 0.01)] * 65}), 'at most 64 priors'),
        (dict(priors={'x': []}, edges=[0.1, 0.1]), 'edges must be finite and strictly increasing'),
        (dict(priors={'x': []}, edges=[nan]), 'edges must be finite and strictly increasing'),
        (dict(priors={'x': []}, edges=list(range(16))), 'edges: at most 15 values'),
        (dict(priors={}), '1 to 64 scenarios'),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            sim.run_priors(10, **kw, **_kw(c))


def test_zero_simulations_give_empty_counts_and_the_scenario_names():
    sim, c = _sim()
    names = list(c['grid_probs'])
    n = len(names)
    res = sim.run_priors(0, {'forecast': [], 'fp1': [PacePrior.driver(d, 0.15) for d in names]}, edges=[-0.1, 0.1],
                         strategies={'two-stop': []}, return_offsets=True, return_orders=True, **_kw(c))
    assert isinstance(res, PriorResult) and isinstance(res, StrategyResult)
    assert res.names == ['forecast', 'fp1', 'two-stop'] and res.drivers == names
    assert res.hist.shape == (3, n, n) and res.delta.shape == (3, n, 2 * n - 1) and res.draws.shape == (3, n, 3, n)
    assert res.offsets.shape == (3, 0, n) and res.offsets.dtype == np.float32 and res.orders.shape == (3, 0, n)
    assert list(res.edges) == [-0.1, 0.1]
    assert sim.run_priors(0, {'a': []}, **_kw(c)).offsets is None


def test_prior_result_on_hand_made_counts():
    drivers = ['A', 'B', 'C']
    draws = np.zeros((2, 3, 3, 3), np.int64)
    # scenario 1, driver A: 10 simulations in bin 0 (all wins), none in bin 1, 30 in bin 2 (10 each position)
    draws[1, 0, 0] = [10, 0, 0]
    draws[1, 0, 2] = [10, 10, 10]
    draws[1, 1, 1] = [0, 40, 0]
    draws[1, 2, 1] = [0, 0, 40]
    draws[0, :, 1] = np.eye(3, dtype=np.int64) * 40
    hist = draws.sum(axis=2)
    res = PriorResult(names=['base', 'drawn'], drivers=drivers, n_simulations=40, hist=hist,
                      delta=np.zeros((2, 3, 5), np.int64), draws=draws, edges=np.array([-0.1, 0.1]))
    assert res.bin_bounds(0) == (-math.inf, -0.1) and res.bin_bounds(1) == (-0.1, 0.1) and res.bin_bounds(2) == (0.1, math.inf)
    with pytest.raises(IndexError):
        res.bin_bounds(3)
    assert np.allclose(res.draw_probabilities('drawn', 'A'), [0.25, 0.0, 0.75])
    p = res.position_probabilities_by_draw('drawn', 'A')
    assert np.allclose(p[0], [1, 0, 0]) and np.isnan(p[1]).all() and np.allclose(p[2], [1 / 3] * 3)
    w = res.win_probability_by_draw('drawn', 'A')
    assert w[0] == 1.0 and math.isnan(w[1]) and abs(w[2] - 1 / 3) < 1e-12
    e = res.expected_points_by_draw('drawn', 'A', points=[25, 18, 15])
    assert e[0] == 25.0 and math.isnan(e[1]) and abs(e[2] - (25 + 18 + 15) / 3) < 1e-12
    assert res.win_probability('drawn', 'A') == 0.5
    with pytest.raises(KeyError):
        res.draw_probabilities('nope', 'A')
    with pytest.raises(KeyError):
        res.draw_probabilities('drawn', 'Z')


# ---------------------------------------------------------------- the command and the predictor's block
def test_command_parsing():
    from monte_carlo_gp_amd import uncertainty as U
    p = U.build_parser()
    a = p.parse_args(['--race', 'Bahrain', '--own', '0.15', '--own', 'VER:0.05', '--team', '0.2', '--edges=-0.2,0,0.2',
                      '--driver', 'VER', '--offline'])
    assert U.sigma_argument(a.own, '--own') == {'*': 0.15, 'VER': 0.05} and U.sigma_argument(a.team, '--team') == 0.2
    assert U.sigma_argument(None, '--own') is None and U.edges_argument(None) is None and U.edges_argument('') == []
    teams = {'VER': 'Red Bull', 'PER': 'Red Bull', 'NOR': 'McLaren'}
    arg = U.argument_of(a, ['VER', 'PER', 'NOR'], teams)
    assert arg == {'own': {'VER': 0.05, 'PER': 0.15, 'NOR': 0.15}, 'team': 0.2, 'edges': [-0.2, 0.0, 0.2]}
    a = p.parse_args(['--race', 'Bahrain', '--team', 'McLaren:0.3', '--offline'])
    assert U.argument_of(a, ['VER', 'PER', 'NOR'], teams) == {'team': {'McLaren': 0.3}}
    for bad in (['--own', 'x'], ['--own', 'VER:'], ['--own', '-0.1'], ['--own', '11'], ['--own', ':0.1'],
                ['--own', '0.1', '--own', '0.2'], ['--edges', '0.1,0.1'], ['--edges', 'a'], ['--edges', 'nan'],
                ['--edges', ','.join(str(i) for i in range(16))], []):
        with pytest.raises(SystemExit):
            U.main(['--race', 'Bahrain', '--offline', '--simulations', '0'] + bad)
    with pytest.raises(SystemExit):
        p.parse_args(['--own', '0.1'])                              # --race is required


def test_predictor_options_and_block_are_json_safe():
    from monte_carlo_gp_amd.predictor import DEFAULT_PACE_EDGES, pace_uncertainty_keys, pace_uncertainty_options
    drivers = ['A', 'B', 'C']
    teams = {'A': 'T1', 'B': 'T1', 'C': 'T2'}
    priors, edges = pace_uncertainty_options({'own': 0.15, 'team': {'T1': 0.2}}, drivers, teams)
    assert [(p.codes, p.sigma, p.shared) for p in priors] == [(('A',), 0.15, False), (('B',), 0.15, False),
                                                              (('C',), 0.15, False), (('A', 'B'), 0.2, True)]
    assert edges == list(DEFAULT_PACE_EDGES)
    priors, edges = pace_uncertainty_options({'own': {'C': 0.1}, 'edges': []}, drivers, teams)
    assert [(p.codes, p.sigma) for p in priors] == [(('C',), 0.1)] and edges == []
    for bad in ({}, {'edges': [0.1]}, {'own': {'Z': 0.1}}, {'team': {'T9': 0.1}}, {'sigma': 0.1}, 0.15):
        with pytest.raises(ValueError):
            pace_uncertainty_options(bad, drivers, teams)
    draws = np.zeros((2, 3, 3, 3), np.int64)
    draws[0, :, 1] = np.eye(3, dtype=np.int64) * 40
    draws[1, 0, 0] = [10, 0, 0]
    draws[1, 0, 2] = [10, 10, 10]
    draws[1, 1, 1] = [20, 20, 0]
    draws[1, 2, 1] = [0, 10, 30]
    delta = np.zeros((2, 3, 5), np.int64)
    delta[:, :, 2] = 40
    res = PriorResult(names=['forecast', 'uncertain'], drivers=drivers, n_simulations=40, hist=draws.sum(axis=2), delta=delta,
                      draws=draws, edges=np.array([-0.1, 0.1]))
    block = pace_uncertainty_keys(res)
    back = json.loads(json.dumps(block, allow_nan=False))            # no NaN, no infinity, no numpy scalar
    assert back == block
    assert block['bins'] == [[None, -0.1], [-0.1, 0.1], [0.1, None]] and block['edges'] == [-0.1, 0.1]
    a = block['drivers']['A']
    assert a['forecast']['win'] == 1.0 and a['uncertain']['win'] == 0.5
    assert a['by_draw']['share'] == [0.25, 0.0, 0.75] and a['by_draw']['win'][1] is None and a['by_draw']['win'][0] == 1.0
    assert a['by_draw']['expected_points'][1] is None and a['paired']['p_same'] == 1.0
