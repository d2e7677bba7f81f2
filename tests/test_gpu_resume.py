"""In-race odds on the device (mcgp_run_from_state): a state the CPU oracle traced for simulation i after lap k,
resumed as simulation i, must finish in the oracle's order of i, bit for bit; many simulations from one state are
split-, shard- and launch-invariant; a car observed running after lap k retires by the per-lap chain from lap k + 1."""
import dataclasses
import json

import numpy as np
import pytest

import oracle_py as O
import resume_ref as RR
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.predictor import F1Predictor
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP

pytestmark = pytest.mark.gpu

CASES = ['S60', 'S78', 'N10', 'HET', 'EVT', 'DMP', 'WET', 'n1', 'n2', 'n32']


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


def _seed(name, case):
    return int(case.get('seed', 0)) if name[0] != 'n' else 70 + int(name[1:])


def _resume_all(case, ref, laps, seed, sim_offset):
    """One call: state i = traced simulation i after laps[i], resumed as simulation sim_offset + i."""
    m, n = ref['orders'].shape
    states = [(RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, sim_offset + i, k))
              for i, k in enumerate(laps)]
    rc, hist, orders = RR.run_c(RR.problem(case), states, 1, sim_offset + np.arange(m), seed)
    assert rc == 0, N.lib().mcgp_last_error()
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_resume_kernel'
    bad = [i for i in range(m) if not np.array_equal(orders[i, 0], ref['orders'][i])]
    assert not bad, f'laps {sorted(set(laps))}: {len(bad)} of {m} continuations differ from the oracle, first sim {bad[0]}'
    for i in range(m):
        assert np.array_equal(hist[i], RR.counts(orders[i], n))


@pytest.mark.parametrize('name', CASES)
def test_continuation_equals_the_oracle(require_gpu, name):
    case = _case(name)
    seed = _seed(name, case)
    sim_offset = 98765 if name == 'WET' else 0
    m = 96 if name == 'EVT' else 64
    ref = RR.traced_run(case, m, seed, sim_offset)
    L = case['config']['total_laps']
    for k in sorted({k for k in (1, 2, 3, L // 2, L - 1, L) if 1 <= k <= L}):
        _resume_all(case, ref, [k] * m, seed, sim_offset)
    # each simulation from the lap of its first race event (where drs_disabled_until matters), and the lap after it
    first = [RR.first_event_lap(case, seed, sim_offset + i) or L // 2 for i in range(m)]
    _resume_all(case, ref, first, seed, sim_offset)
    _resume_all(case, ref, [min(L, k + 1) for k in first], seed, sim_offset)


def test_python_continuation_equals_run_monte_carlo(require_gpu):
    """RaceSimulator.run_from_state with run_monte_carlo's driver order: simulation i continues into that run's order."""
    case = O.load_case('S60')
    seed, m, k = 42, 48, 25
    drivers = list(case['grid_probs'])
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=O.load_cases()['set_pop'])
    args = (case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    _, full = sim.run_monte_carlo(m, case['grid_probs'], *args, seed=seed, track_condition='dry', return_orders=True)
    ref = RR.traced_run(case, m, seed)
    states = [RR.race_state(RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, i, k), drivers)
              for i in range(m)]
    probs, orders = sim.run_from_state(1, states, *args, seed=seed, track_condition='dry', sim_offset=list(range(m)),
                                       drivers=drivers, return_orders=True)
    assert orders.shape == (m, 1, 20) and np.array_equal(orders[:, 0], full)
    assert len(probs) == m and sim.last_histogram.shape == (m, 20, 20)
    one = sim.run_from_state(1, states[7], *args, seed=seed, sim_offset=7, drivers=drivers)
    assert {d: p for d, p in one.items() if p} == {drivers[int(d)]: {pos + 1: 1.0} for pos, d in enumerate(full[7])}


@pytest.fixture(scope='module')
def one_state():
    case = O.load_case('S60')
    seed = 42
    ref = RR.traced_run(case, 8, seed)
    k = 30
    st = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, seed, 3, k))
    return case, seed, st


def test_many_simulations_from_one_state(require_gpu, one_state, monkeypatch):
    case, seed, st = one_state
    prob = RR.problem(case)
    N_SIMS = 100_000
    rc, hist, orders = RR.run_c(prob, [st], N_SIMS, [0], seed)
    assert rc == 0
    assert np.array_equal(hist[0], RR.counts(orders[0], 20))
    assert hist[0].sum() == N_SIMS * 20
    ids = np.random.default_rng(1).choice(N_SIMS, 64, replace=False)
    for i in ids[:8]:
        rc, _, o = RR.run_c(prob, [st], 1, [int(i)], seed)
        assert rc == 0 and np.array_equal(o[0, 0], orders[0, i])
    rc, _, o = RR.run_c(prob, [st] * 64, 1, ids, seed)                # the 64 ids as 64 states of one call
    assert rc == 0 and np.array_equal(o[:, 0], orders[0, ids])
    # splits of [0, N) over calls
    a = 37_123
    rc1, h1, _ = RR.run_c(prob, [st], a, [0], seed, orders=False)
    rc2, h2, _ = RR.run_c(prob, [st], N_SIMS - a, [a], seed, orders=False)
    assert rc1 == 0 and rc2 == 0 and np.array_equal(h1 + h2, hist)
    # three identical states: three identical histograms
    rc, h3, o3 = RR.run_c(prob, [st] * 3, N_SIMS, [0, 0, 0], seed)
    assert rc == 0 and all(np.array_equal(h3[s], hist[0]) for s in range(3))
    assert all(np.array_equal(o3[s], orders[0]) for s in range(3))
    # several launches per state
    monkeypatch.setenv('MCGP_MAX_SIMS_PER_LAUNCH', '30000')
    rc, h4, o4 = RR.run_c(prob, [st] * 2, N_SIMS, [0, 0], seed)
    assert rc == 0 and np.array_equal(h4[0], hist[0]) and np.array_equal(h4[1], hist[0])
    assert np.array_equal(o4[1], orders[0])
    rc, h5, _ = RR.run_c(prob, [st], N_SIMS, [0], seed, orders=False)
    assert rc == 0 and np.array_equal(h5[0], hist[0])
    monkeypatch.delenv('MCGP_MAX_SIMS_PER_LAUNCH')
    # sharded over device=[0, 0, 0] through the Python layer
    drivers = list(case['grid_probs'])
    state = RR.race_state(st[0], st[1], st[2], drivers)
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=O.load_cases()['set_pop'], device=[0, 0, 0])
    sim.run_from_state(N_SIMS, state, case['base_pace'], case['tire_deg'], case['driver_variance'],
                       case['driver_dnf_rates'], seed=seed, track_condition='dry', drivers=drivers)
    assert np.array_equal(sim.last_histogram, hist[0])


def _duel(n_extra=0):
    """Two cars, 60 laps, no race events: A slow and never retiring, B 30 s ahead and retiring with p = 0.02 a lap."""
    base = O.load_case('S60')
    drivers = ['A', 'B'] + [f'R{i}' for i in range(n_extra)]
    cfg = dict(base['config'], total_laps=60, sc_probability=0.0, vsc_probability=0.0, red_flag_probability=0.0,
               driver_teams={d: 'T' for d in drivers}, dnf_rates={'T': 0.0})
    case = dict(base, config=cfg, track_condition='dry',
                grid_probs={d: [1.0 / len(drivers)] * len(drivers) for d in drivers},
                base_pace=dict({'A': 100.0, 'B': 90.0}, **{d: 95.0 for d in drivers[2:]}),
                tire_deg={d: 0.05 for d in drivers}, driver_variance={d: 0.15 for d in drivers},
                driver_dnf_rates=dict({'A': 0.0, 'B': 0.02}, **{d: 0.0 for d in drivers[2:]}))
    return case, drivers


def _car(cum, last, slot, retired=0):
    return dict(cum=cum, last=last, slot=slot, retired=retired)


def _arrays(cars):
    n = len(cars)
    return dict(cumulative_time=np.array([c['cum'] for c in cars], np.float64),
                last_lap_time=np.array([c['last'] for c in cars], np.float64),
                grid_slot=np.array([c['slot'] for c in cars], np.uint8), compound=np.full(n, 1, np.uint8),
                used_compounds=np.full(n, 0b010, np.uint8), tire_age=np.full(n, 10, np.int16),
                retired_lap=np.array([c['retired'] for c in cars], np.int16))


def test_conditional_retirement_law(require_gpu):
    case, drivers = _duel()
    k, L, N_SIMS = 20, 60, 1_000_000
    st = _arrays([_car(2000.0, 100.0, 1), _car(1970.0, 90.0, 0)])
    rc, hist, _ = RR.run_c(RR.problem(case), [(st, k, 0)], N_SIMS, [0], 2024, orders=False)
    assert rc == 0
    h = hist[0]
    assert h[0, 0] + h[1, 0] == N_SIMS and h[1, 1] + h[1, 0] == N_SIMS
    # B is classified 2nd exactly when it retires after lap 20: its draw says lap 21 .. 60, or it said 2 .. 20 (the
    # state contradicts that) and the chain shifted to lap 21 retires it by lap 60
    t = RR.threshold(0.02)
    q = 2 ** 32 - t
    S = {2: q}
    for j in range(3, L + 1):
        S[j] = (S[j - 1] * q) >> 32
    p_late = (S[k] - S[L]) / 2 ** 32
    p_stale = 1 - S[k] / 2 ** 32
    p = p_late + p_stale * (1 - S[L - k + 1] / 2 ** 32)
    se = (p * (1 - p) / N_SIMS) ** 0.5
    got = h[1, 1] / N_SIMS
    assert abs(got - p) < 5 * se, (got, p, se)
    assert abs(p - (1 - 0.98 ** 40)) < 1e-3 and abs(p - 0.554) < 0.002
    # the raw draw alone (no redraw) would give P(draw in 21 .. 60) ~ 0.378: far outside
    assert abs(got - p_late) > 100 * se


def test_retired_cars_stay_retired_and_classify_by_lap_and_time(require_gpu):
    case, drivers = _duel(n_extra=4)
    case['driver_dnf_rates']['B'] = 0.0
    cars = [_car(2000.0, 100.0, 5), _car(1900.0, 90.0, 0),
            _car(450.0, 95.0, 2, retired=5),       # R0
            _car(1100.0, 95.0, 3, retired=12),     # R1
            _car(1150.0, 95.0, 4, retired=12),     # R2
            _car(450.0, 95.0, 1, retired=5)]       # R3: R0's lap and time, the lower grid slot
    rc, hist, orders = RR.run_c(RR.problem(case), [(_arrays(cars), 20, 0)], 2000, [0], 9)
    assert rc == 0
    want = [1, 0, 4, 3, 5, 2]                      # B, A; then (lap, time) descending: R2, R1, then R3 before R0
    assert (orders[0] == np.array(want, np.uint8)).all()
    assert hist[0][want, np.arange(6)].tolist() == [2000] * 6


def _cli_state(tmp_path, k=30, seed=5):
    """A state file of the race `cli in-race --race Bahrain --offline` runs, traced by the oracle for simulation 0."""
    inp = F1Predictor().simulator_inputs(cli.synthetic_fixture(), 'Bahrain')
    cfg = dataclasses.asdict(inp['config'])
    case = dict(config=cfg, grid_probs=inp['grid_probs'], base_pace=inp['base_pace'], tire_deg=inp['tire_deg'],
                driver_variance=inp['driver_variance'], driver_dnf_rates=inp['driver_dnf_rates'],
                track_condition=inp['track_condition'])
    ref = O.Problem(case, set_pop=DEFAULT_SET_POP).run(1, rng=O.RNG_PHILOX, seed=seed, want_orders=True,
                                                       want_grids=True, n_trace=1)
    drivers = list(case['grid_probs'])
    state = RR.race_state(RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, 0, k), drivers)
    path = tmp_path / f'lap{k}.json'
    path.write_text(json.dumps(state.to_json()))
    return path, [drivers[d] for d in ref['orders'][0]]


def test_in_race_cli_end_to_end(require_gpu, tmp_path, capsys):
    path, finish = _cli_state(tmp_path)
    base = ['in-race', '--race', 'Bahrain', '--season', '2024', '--offline', '--seed', '5']
    one, two, single = tmp_path / 'one.json', tmp_path / 'two.json', tmp_path / 'single.json'
    assert cli.main(base + ['--simulations', '20000', '--state', str(path), '--json', str(one)]) == 0
    out = capsys.readouterr().out
    assert 'RACE WINNER PROBABILITIES' in out and 'after lap 30' in out
    assert cli.main(base + ['--simulations', '20000', '--state', str(path), '--state', str(path), '--json', str(two)]) == 0
    r1, r2 = json.loads(one.read_text()), json.loads(two.read_text())
    assert len(r1) == 1 and len(r2) == 2
    assert r2[0]['win_probabilities'] == r2[1]['win_probabilities'] == r1[0]['win_probabilities']
    assert r2[0]['podium_probabilities'] == r2[1]['podium_probabilities']
    assert abs(sum(r1[0]['win_probabilities'].values()) - 1.0) < 1e-9
    # one simulation: simulation 0 continues into the oracle's finishing order of simulation 0
    assert cli.main(base + ['--simulations', '1', '--state', str(path), '--json', str(single)]) == 0
    r = json.loads(single.read_text())[0]
    assert r['win_probabilities'][finish[0]] == 1.0
    assert {d for d, p in r['podium_probabilities'].items() if p == 1.0} == set(finish[:3])
