"""Pit-strategy comparison on the device (mcgp_run_strategies): an empty scenario is mcgp_run (or mcgp_run_from_state)
bit for bit; planning exactly the model's own stops changes nothing; plans that differ from the rule give the Python
restatement's finishing orders (strategy_ref); delta_out is the paired count of orders_out; counts are split-, shard-
and chunk-invariant; the `strategy` CLI runs end to end."""
import json

import numpy as np
import pytest

import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
from helpers import product_run
from monte_carlo_gp_amd import PitPlan, RaceConfig, RaceSimulator, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP

pytestmark = pytest.mark.gpu

GOLDEN = ['S60', 'S78', 'S50', 'N10', 'HET', 'EVT', 'DMP', 'WET']
SOFT, MEDIUM, HARD = 0, 1, 2


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


def _check(rc):
    assert rc == 0, N.lib().mcgp_last_error().decode()


@pytest.mark.parametrize('name', GOLDEN + ['n1', 'n2', 'n32'])
def test_empty_scenario_is_mcgp_run(require_gpu, name):
    case = _case(name)
    seed, m, off = 4242, 3000, 777
    hist, _, orders = product_run(case, m, seed, sim_offset=off, orders=True)
    rc, h, dl, o = SR.run_c(case, [{}, {}], m, seed, sim_offset=off)
    _check(rc)
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_strategy_kernel'
    for s in range(2):
        assert np.array_equal(o[s], orders) and np.array_equal(h[s], hist)
    n = len(case['grid_probs'])
    assert (dl[:, :, n - 1] == m).all() and dl.sum() == 2 * m * n


def test_empty_scenario_from_a_state_is_mcgp_run_from_state(require_gpu):
    case = O.load_case('EVT')
    seed = 9
    ref = RR.traced_run(case, 4, seed)
    L = case['config']['total_laps']
    for k in (1, L // 2, L):
        st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, seed, 2, k))
        rc, hist, orders = RR.run_c(RR.problem(case), [st], 5000, [123], seed)
        _check(rc)
        rc, h, _, o = SR.run_c(case, [{}], 5000, seed, sim_offset=123, state=st)
        _check(rc)
        assert np.array_equal(o[0], orders[0]) and np.array_equal(h[0], hist[0])


def _quiet(case, n=None):
    """The case without race events and with a one-hot grid (driver d on slot d): every car's rule stops are fixed."""
    c = dict(case)
    c['config'] = dict(case['config'], sc_probability=0.0, vsc_probability=0.0, red_flag_probability=0.0)
    drivers = list(case['grid_probs'])
    c['grid_probs'] = {d: [1.0 if j == i else 0.0 for j in range(len(drivers))] for i, d in enumerate(drivers)}
    return c


@pytest.mark.parametrize('name', ['S60', 'HET', 'n32'])
def test_planning_the_rules_own_stops_changes_nothing(require_gpu, name):
    case = _quiet(_case(name))
    n = len(case['grid_probs'])
    stops = SR.rule_stops(case, list(range(n)))
    assert any(stops.values())
    every = {d: (-1, 0, stops[d]) for d in range(n)}
    subset = {d: (-1, 0, stops[d]) for d in range(0, n, 3)}
    m, seed = 4000, 31
    _, hist, orders = product_run(case, m, seed, orders=True)
    rc, h, dl, o = SR.run_c(case, [{}, every, subset], m, seed)
    _check(rc)
    for s in range(3):
        assert np.array_equal(o[s], orders), s
        assert np.array_equal(h[s], h[0])
    assert (dl[:, :, n - 1] == m).all()
    # and a plan that differs from the rule does change the race
    d0 = next(d for d in range(n) if stops[d])
    moved = {d0: (-1, 0, [(min(stops[d0][0][0] + 3, case['config']['total_laps']), stops[d0][0][1])])}
    rc, _, _, o2 = SR.run_c(case, [{}, moved], m, seed)
    _check(rc)
    assert not np.array_equal(o2[1], orders)


def _plans(case, L, n):
    """Plans that differ from the rule, for drivers 0, 1 and n - 1."""
    return [
        {},
        {0: (-1, 0, [(8, HARD)])},                                         # an early single stop
        {1: (-1, 0, [(15, MEDIUM), (L - 5, SOFT)]), 0: (-1, 0, [])},       # two stops; a driver who never stops
        {n - 1: (HARD, 2, [(L // 2, SOFT)])},                              # a start-compound override
        {0: (-1, 0, [(L, SOFT)]), 1: (SOFT, 0, [(2, MEDIUM), (L, HARD)])},  # stops on lap 2 and on lap L
    ]


@pytest.mark.parametrize('name', ['S60', 'EVT', 'n32'])
def test_device_equals_the_restatement(require_gpu, name):
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    seed, m = 55, 160
    ref = RR.traced_run(case, m, seed, 400)
    scen = _plans(case, L, n)
    rc, h, dl, o = SR.run_c(case, scen, m, seed, sim_offset=400)
    _check(rc)
    assert np.array_equal(o[0], ref['orders'])
    for s, plans in enumerate(scen):
        want = SR.orders(case, m, seed, 400, plans=plans, grids=ref['grids'])
        bad = [i for i in range(m) if not np.array_equal(o[s, i], want[i])]
        assert not bad, f'scenario {s}: {len(bad)} of {m} orders differ, first sim {bad[0]}'
        assert np.array_equal(h[s], RR.counts(o[s], n))
    assert np.array_equal(dl, SR.delta_counts(o, n))


def test_stops_on_red_flag_laps_and_around_retirements(require_gpu):
    """EVT: a stop on the lap of a red flag (the free tyre change first, then the planned stop); a planned car that
    retires before, or on, its stop lap (no stop)."""
    case = _case('EVT')
    seed, m = 77, 100
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    cfg = case['config']
    red = []
    for i in range(m):
        for lap in range(2, L + 1):
            e = O.philox([i, 0, lap, RR.PURPOSE_EVENT], [seed, 0])
            if e[0] < RR.threshold(cfg['red_flag_probability']):
                red.append((i, lap))
                break
    assert red, 'no red flag in these simulations'
    prob = RR.problem(case)
    outs = []
    for i in range(m):
        for d in range(n):
            w = O.philox([i, 0, 0, RR.PURPOSE_RETIRE | (d >> 2)], [seed, 0])[d & 3]
            r = RR.retirement_lap(int(w), RR.threshold(float(prob.arrays['lap_dnf'][d])), L)
            if r >= 3:
                outs.append((i, d, r))
    assert outs, 'no retirement in these simulations'
    ref = RR.traced_run(case, m, seed)
    scen = [{}]
    for i, lap in red[:4]:
        scen.append({d: (-1, 0, [(lap, HARD)]) for d in range(0, n, 4)})
    for i, d, r in outs[:4]:
        scen.append({d: (-1, 0, [(r - 1, HARD), (r, SOFT)])})          # before, and on, its retirement lap
        scen.append({d: (-1, 0, [(r, MEDIUM)])})
    rc, h, dl, o = SR.run_c(case, scen, m, seed)
    _check(rc)
    for s, plans in enumerate(scen):
        want = SR.orders(case, m, seed, plans=plans, grids=ref['grids'])
        assert np.array_equal(o[s], want), s


@pytest.mark.parametrize('name', ['S60', 'EVT'])
def test_plans_from_a_state_equal_the_restatement(require_gpu, name):
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    k = min(30, L - 4)
    seed, m = 21, 120
    ref = RR.traced_run(case, 3, seed)
    st = (RR.state_arrays(ref, 1, k), k, RR.drs_disabled_until(case, seed, 1, k))
    scen = [{}, {0: (-1, 0, [(k + 1, SOFT)])}, {1: (-1, 0, [(k + 2, HARD), (L, SOFT)]), 2: (-1, 0, [])}]
    rc, h, dl, o = SR.run_c(case, scen, m, seed, sim_offset=50, state=st)
    _check(rc)
    for s, plans in enumerate(scen):
        want = SR.orders(case, m, seed, 50, plans=plans, state=st)
        assert np.array_equal(o[s], want), s
    assert np.array_equal(dl, SR.delta_counts(o, n))


def test_counts_are_split_shard_and_chunk_invariant(require_gpu):
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    scen = _plans(case, L, n)
    seed, m = 8, 60_000
    rc, h, dl, o = SR.run_c(case, scen, m, seed)
    _check(rc)
    assert np.array_equal(dl, SR.delta_counts(o, n))
    a = 21_111
    rc1, h1, d1, _ = SR.run_c(case, scen, a, seed, orders=False)
    rc2, h2, d2, o2 = SR.run_c(case, scen, m - a, seed, sim_offset=a)
    _check(rc1)
    _check(rc2)
    assert np.array_equal(h1 + h2, h) and np.array_equal(d1 + d2, dl) and np.array_equal(o2, o[:, a:])
    # through the Python layer, sharded over two devices (or twice over device 0)
    sim = RaceSimulator(RaceConfig(**case['config']), device=[0, min(1, require_gpu - 1)], set_pop=DEFAULT_SET_POP)
    drivers = list(case['grid_probs'])
    strategies = {f's{s}': [PitPlan(drivers[d], [(lap, N.COMPOUNDS[c]) for lap, c in stops],
                                    start=None if st < 0 else N.COMPOUNDS[st], start_age=age)
                            for d, (st, age, stops) in plans.items()] for s, plans in enumerate(scen)}
    res = sim.run_strategies(m, strategies, case['base_pace'], case['tire_deg'], case['driver_variance'],
                             case['driver_dnf_rates'], grid_probs=case['grid_probs'], seed=seed,
                             track_condition=case['track_condition'], allow_single_compound=True)
    assert np.array_equal(res.hist, h) and np.array_equal(res.delta, dl)
    c = res.compare('s1', drivers[0])
    assert 0 < c['se'] and c['p_better'] + c['p_same'] + c['p_worse'] == pytest.approx(1.0)


def test_a_run_that_crosses_a_staging_chunk(require_gpu):
    """64 scenarios of a 32-car field: the staging budget (256 MiB / (S n)) holds 131072 simulations; 140000 take two
    chunks and give what two calls inside one chunk give."""
    case = _case('n32')
    L, n = case['config']['total_laps'], 32
    base = _plans(case, L, n)
    scen = [base[s % len(base)] for s in range(64)]
    m, seed = 140_000, 3
    assert (256 << 20) // (64 * n) < m
    rc, h, dl, _ = SR.run_c(case, scen, m, seed, orders=False)
    _check(rc)
    rc1, h1, d1, _ = SR.run_c(case, scen, 70_000, seed, orders=False)
    rc2, h2, d2, _ = SR.run_c(case, scen, m - 70_000, seed, sim_offset=70_000, orders=False)
    _check(rc1)
    _check(rc2)
    assert np.array_equal(h1 + h2, h) and np.array_equal(d1 + d2, dl)
    for s in range(64):
        assert np.array_equal(h[s], h[s % len(base)])
    assert h[0].sum() == m * n


def test_strategy_cli_end_to_end(require_gpu, tmp_path, capsys):
    out, pred = tmp_path / 's.json', tmp_path / 'p.json'
    seed, m = 7, 20_000
    assert cli.main(['predict', '--race', 'Bahrain', '--offline', '--simulations', str(m), '--seed', str(seed),
                     '--json', str(pred)]) == 0
    win = json.load(open(pred))['win_probabilities']
    driver = max(win, key=win.get)
    assert cli.main(['strategy', '--race', 'Bahrain', '--offline', '--driver', driver, '--plan', 'early=:12/HARD',
                     '--plan', 'two=:15/MEDIUM,40/HARD', '--window', '20-22/HARD', '--simulations', str(m), '--seed',
                     str(seed), '--json', str(out)]) == 0
    text = capsys.readouterr().out
    assert 'early' in text and f'{driver} L21' in text
    rows = json.load(open(out))['scenarios']
    assert [r['scenario'] for r in rows] == ['model', 'early', 'two', f'{driver} L20', f'{driver} L21', f'{driver} L22']
    model = rows[0]['win_probabilities']
    assert set(model) == set(win)
    for d in win:
        assert model[d] == pytest.approx(win[d], abs=1e-12)
    assert rows[0]['p_same'] == 1.0 and rows[0]['mean_gain'] == 0.0
