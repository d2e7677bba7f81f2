"""Pace uncertainty on the device (mcgp_run_priors, through the C ABI) against the references of
tests/test_priors_host_build.py -- the drawn offsets from the oracle's Philox and inverse-normal, bit for bit; every
simulation's finishing order from the pinned C oracle under base_pace[d] + float(x_d(i)), and from a state from paces_ref's
restatement -- against mcgp_run_paces, the existing kernel doing the same additions, one simulation at a time, and against
itself: the count outputs are accumulated into, a split by sim_offset sums to the one call, several staging chunks equal
one.  Then the 100 inputs of generic_cases.run_inputs(), and RaceSimulator.run_priors, the predictor's block and the
`uncertainty` command end to end."""
import numpy as np
import pytest

import oracle_py as O
import paces_ref as PR
import priors_ref as QR
import resume_ref as RR
import strategy_ref as SR
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

KERNEL = 'mcgp::race_priors_kernel'
SEED, OFF = 47, 300
EDGES = QR.SWEEP_EDGES


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(case, scen, m, seed, off=0, edges=EDGES, plans=None, **kw):
    got = QR.run_c(case, plans, scen, edges, m, seed, sim_offset=off, **kw)
    assert got['rc'] == 0, N.lib().mcgp_last_error().decode()
    if m:
        assert N.lib().mcgp_last_kernel_name(0).decode() == KERNEL
    return got


@pytest.mark.parametrize('n', [1, 2, 5, 32])
def test_offsets_are_the_reference_bit_for_bit(require_gpu, n):
    case = RR.field_case(n)
    items = QR.sweep_items(n)
    for seed, off in ((SEED, OFF), (SEED, 2 ** 32 - 3), (0x9E3779B97F4A7C15, 5)):
        got = _run(case, [[], items], 8, seed, off)
        want = QR.offsets(items, n, 8, seed, off)
        assert np.array_equal(_bits(got['offsets'][1]), _bits(want)), (seed, off)
        assert not _bits(got['offsets'][0]).any()


@pytest.mark.parametrize('name,m', [('S60', 64), ('EVT', 64), ('N10', 64), ('n32', 16), ('n2', 16), ('n1', 16)])
def test_every_simulation_is_the_oracle_under_its_drawn_base_pace(require_gpu, name, m):
    case = _case(name)
    n, L = len(case['grid_probs']), case['config']['total_laps']
    items = QR.sweep_items(n)
    got = _run(case, [[], items], m, SEED, OFF)
    x = QR.offsets(items, n, m, SEED, OFF)
    assert np.array_equal(_bits(got['offsets'][1]), _bits(x))
    base = O.Problem(case).run(m, rng=O.RNG_PHILOX, seed=SEED, sim_offset=OFF, want_orders=True)['orders']
    want = QR.orders(case, items, m, SEED, OFF, x=x)
    both, xs = np.stack([base, want]), np.stack([np.zeros_like(x), x])
    bad = [i for i in range(m) if not np.array_equal(got['orders'][1, i], want[i])]
    assert not bad, f'{len(bad)} of {m} orders differ, first sim {bad[0]}'
    assert np.array_equal(got['orders'][0], base)
    assert np.array_equal(got['hist'], PR.hist_counts(both, n))
    assert np.array_equal(got['delta'], SR.delta_counts(both, n))
    assert np.array_equal(got['draws'], QR.draw_counts(both, xs, EDGES))
    # from states after laps 1, L // 2 and L - 1
    ref = RR.traced_run(case, 4, SEED, OFF)
    for k in sorted({1, L // 2, L - 1}):
        state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFF + 3, k))
        got = _run(case, [[], items], 16, SEED, OFF, state=state)
        assert np.array_equal(_bits(got['offsets'][1]), _bits(x[:16]))
        assert np.array_equal(got['orders'][1], QR.orders(case, items, 16, SEED, OFF, state=state, x=x)), k
        assert np.array_equal(got['orders'][0], PR.orders(case, 16, SEED, OFF, state=state)[0]), k


def test_one_by_one_against_the_paces_call_under_the_drawn_offsets(require_gpu):
    """mcgp_run_paces with a LAPS offset [first, L] of x_d(i) on every driver is the existing kernel doing the same
    additions."""
    case = _case('S60')
    n, L = len(case['grid_probs']), case['config']['total_laps']
    items = QR.sweep_items(n)
    got = _run(case, [items], 16, SEED, OFF)
    ref = RR.traced_run(case, 4, SEED, OFF)
    k = L // 2
    state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFF + 3, k))
    got_state = _run(case, [items], 16, SEED, OFF, state=state)
    for i in range(16):
        x = got['offsets'][0, i]
        rc, _, _, _, o = PR.run_c(case, None, [[PR.laps(d, 1, L, float(x[d])) for d in range(n)]], 1, SEED, OFF + i)
        assert rc == 0 and np.array_equal(o[0, 0], got['orders'][0, i]), i
        rc, _, _, _, o = PR.run_c(case, None, [[PR.laps(d, k + 1, L, float(x[d])) for d in range(n)]], 1, SEED, OFF + i,
                                  state=state)
        assert rc == 0 and np.array_equal(o[0, 0], got_state['orders'][0, i]), i


def test_split_calls_chunks_and_prefilled_outputs(require_gpu, monkeypatch):
    case = _case('S60')
    n = len(case['grid_probs'])
    scen = [[], QR.sweep_items(n), [QR.group(range(n), 0.3)]]
    m = 1000
    whole = _run(case, scen, m, SEED, OFF)
    assert np.array_equal(whole['hist'], PR.hist_counts(whole['orders'], n))
    assert np.array_equal(whole['delta'], SR.delta_counts(whole['orders'], n))
    assert np.array_equal(whole['draws'], QR.draw_counts(whole['orders'], whole['offsets'], EDGES))
    assert (whole['draws'].sum(axis=(2, 3)) == m).all()
    a, b = _run(case, scen, 389, SEED, OFF, fill=7), _run(case, scen, 611, SEED, OFF + 389)
    for key in ('hist', 'delta', 'draws'):
        assert np.array_equal(whole[key], a[key] - 7 + b[key]), key
    assert np.array_equal(whole['orders'], np.concatenate([a['orders'], b['orders']], axis=1))
    assert np.array_equal(_bits(whole['offsets']), _bits(np.concatenate([a['offsets'], b['offsets']], axis=1)))
    # several launches of a chunk each, and outputs that are not wanted
    monkeypatch.setenv('MCGP_MAX_SIMS_PER_LAUNCH', '300')
    parts = _run(case, scen, m, SEED, OFF)
    for key in ('hist', 'delta', 'draws', 'orders'):
        assert np.array_equal(whole[key], parts[key]), key
    assert np.array_equal(_bits(whole['offsets']), _bits(parts['offsets']))
    bare = _run(case, scen, m, SEED, OFF, orders=False, delta=False, draws=False, offsets=False)
    assert np.array_equal(bare['hist'], whole['hist']) and not bare['delta'].any() and not bare['draws'].any()


def test_sixty_four_scenarios_fifteen_edges_and_no_edges(require_gpu):
    n = 32
    case = RR.field_case(n)
    scen = [[QR.driver(d, 0.01 * ((s + d) % 40)) for d in range(n)] + [QR.group([(d + s) % n], 0.02 * ((s * 7 + d) % 11))
                                                                          for d in range(n)] for s in range(64)]
    edges = tuple(-0.35 + 0.05 * i for i in range(15))
    m = 70                                                          # a ragged wave
    got = _run(case, scen, m, SEED, 9, edges=edges)
    for s in (0, 1, 31, 63):
        x = QR.offsets(scen[s], n, m, SEED, 9)
        assert np.array_equal(_bits(got['offsets'][s]), _bits(x)), s
        assert np.array_equal(got['orders'][s, :4], QR.orders(case, scen[s], 4, SEED, 9, x=x)), s
    assert np.array_equal(got['draws'], QR.draw_counts(got['orders'], got['offsets'], edges))
    assert np.array_equal(got['delta'], SR.delta_counts(got['orders'], n))
    none = _run(case, scen[:2], m, SEED, 9, edges=())
    assert np.array_equal(none['draws'][:, :, 0, :], none['hist']) and np.array_equal(none['orders'], got['orders'][:2])


def test_a_thousand_laps_and_one_lap(require_gpu):
    case = RR.field_case(2)
    case['config'] = dict(case['config'], total_laps=1000)
    items = QR.sweep_items(2)
    got = _run(case, [[], items], 4, SEED, 1)
    assert np.array_equal(got['orders'][1], QR.orders(case, items, 4, SEED, 1))
    case = RR.field_case(5)
    case['config'] = dict(case['config'], total_laps=1)
    items = [QR.driver(d, 1.5) for d in range(5)] + [QR.group([0, 4], 1.0)]
    got = _run(case, [[], items], 32, SEED, 5)
    assert np.array_equal(got['orders'][1], QR.orders(case, items, 32, SEED, 5))
    assert not np.array_equal(got['orders'][1], got['orders'][0])


def test_device_on_every_input(require_gpu):
    QR.check_sweep(lambda case, seed, scen: _run(case, scen, QR.SWEEP_SIMS, seed, QR.SWEEP_OFFSET))


def test_python_layer_predictor_block_and_command(require_gpu, tmp_path, capsys):
    import json

    from monte_carlo_gp_amd import PacePrior, RaceConfig, RaceSimulator, uncertainty
    from monte_carlo_gp_amd.cli import synthetic_fixture
    from monte_carlo_gp_amd.predictor import F1Predictor
    case = _case('S60')
    names = list(case['grid_probs'])
    n, m = len(names), 512
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=O.load_cases()['set_pop'])
    priors = [PacePrior.driver(d, 0.15) for d in names] + [PacePrior.group(names[i:i + 2], 0.2) for i in range(0, n, 2)]
    res = sim.run_priors(m, {'forecast': [], 'uncertain': priors}, EDGES, None, case['base_pace'], case['tire_deg'],
                         case['driver_variance'], case['driver_dnf_rates'], grid_probs=case['grid_probs'], seed=SEED,
                         sim_offset=OFF, return_orders=True, return_offsets=True)
    want = _run(case, [[], QR.sweep_items(n)], m, sim._resolve_seed(SEED), OFF)
    for key in ('hist', 'delta', 'draws', 'orders'):
        assert np.array_equal(getattr(res, key), want[key]), key
    assert np.array_equal(_bits(res.offsets), _bits(want['offsets']))
    assert np.allclose(res.draw_probabilities('uncertain', names[0]).sum(), 1.0)
    c = res.compare('uncertain', names[0])
    assert abs(c['p_better'] + c['p_same'] + c['p_worse'] - 1.0) < 1e-12 and c['p_same'] < 1.0
    # the predictor's block beside the forecast it belongs to, and the command end to end
    fixture = synthetic_fixture()
    p = F1Predictor()
    plain = p.predict_weekend(2024, 'Bahrain', fixture, n_simulations=2000, seed=7)
    both = p.predict_weekend(2024, 'Bahrain', fixture, n_simulations=2000, seed=7, pace_uncertainty={'own': 0.15, 'team': 0.2})
    assert both['win_probabilities'] == plain['win_probabilities']
    block = both['pace_uncertainty']
    assert json.loads(json.dumps(block, allow_nan=False)) == block and block['n_simulations'] == 2000
    for d, row in block['drivers'].items():
        assert abs(row['forecast']['win'] - plain['win_probabilities'][d]) < 1e-12, d
    out = tmp_path / 'u.json'
    rc = uncertainty.main(['--race', 'Bahrain', '--season', '2024', '--offline', '--simulations', '2000', '--seed', '7', '--own',
                           '0.15', '--team', '0.2', '--driver', fixture['drivers'][0], '--json', str(out)])
    assert rc == 0 and 'PACE UNCERTAINTY' in capsys.readouterr().out
    assert json.loads(out.read_text())['pace_uncertainty'] == block
