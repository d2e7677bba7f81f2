"""Head-to-head and podium counts on the device (mcgp_run_matchups) against matchups_ref fed with the CPU oracle's
finishing orders, or with the product's own run_monte_carlo(return_orders=True) orders: every count equal."""
import copy
import ctypes as C
import json

import numpy as np
import pytest

import matchups_ref as MR
import oracle_py as O
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, cli
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

SET_POP = O.load_cases()['set_pop']


def _sim(case, deviates=32, device=0):
    return RaceSimulator(RaceConfig(**case['config']), set_pop=SET_POP, deviates=deviates, device=device)


def _args(case):
    return (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])


def _run(case, n_sims, seed, sim_offset=0, deviates=32, podiums=True, device=0):
    return _sim(case, deviates, device).run_matchups(n_sims, *_args(case), seed=seed,
                                                     track_condition=case['track_condition'], sim_offset=sim_offset,
                                                     podiums=podiums)


def _identities(res):
    n, s = len(res.drivers), res.n_simulations
    a = res.ahead
    assert not np.diag(a).any()
    off = ~np.eye(n, dtype=bool)
    assert ((a + a.T)[off] == s).all()
    assert (res.hist.sum(axis=0) == s).all() and (res.hist.sum(axis=1) == s).all()
    if res.podium is not None:
        assert res.podium.sum() == s
        assert np.array_equal(res.podium.sum(axis=(1, 2)), res.hist[:, 0])
        assert np.array_equal(res.podium.sum(axis=(0, 2)), res.hist[:, 1])
        assert np.array_equal(res.podium.sum(axis=(0, 1)), res.hist[:, 2])


def _equals_orders(res, orders):
    h, a, p = MR.matchups(orders, podiums=res.podium is not None)
    assert np.array_equal(res.hist, h)
    assert np.array_equal(res.ahead, a)
    if p is None:
        assert res.podium is None
    else:
        assert np.array_equal(res.podium, p)


def _equals_oracle(res, case, n_sims, seed, sim_offset=0, deviates=32):
    rng = O.RNG_PHILOX53 if deviates == 53 else O.RNG_PHILOX
    ref = O.Problem(case).run(n_sims, rng=rng, seed=seed, sim_offset=sim_offset, want_orders=True)
    assert np.array_equal(res.hist, ref['hist'])
    _equals_orders(res, ref['orders'])


# name: (deviates, sim_offset)
GOLDEN = {'S60': (32, 0), 'N10': (32, 0), 'EVT': (53, 0), 'HET': (32, 0), 'WET': (32, 98765), 'DMP': (32, 0),
          'S78': (32, 0)}


@pytest.mark.parametrize('name', list(GOLDEN))
def test_golden_cases_equal_the_oracle(require_gpu, name):
    case = O.load_case(name)
    deviates, offset = GOLDEN[name]
    n_sims, seed = 4000, 1000 + sum(map(ord, name))
    res = _run(case, n_sims, seed, offset, deviates)
    _equals_oracle(res, case, n_sims, seed, offset, deviates)
    _identities(res)
    # hist is mcgp_run's, count for count
    sim = _sim(case, deviates)
    probs = sim.run_monte_carlo(n_sims, *_args(case), seed=seed, track_condition=case['track_condition'],
                                sim_offset=offset)
    assert np.array_equal(res.hist, sim.last_histogram) and res.position_probabilities == probs


def _field(n):
    """An n-car field with S60's parameters, 25 laps and an all-zero grid column (the builder of test_gpu_parity)."""
    rng = np.random.default_rng(n)
    drivers = [f'D{i:02d}' for i in range(n)]
    base = O.load_case('S60')
    case = dict(base)
    case['config'] = dict(base['config'], total_laps=25,
                          driver_teams={d: list(base['config']['dnf_rates'])[i % 10] for i, d in enumerate(drivers)})
    g = rng.random((n, n))
    g[:, n // 2] = 0.0
    case['grid_probs'] = {d: [float(x) for x in g[i]] for i, d in enumerate(drivers)}
    case['base_pace'] = {d: 90.0 + 0.2 * i for i, d in enumerate(drivers)}
    case['tire_deg'] = {d: 0.05 for d in drivers}
    case['driver_variance'] = {d: 0.2 for d in drivers}
    case['driver_dnf_rates'] = {d: 0.01 for d in drivers}
    return case


@pytest.mark.parametrize('n', list(range(1, 33)))
def test_field_sizes_equal_the_oracle(require_gpu, n):
    case = _field(n)
    res = _run(case, 700, 60 + n, sim_offset=3)
    assert (res.podium is None) == (n < 3)
    _equals_oracle(res, case, 700, 60 + n, 3)
    _identities(res)


@pytest.mark.parametrize('n_sims', [501, 502, 503])
def test_byte_tail_of_the_staged_orders(require_gpu, n_sims):
    """23 cars and a last tile of 245, 246 and 247 simulations: its orders end 3, 2 and 1 bytes past a whole word, the
    bytes race_matchups copies one by one (the same for its blocks of 256, 128 and 64)."""
    n = 23
    assert all((n_sims % b) * n % 4 == 504 - n_sims for b in (256, 128, 64))
    case = _field(n)
    res = _run(case, n_sims, 90 + n_sims, sim_offset=5)
    _equals_oracle(res, case, n_sims, 90 + n_sims, 5)
    _identities(res)


def test_generic_kernel_problem(require_gpu):
    """A negative overtake_delta is served by the generic race kernel only; the counting is the same."""
    case = copy.deepcopy(O.load_case('S60'))
    case['config']['overtake_delta'] = -0.5
    res = _run(case, 3000, 17)
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_kernel'
    _equals_oracle(res, case, 3000, 17)
    _identities(res)


def test_podium_by_global_atomics_and_without_podium(require_gpu, monkeypatch):
    """A block LDS budget too small for the podium table (MCGP_LDS_PER_BLOCK, read per call by this entry point):
    the podium goes to global atomics, with the same counts; podiums=False leaves the other counts as they were."""
    for case in (O.load_case('S60'), _field(32)):
        whole = _run(case, 5000, 23, sim_offset=77)
        monkeypatch.setenv('MCGP_LDS_PER_BLOCK', '16384')
        small = _run(case, 5000, 23, sim_offset=77)
        monkeypatch.delenv('MCGP_LDS_PER_BLOCK')
        for k in ('hist', 'ahead', 'podium'):
            assert np.array_equal(getattr(small, k), getattr(whole, k)), k
        bare = _run(case, 5000, 23, sim_offset=77, podiums=False)
        assert bare.podium is None
        assert np.array_equal(bare.hist, whole.hist) and np.array_equal(bare.ahead, whole.ahead)
        _equals_oracle(small, case, 5000, 23, 77)


def test_across_the_chunk_boundary_and_split(require_gpu):
    """2^22 + 4097 N10 simulations (two chunks) against the product's own orders; a split at an odd offset sums to the
    unsplit run."""
    case = O.load_case('N10')
    n_sims, seed, cut = (1 << 22) + 4097, 5, 1234567
    res = _run(case, n_sims, seed)
    sim = _sim(case)
    _, orders = sim.run_monte_carlo(n_sims, *_args(case), seed=seed, track_condition=case['track_condition'],
                                    return_orders=True)
    _equals_orders(res, orders)
    _identities(res)
    a = _run(case, cut, seed)
    b = _run(case, n_sims - cut, seed, sim_offset=cut)
    for k in ('hist', 'ahead', 'podium'):
        assert np.array_equal(getattr(a, k) + getattr(b, k), getattr(res, k)), k


def test_shards_over_devices_equal_one_device(require_gpu):
    case = O.load_case('S60')
    one = _run(case, 20001, 31, sim_offset=11)
    two = _run(case, 20001, 31, sim_offset=11, device=[0, 0])
    for k in ('hist', 'ahead', 'podium'):
        assert np.array_equal(getattr(two, k), getattr(one, k)), k
    assert two.n_simulations == 20001


def test_device_time_covers_the_call(require_gpu):
    case = O.load_case('S60')
    _run(case, 200_000, 3)
    ms = C.c_float()
    N.check(N.lib().mcgp_last_kernel_ms(0, C.byref(ms)))
    assert ms.value > 0.0


def test_cli_predict_matchups_end_to_end(require_gpu, tmp_path, capsys):
    plain, extra = tmp_path / 'plain.json', tmp_path / 'matchups.json'
    base = ['predict', '--race', 'Bahrain', '--season', '2024', '--simulations', '20000', '--seed', '42', '--offline']
    assert cli.main(base + ['--json', str(plain)]) == 0
    capsys.readouterr()
    assert cli.main(base + ['--matchups', '--json', str(extra)]) == 0
    text = capsys.readouterr().out
    assert 'TEAMMATE HEAD-TO-HEAD' in text and 'MOST LIKELY PODIUMS' in text
    a, b = json.loads(plain.read_text()), json.loads(extra.read_text())
    assert {k: b[k] for k in a} == a                    # every other key keeps its value
    assert set(b) - set(a) == {'head_to_head', 'teammate_battles', 'likely_podiums'}
    h2h = b['head_to_head']
    assert len(b['teammate_battles']) == 10
    for battle in b['teammate_battles']:
        x, y = battle['drivers']
        assert battle['probabilities'] == [h2h[x][y], h2h[y][x]]
        assert abs(sum(battle['probabilities']) - 1.0) < 1e-12
    top = b['likely_podiums']
    assert len(top) == 10 and all(r['probability'] <= b['win_probabilities'][r['podium'][0]] for r in top)


def test_predict_weekend_matchups_with_the_device_front_end(require_gpu):
    """device_front_end: the matrix from grid_probs_on_device goes to run_matchups; every other key keeps its value."""
    from monte_carlo_gp_amd.predictor import F1Predictor
    fx = cli.synthetic_fixture()
    plain = F1Predictor(device_front_end=True).predict_weekend(2024, 'Bahrain', fx, n_simulations=30000, seed=8)
    more = F1Predictor(device_front_end=True).predict_weekend(2024, 'Bahrain', fx, n_simulations=30000, seed=8,
                                                              matchups=True)
    assert {k: more[k] for k in plain} == plain
    assert set(more) - set(plain) == {'head_to_head', 'teammate_battles', 'likely_podiums'}
