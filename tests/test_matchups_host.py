"""Head-to-head and podium counts, host side: the numpy restatement (matchups_ref) on hand-built orders, the C-ABI
argument checks of mcgp_run_matchups (no device needed), the MatchupResult helpers on synthetic counts, and the
`predict --matchups` flag with a stand-in predictor."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest

import matchups_ref as MR
import oracle_py as O
from monte_carlo_gp_amd import MatchupResult, RaceConfig, RaceSimulator, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import predictor as P


# ---------------------------------------------------------------- the restatement on hand-built orders
@pytest.mark.parametrize('n', [1, 2, 3, 32])
def test_identity_and_reversed_orders(n):
    sims = 5
    ident = np.tile(np.arange(n, dtype=np.uint8), (sims, 1))
    h, a, p = MR.matchups(ident)
    assert np.array_equal(h, sims * np.eye(n, dtype=np.int64))
    assert np.array_equal(a, sims * np.triu(np.ones((n, n), np.int64), 1))       # i ahead of every j > i
    if n >= 3:
        assert p[0, 1, 2] == sims and p.sum() == sims
    else:
        assert p is None
    rev = ident[:, ::-1].copy()
    h, a, p = MR.matchups(rev)
    assert np.array_equal(h, sims * np.fliplr(np.eye(n, dtype=np.int64)))
    assert np.array_equal(a, sims * np.tril(np.ones((n, n), np.int64), -1))
    if n >= 3:
        assert p[n - 1, n - 2, n - 3] == sims and p.sum() == sims


@pytest.mark.parametrize('n', [1, 2, 3, 32])
def test_random_permutations_satisfy_the_identities(n):
    rng = np.random.default_rng(n)
    sims = 400
    orders = np.array([rng.permutation(n) for _ in range(sims)], np.uint8)
    h, a, p = MR.matchups(orders)
    assert np.array_equal(a, MR.ahead_by_loop(orders))
    assert np.array_equal(np.diag(a), np.zeros(n, np.int64))
    off = ~np.eye(n, dtype=bool)
    assert ((a + a.T)[off] == sims).all()
    assert (h.sum(axis=0) == sims).all() and (h.sum(axis=1) == sims).all()
    if n >= 3:
        assert np.array_equal(p.sum(axis=(1, 2)), h[:, 0])
        assert np.array_equal(p.sum(axis=(0, 2)), h[:, 1])
        assert np.array_equal(p.sum(axis=(0, 1)), h[:, 2])
        # a podium cell by a plain count
        o = orders.astype(int)
        a0, b0, c0 = o[0, :3]
        assert p[a0, b0, c0] == sum(1 for r in o if tuple(r[:3]) == (a0, b0, c0))


def test_hand_built_pairs():
    # three simulations of four drivers
    orders = np.array([[2, 0, 1, 3], [0, 2, 3, 1], [2, 3, 0, 1]], np.uint8)
    h, a, p = MR.matchups(orders)
    assert a[2, 0] == 2 and a[0, 2] == 1            # 2 ahead of 0 in the first and third
    assert a[3, 1] == 2 and a[1, 3] == 1
    assert a[0, 1] == 3 and a[1, 0] == 0
    assert p[2, 0, 1] == 1 and p[0, 2, 3] == 1 and p[2, 3, 0] == 1 and p.sum() == 3
    assert h[:, 0].tolist() == [1, 0, 2, 0]


# ---------------------------------------------------------------- the C ABI without a device
def _abi_call(n=3, hist=True, ahead=True, podium=False, n_sims=100, device=0, case='S60', deviates=32, config=None,
              fill=0):
    lib = N.lib()
    c = O.load_case(case)
    from monte_carlo_gp_amd.simulation import _Problem, DEFAULT_SET_POP, _dptr
    m = max(n, 1)
    drivers = [f'D{i:02d}' for i in range(m)]        # (arrays as long as the n the call names)
    prob = _Problem(RaceConfig(**dict(c['config'], **(config or {}))), drivers, {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)
    g = np.full((m, m), 1.0 / m)
    bufs = [np.full(64 ** 3, fill, np.uint64) for _ in range(3)]
    ptr = lambda b, on: b.ctypes.data_as(C.POINTER(C.c_uint64)) if on else None
    rc = lib.mcgp_run_matchups(C.byref(prob.cfg), C.byref(prob.drv), _dptr(g), n, n_sims, 0, 1, device,
                               ptr(bufs[0], hist), ptr(bufs[1], ahead), ptr(bufs[2], podium))
    return rc, lib.mcgp_last_error().decode(), bufs


def test_library_rejects_bad_arguments_before_any_device_lookup():
    """MCGP_E_BAD_ARG with a message, on a machine with or without a GPU (the checks come first)."""
    cases = [
        (dict(hist=False), 'hist_out'),
        (dict(ahead=False), 'ahead_out'),
        (dict(n=0), 'n must be in [1, 32]'),
        (dict(n=33), 'n must be in [1, 32]'),
        (dict(n=2, podium=True), 'n >= 3'),
        (dict(n=1, podium=True), 'n >= 3'),
        (dict(n=3, deviates=53, config=dict(overtake_delta=-0.5)), 'reg_kernel_serves'),
    ]
    for kw, msg in cases:
        rc, err, _ = _abi_call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    # valid calls of zero simulations return without a device
    for kw in (dict(n=3, podium=True), dict(n=2), dict(n=32, podium=True)):
        rc, err, _ = _abi_call(n_sims=0, **kw)
        assert rc == 0, (kw, err)


def test_outputs_untouched_when_the_call_fails():
    """A device index no machine has: every argument passes, the device lookup fails, the buffers keep their values."""
    rc, err, bufs = _abi_call(n=4, podium=True, device=999, fill=7)
    assert rc == -2 and 'device' in err
    assert all((b == 7).all() for b in bufs)


def test_run_matchups_of_nothing_needs_no_device():
    case = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**case['config']))
    res = sim.run_matchups(0, case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'])
    assert isinstance(res, MatchupResult) and res.n_simulations == 0
    assert res.hist.shape == (20, 20) and not res.ahead.any() and res.podium.shape == (20, 20, 20)
    assert sim.last_drivers == list(case['grid_probs']) and not sim.last_histogram.any()
    res = sim.run_matchups(0, case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'],
                           podiums=False)
    assert res.podium is None


# ---------------------------------------------------------------- MatchupResult on synthetic counts
def _result(orders, drivers):
    h, a, p = MR.matchups(orders)
    return MatchupResult(drivers=drivers, n_simulations=len(orders), hist=h, ahead=a, podium=p)


def test_result_helpers():
    drivers = ['VER', 'PER', 'HAM', 'RUS']
    # VER-PER and HAM-RUS are teams; 4 simulations
    orders = np.array([[0, 2, 1, 3], [0, 2, 1, 3], [2, 0, 3, 1], [1, 0, 2, 3]], np.uint8)
    r = _result(orders, drivers)
    assert r.head_to_head('VER', 'PER') == 0.75 and r.head_to_head('PER', 'VER') == 0.25
    assert r.ahead_probabilities['HAM']['RUS'] == 1.0 and 'HAM' not in r.ahead_probabilities['HAM']
    assert r.position_probabilities == {'VER': {1: 0.5, 2: 0.5}, 'PER': {1: 0.25, 3: 0.5, 4: 0.25},
                                        'HAM': {1: 0.25, 2: 0.5, 3: 0.25}, 'RUS': {3: 0.25, 4: 0.75}}
    teams = {'VER': 'Red Bull', 'PER': 'Red Bull', 'HAM': 'Mercedes', 'RUS': 'Mercedes', 'XXX': 'Mercedes'}
    battles = r.teammate_battles(teams)
    assert battles == [{'team': 'Red Bull', 'drivers': ['VER', 'PER'], 'probabilities': [0.75, 0.25]},
                       {'team': 'Mercedes', 'drivers': ['HAM', 'RUS'], 'probabilities': [1.0, 0.0]}]
    assert r.teammate_battles({'VER': 'A', 'HAM': 'A'}) == [
        {'team': 'A', 'drivers': ['VER', 'HAM'], 'probabilities': [0.75, 0.25]}]
    assert r.teammate_battles({}) == []
    sets = r.podium_set_probabilities()
    assert sets == {frozenset({'VER', 'HAM', 'PER'}): 0.75, frozenset({'HAM', 'VER', 'RUS'}): 0.25}
    assert abs(sum(sets.values()) - 1.0) < 1e-12
    top = r.most_likely_podiums(5)
    assert top == [(('VER', 'HAM', 'PER'), 0.5), (('PER', 'VER', 'HAM'), 0.25), (('HAM', 'VER', 'RUS'), 0.25)]
    assert r.most_likely_podiums(1) == top[:1] and r.most_likely_podiums(0) == []


def test_unordered_podiums_sum_the_six_orders():
    rng = np.random.default_rng(5)
    n = 6
    drivers = [f'D{i}' for i in range(n)]
    r = _result(np.array([rng.permutation(n) for _ in range(3000)], np.uint8), drivers)
    sets = r.podium_set_probabilities()
    for trio in itertools.combinations(range(n), 3):
        want = sum(int(r.podium[a, b, c]) for a, b, c in itertools.permutations(trio)) / 3000
        assert sets.get(frozenset(drivers[i] for i in trio), 0.0) == want
    top = r.most_likely_podiums(200)
    assert len(top) == np.count_nonzero(r.podium)
    probs = [q for _, q in top]
    assert probs == sorted(probs, reverse=True) and abs(sum(probs) - 1.0) < 1e-12


def test_podium_helpers_need_podium_counts():
    r = MatchupResult(drivers=['A', 'B'], n_simulations=1, hist=np.eye(2, dtype=np.int64),
                      ahead=np.array([[0, 1], [0, 0]]), podium=None)
    with pytest.raises(ValueError, match='podium'):
        r.most_likely_podiums()
    with pytest.raises(ValueError, match='podium'):
        r.podium_set_probabilities()
    assert P.matchup_keys(r, {'A': 't', 'B': 't'}) == {
        'head_to_head': {'A': {'B': 1.0}, 'B': {'A': 0.0}},
        'teammate_battles': [{'team': 't', 'drivers': ['A', 'B'], 'probabilities': [1.0, 0.0]}],
        'likely_podiums': []}


# ---------------------------------------------------------------- the CLI flag
class _FakePredictor:
    """predict_weekend's result shape from synthetic counts (no device)."""
    calls = []

    def __init__(self, device=0):
        pass

    def predict_weekend(self, season, race, fixture, prediction_point='fp2', n_simulations=0, seed=None, matchups=False):
        _FakePredictor.calls.append(matchups)
        drivers = list(fixture['drivers'])
        n = len(drivers)
        orders = np.array([np.roll(np.arange(n), k) for k in range(n)], np.uint8)
        r = _result(orders, drivers)
        res = P.pack_result(drivers, {d: [1.0 / n] * n for d in drivers}, r.position_probabilities, {}, prediction_point,
                            None)
        if matchups:
            from monte_carlo_gp_amd import config as K
            res.update(P.matchup_keys(r, K.DRIVER_TEAMS))
        return res


def test_predict_matchups_flag(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    plain, extra = tmp_path / 'plain.json', tmp_path / 'matchups.json'
    base = ['predict', '--race', 'Bahrain', '--offline', '--simulations', '20', '--seed', '1']
    assert cli.main(base + ['--json', str(plain)]) == 0
    out = capsys.readouterr().out
    assert 'TEAMMATE HEAD-TO-HEAD' not in out and 'MOST LIKELY PODIUMS' not in out
    assert cli.main(base + ['--matchups', '--json', str(extra)]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [False, True]
    assert out.index('PODIUM PROBABILITIES') < out.index('TEAMMATE HEAD-TO-HEAD') < out.index('MOST LIKELY PODIUMS')
    a, b = json.loads(plain.read_text()), json.loads(extra.read_text())
    new = {'head_to_head', 'teammate_battles', 'likely_podiums'}
    assert not new & set(a)                              # the default JSON has no new keys
    assert set(b) == set(a) | new
    assert {k: b[k] for k in a} == a
    assert len(b['teammate_battles']) == 10 and len(b['likely_podiums']) == 10
    for battle in b['teammate_battles']:
        x, y = battle['drivers']
        assert battle['probabilities'] == [b['head_to_head'][x][y], b['head_to_head'][y][x]]
        assert f'{x:4}' in out
