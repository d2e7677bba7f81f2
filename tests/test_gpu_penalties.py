"""Time penalties on the device (mcgp_run_penalties): scenarios without penalties are mcgp_run_strategies bit for bit;
penalised scenarios give the Python restatement's finishing orders and fates (penalties_ref); a huge post-race penalty
moves only its driver; a serve penalty that no stop can serve is the post-race penalty; counts are split-, shard- and
chunk-invariant; the `penalty` CLI runs end to end."""
import json

import numpy as np
import pytest

import oracle_py as O
import penalties_ref as PR
import resume_ref as RR
import strategy_ref as SR
from monte_carlo_gp_amd import PitPlan, RaceConfig, RaceSimulator, TimePenalty, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP

pytestmark = pytest.mark.gpu

GOLDEN = ['S60', 'S78', 'S50', 'N10', 'HET', 'EVT', 'DMP', 'WET']
SERVE, FLAG, LAP = PR.SERVE, PR.FLAG, PR.LAP
HARD = 2


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


def _check(rc):
    assert rc == 0, N.lib().mcgp_last_error().decode()


_traced = {}


def _ref(name, m, seed, off):
    """The oracle's traced run of a case, computed once and shared."""
    key = (name, m, seed, off)
    if key not in _traced:
        _traced[key] = RR.traced_run(_case(name), m, seed, off)
    return _traced[key]


# ---------------------------------------------------------------- 1. scenarios without penalties
@pytest.mark.parametrize('name', GOLDEN + ['n1', 'n2', 'n32'])
def test_scenarios_without_penalties_are_mcgp_run_strategies(require_gpu, name):
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    seed, m, off = 4242, 3000, 777
    plans = [{}, {0: (-1, 0, [(8, HARD)])}, {n - 1: (-1, 0, [(15, 1), (L - 5, 0)]), 0: (-1, 0, [])}, {}]
    rc, h0, d0, o0 = SR.run_c(case, plans, m, seed, sim_offset=off)
    _check(rc)
    rc, h, dl, ft, o = PR.run_c(case, plans, [[]] * len(plans), m, seed, sim_offset=off)
    _check(rc)
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_penalties_kernel'
    assert np.array_equal(o, o0) and np.array_equal(h, h0) and np.array_equal(dl, d0)
    assert (ft[:, :, 0] == m).all() and ft.sum() == len(plans) * n * m
    # ... and without delta, fate or orders the histogram is the same
    rc, h1, d1, f1, _ = PR.run_c(case, plans, [[]] * len(plans), m, seed, sim_offset=off, orders=False, delta=False,
                                 fate=False)
    _check(rc)
    assert np.array_equal(h1, h0) and not d1.any() and not f1.any()


# ---------------------------------------------------------------- 2. the device equals the restatement
@pytest.mark.parametrize('s', range(7))
@pytest.mark.parametrize('start', ['grid', 'state'])
@pytest.mark.parametrize('name', ['S60', 'EVT', 'n32'])
def test_device_equals_the_restatement(require_gpu, name, start, s):
    """Scenario s of penalties_ref.scenarios beside the empty scenario, m = 160: the returned orders and fate counts are
    the restatement's, and hist and delta are the counts of the returned orders."""
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    seed, m, off = 55, 160, 400
    ref = _ref(name, m, seed, off)
    if start == 'grid':
        state, first, kw = None, 2, dict(grids=ref['grids'])
    else:
        k = L // 2
        state = (RR.state_arrays(ref, 1, k), k, RR.drs_disabled_until(case, seed, off + 1, k))
        first, kw = k + 1, dict(state=state)
    pens, plans = PR.scenarios(first, L, n)[s]
    rc, h, dl, ft, o = PR.run_c(case, [{}, plans], [[], pens], m, seed, sim_offset=off, state=state)
    _check(rc)
    if start == 'grid':
        assert np.array_equal(o[0], ref['orders'])
    want, fates = PR.orders(case, m, seed, off, plans=plans, penalties=pens, **kw)
    bad = [i for i in range(m) if not np.array_equal(o[1, i], want[i])]
    assert not bad, f'{len(bad)} of {m} orders differ, first sim {bad[0]}'
    assert np.array_equal(h, PR.hist_counts(o, n)) and np.array_equal(dl, SR.delta_counts(o, n))
    assert np.array_equal(ft[1], PR.fate_counts(fates[None], n)[0])
    assert (ft[0, :, 0] == m).all() and (ft.sum(axis=2) == m).all()


# ---------------------------------------------------------------- 3. exact properties
def test_a_huge_post_race_penalty_moves_only_its_driver_and_an_unservable_penalty_is_a_post_race_one(require_gpu):
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    seed, m, d, x = 91, 20_000, 3, 5.0
    pens = [[], [(d, FLAG, 0, 1e6)], [(d, SERVE, L - 5, x)], [(d, FLAG, 0, x)]]
    rc, h, dl, ft, o = PR.run_c(case, None, pens, m, seed)
    _check(rc)
    # only d's key changes in a total order: everybody else keeps their relative order, and d never gains
    others = lambda a: a[a != d].reshape(m, n - 1)
    assert np.array_equal(others(o[1]), others(o[0]))
    pos = lambda a: np.argmax(a == d, axis=1)
    assert (pos(o[1]) >= pos(o[0])).all() and (pos(o[1]) > pos(o[0])).any()
    assert dl[1, d, :n - 1].sum() == 0
    # the rule stops only while more than 5 laps remain: pending from lap L - 5, no stop can serve the penalty
    assert np.array_equal(o[2], o[3]) and np.array_equal(h[2], h[3]) and np.array_equal(dl[2], dl[3])
    assert ft[2, d, 1] == 0 and ft[2, d, 0] == 0 and ft[2, d, 2] + ft[2, d, 3] == m and ft[2, d, 2] > 0
    assert (ft[3, :, 0] == m).all()
    assert not np.array_equal(o[3], o[0])


def test_a_two_lap_race(require_gpu):
    """L = 2: lap 2 is the first lap with a pit step and the last; ON_LAP on lap 2 and AT_FLAG against the restatement."""
    case = _case('S60')
    case = dict(case, config=dict(case['config'], total_laps=2))
    n = len(case['grid_probs'])
    seed, m = 12, 160
    ref = RR.traced_run(case, m, seed)
    pens = [[], [(0, LAP, 2, 4.0), (n - 1, LAP, 2, 0.5)], [(1, FLAG, 0, 4.0)], [(2, SERVE, 2, 4.0)]]
    rc, h, dl, ft, o = PR.run_c(case, None, pens, m, seed)
    _check(rc)
    assert np.array_equal(o[0], ref['orders'])
    for s, p in enumerate(pens):
        want, fates = PR.orders(case, m, seed, penalties=p, grids=ref['grids'])
        assert np.array_equal(o[s], want), s
        assert np.array_equal(ft[s], PR.fate_counts(fates[None], n)[0]), s
    assert not np.array_equal(o[1], o[0]) and not np.array_equal(o[2], o[0])
    assert np.array_equal(h, PR.hist_counts(o, n)) and np.array_equal(dl, SR.delta_counts(o, n))


# ---------------------------------------------------------------- 4. counts do not depend on the split
KIND = {SERVE: 'serve', FLAG: 'flag', LAP: 'lap'}


def test_counts_are_split_shard_and_chunk_invariant(require_gpu, monkeypatch):
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    scen = PR.scenarios(2, L, n)
    pens, plans = [p for p, _ in scen], [pl for _, pl in scen]
    seed, m = 8, 20_000
    rc, h, dl, ft, o = PR.run_c(case, plans, pens, m, seed)
    _check(rc)
    assert np.array_equal(dl, SR.delta_counts(o, n)) and np.array_equal(h, PR.hist_counts(o, n))
    assert (ft.sum(axis=2) == m).all()
    a = 7_111                                               # an odd simulation id
    rc1, h1, d1, f1, _ = PR.run_c(case, plans, pens, a, seed, orders=False)
    rc2, h2, d2, f2, o2 = PR.run_c(case, plans, pens, m - a, seed, sim_offset=a)
    _check(rc1)
    _check(rc2)
    assert np.array_equal(h1 + h2, h) and np.array_equal(d1 + d2, dl) and np.array_equal(f1 + f2, ft)
    assert np.array_equal(o2, o[:, a:])
    # through the Python layer, sharded over two devices (or twice over device 0)
    sim = RaceSimulator(RaceConfig(**case['config']), device=[0, min(1, require_gpu - 1)], set_pop=DEFAULT_SET_POP)
    drivers = list(case['grid_probs'])
    penalties = {f's{s}': [TimePenalty(drivers[d], sec, KIND[k], None if k == FLAG else lap) for d, k, lap, sec in p]
                 for s, p in enumerate(pens)}
    strategies = {f's{s}': [PitPlan(drivers[d], [(lap, N.COMPOUNDS[c]) for lap, c in stops]) for d, (_, _, stops) in pl.items()]
                  for s, pl in enumerate(plans) if pl}
    res = sim.run_penalties(m, penalties, strategies, case['base_pace'], case['tire_deg'], case['driver_variance'],
                            case['driver_dnf_rates'], grid_probs=case['grid_probs'], seed=seed,
                            track_condition=case['track_condition'], allow_single_compound=True, return_orders=True)
    assert res.names == [f's{s}' for s in range(len(scen))]
    assert np.array_equal(res.hist, h) and np.array_equal(res.delta, dl) and np.array_equal(res.fate, ft)
    assert np.array_equal(res.orders, o)
    f = res.fate_probabilities('s2', drivers[1])
    assert f['none'] == 0.0 and f['served'] > 0.5 and sum(f.values()) == pytest.approx(1.0)
    # across staging chunks: launches of at most 1000 simulations
    mc = 2500
    rc, hw, dw, fw, ow = PR.run_c(case, plans, pens, mc, seed, sim_offset=5)
    _check(rc)
    monkeypatch.setenv('MCGP_MAX_SIMS_PER_LAUNCH', '1000')
    rc, hc, dc, fc, oc = PR.run_c(case, plans, pens, mc, seed, sim_offset=5)
    monkeypatch.delenv('MCGP_MAX_SIMS_PER_LAUNCH')
    _check(rc)
    assert np.array_equal(hc, hw) and np.array_equal(dc, dw) and np.array_equal(fc, fw) and np.array_equal(oc, ow)


# ---------------------------------------------------------------- 5. the CLI
def test_penalty_cli_end_to_end(require_gpu, tmp_path, capsys):
    out, pred = tmp_path / 'pen.json', tmp_path / 'p.json'
    seed, m = 7, 20_000
    assert cli.main(['predict', '--race', 'Bahrain', '--offline', '--simulations', str(m), '--seed', str(seed),
                     '--json', str(pred)]) == 0
    win = json.load(open(pred))['win_probabilities']
    driver = max(win, key=win.get)
    other = sorted(win, key=win.get)[-2]
    assert cli.main(['penalty', '--race', 'Bahrain', '--offline', '--give', f'{driver}:5:flag', '--driver', driver,
                     '--plan', 'box=:30/HARD', '--simulations', str(m), '--seed', str(seed), '--json', str(out)]) == 0
    text = capsys.readouterr().out
    assert 'scenario: penalised + box' in text and driver in text
    doc = json.load(open(out))
    rows = doc['scenarios']
    assert [r['scenario'] for r in rows] == ['none', 'penalised', 'penalised + box'] and doc['penalised'] == [driver]
    none = rows[0]['win_probabilities']
    assert set(none) == set(win)
    for d in win:
        assert none[d] == pytest.approx(win[d], abs=1e-12)
    assert rows[0]['drivers'][driver]['p_same'] == 1.0 and rows[0]['drivers'][driver]['fate']['none'] == 1.0
    # a post-race penalty changes nobody's race: its driver never finishes ahead of where it finished without it
    assert rows[1]['drivers'][driver]['p_better'] == 0.0 and rows[1]['drivers'][driver]['p_worse'] > 0.0
    assert rows[1]['drivers'][driver]['fate']['none'] == 1.0
    # a 10 s penalty to serve: the split of where it ends up
    assert cli.main(['penalty', '--race', 'Bahrain', '--offline', '--give', f'{other}:10', '--simulations', str(m),
                     '--seed', str(seed), '--json', str(out)]) == 0
    f = json.load(open(out))['scenarios'][1]['drivers'][other]['fate']
    assert f['none'] == 0.0 and f['served'] > 0.5 and f['served'] + f['at_flag'] + f['retired'] == pytest.approx(1.0)
