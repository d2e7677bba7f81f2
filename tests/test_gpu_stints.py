"""Tyre stints on the GPU (mcgp_run_stints / RaceSimulator.run_stints): every count equals, cell for cell, what the numpy
restatement (stints_ref) derives from the CPU oracle's per-lap trace (tyre age, compound, retirement) and the restated
event draws of the same simulations.  From the grid and from mid-race states; coverage conditions asserted from the
reference before comparing, so that equality is not vacuous; split, shard and staging-chunk invariance; consistency at
10^6 simulations with mcgp_run_trace; the CLI.  All comparisons are integer equality."""
import ctypes as C
import dataclasses
import json

import numpy as np
import pytest

import oracle_py as O
import resume_ref as RR
import stints_ref as SR
import trace_ref as TR
from helpers import product_run
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, cli, _native as N
from monte_carlo_gp_amd.predictor import F1Predictor
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP

pytestmark = pytest.mark.gpu

KEYS = SR.KEYS


def _equal(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        bad = np.argwhere(a[k] != b[k])
        assert bad.size == 0, (what, k, bad[:5].tolist(), a[k][tuple(bad[0])], b[k][tuple(bad[0])])


def _err():
    return N.lib().mcgp_last_error()


def _invariants(got, m):
    assert (got['stop_lap'].sum(axis=2) == m).all() and not got['stop_lap'][:, :, 1].any()
    assert (got['seq'].sum(axis=1) == m).all()
    assert np.array_equal(got['stops_pos'].sum(axis=1), got['hist'])


# ---------------------------------------------------------------- from the grid
@pytest.mark.parametrize('name,m', [('S60', 512), ('EVT', 512), ('WET', 256), ('N10', 256), ('HET', 256), ('S78', 256),
                                    ('DMP', 256)])
def test_golden_cases_equal_the_oracle_trace(require_gpu, name, m):
    case = O.load_case(name)
    ref, t = SR.stint_counts(case, m, seed=7, with_tallies=True)
    stops, stints = np.bincount(t['stops'].ravel()).tolist(), np.bincount(t['stints'].ravel()).tolist()
    # coverage (conditions, not measurements), per (simulation, car)
    if name == 'S60':
        assert stops == [411, 6355, 3474]
        assert int((ref['seq'].sum(axis=0) > 0).sum()) == 15
        first = np.nonzero(ref['stop_lap'][:, 0, 1:].sum(axis=0))[0] + 1
        assert (int(first[0]), int(first[-1])) == (12, 54)
    if name == 'EVT':
        assert sum(stints[5:]) == 766 and ref['seq'][:, 0].sum() == 766          # column 0 of seq is exercised
    if name == 'WET':
        assert stops == [m * 20] and stints[1:] == [2423, 1737, 617, 305, 38]    # stints without a stop: red flags
    if name == 'N10':
        assert stops[3] == 408
    rc, got = SR.run_c(case, m, seed=7)
    assert rc == 0, _err()
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_stints_kernel'
    _equal(got, ref, name)
    _invariants(got, m)
    hist, _, _ = product_run(case, m, 7)                                         # the histogram is mcgp_run's
    assert np.array_equal(got['hist'], hist)


def test_the_cap_case(require_gpu):
    """A fifth stop is recorded nowhere and counts in the capped column; a stop under a red flag starts one stint."""
    case = SR.cap_case()
    ref, t = SR.stint_counts(case, 64, seed=3, with_tallies=True)
    assert int((t['stops'] == 5).sum()) == 1267 and t['stops'].size == 1280
    assert t['both'] == 3168 and t['stints'].max() == 12
    rc, got = SR.run_c(case, 64, seed=3)
    assert rc == 0, _err()
    _equal(got, ref, 'cap')
    _invariants(got, 64)
    assert got['stops_pos'][:, 4].sum() >= 1267


@pytest.mark.parametrize('n', [1, 2, 32])
def test_synthetic_fields_equal_the_oracle_trace(require_gpu, n):
    case = RR.field_case(n)
    rc, got = SR.run_c(case, 512, seed=3)
    assert rc == 0, _err()
    _equal(got, SR.stint_counts(case, 512, seed=3), f'n={n}')
    _invariants(got, 512)


# ---------------------------------------------------------------- from a state
def test_oracle_states_continue_into_the_oracle_trace(require_gpu):
    """Oracle states continued as their own simulation: the counts are the oracle trace's of laps k + 1 .. L with stint
    0 on the state's compound, the histogram is mcgp_run_from_state's."""
    total = with_stop = 0
    for name in ('S60', 'EVT', 'N10', 'WET'):
        case = O.load_case(name)
        L, seed, base = case['config']['total_laps'], 11, 500
        ref = RR.traced_run(case, 6, seed, base)
        prob = RR.problem(case)
        for i in range(6):
            e = RR.first_event_lap(case, seed, base + i)
            for k in sorted({1, L // 2, L - 1, L} | ({e} if e is not None else set())):
                st = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k))
                rc, got = SR.run_c(case, 1, seed, sim_offset=base + i, state=st, prob=prob)
                assert rc == 0, _err()
                want = SR.continued_counts(ref, [i], k, case, seed, base)
                _equal(got, want, (name, i, k))
                _invariants(got, 1)
                rc, hist, _ = RR.run_c(prob, [st], 1, [base + i], seed, orders=False)
                assert rc == 0 and np.array_equal(got['hist'], hist[0])
                total += 1
                with_stop += bool(want['stop_lap'][:, 0, 2:].any())
    assert total >= 16 and with_stop >= 4


def test_one_state_continued_as_many_equals_the_restatement(require_gpu):
    case = O.load_case('S60')
    seed, k, m = 13, 31, 256
    ref = RR.traced_run(case, 3, seed)
    st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, seed, 2, k))
    want = SR.restated_counts(case, m, seed, sim_offset=1000, state=st)
    assert not want['stop_lap'][:, :, 1:k + 1].any() and want['stop_lap'][:, 0, k + 1:].any()   # stops after the state only
    assert (want['seq'].sum(axis=0) > 0).sum() >= 4                                # the futures spread over sequences
    into = {key: np.full_like(v, 5, dtype=np.uint64) for key, v in want.items()}
    rc, got = SR.run_c(case, m, seed, sim_offset=1000, state=st, into=into)
    assert rc == 0, _err()
    _equal({key: v - 5 for key, v in got.items()}, want, 'many from one')
    rc, hist, _ = RR.run_c(RR.problem(case), [st], m, [1000], seed, orders=False)
    assert rc == 0 and np.array_equal(got['hist'] - 5, hist[0])


# ---------------------------------------------------------------- invariance
def _sum(a, b):
    return {k: a[k] + b[k] for k in KEYS}


def test_split_and_shards_equal_one_call_across_chunks(require_gpu):
    case = O.load_case('S60')
    rc, _ = SR.run_c(case, 2 * 10 ** 6, seed=9)                       # a full launch: the device's round
    assert rc == 0, _err()
    chunk = SR.chunk_sims(20, TR.device_round())
    assert SR.budget_sims(20) == (256 << 20) // (9 * 20) // 256 * 256 and chunk < 2 * 10 ** 6
    N_ = chunk + 70001                                # one call crosses a chunk boundary, the halves do not
    rc, whole = SR.run_c(case, N_, seed=9, sim_offset=100)
    assert rc == 0, _err()
    h = N_ // 2
    rc1, a = SR.run_c(case, h, seed=9, sim_offset=100)
    rc2, b = SR.run_c(case, N_ - h, seed=9, sim_offset=100 + h)
    assert rc1 == rc2 == 0
    _equal(whole, _sum(a, b), 'split')
    _invariants(whole, N_)
    # two-device-style shards through the simulator surface: device [0, 0] shards by offset
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    one = RaceSimulator(RaceConfig(**case['config']), device=0, set_pop=RR.SET_POP).run_stints(30001, *args, seed=9,
                                                                                             sim_offset=100)
    two = RaceSimulator(RaceConfig(**case['config']), device=[0, 0], set_pop=RR.SET_POP).run_stints(30001, *args, seed=9,
                                                                                                  sim_offset=100)
    rc, direct = SR.run_c(case, 30001, seed=9, sim_offset=100)
    assert rc == 0
    for k in KEYS:
        assert np.array_equal(getattr(one, k), getattr(two, k)) and np.array_equal(getattr(one, k), direct[k]), k
    # the optional outputs left out: the required ones are unchanged, the others untouched
    rc, part = SR.run_c(case, 30001, seed=9, sim_offset=100, optional=False)
    assert rc == 0 and np.array_equal(part['stop_lap'], direct['stop_lap']) and np.array_equal(part['hist'], direct['hist'])
    assert not part['stops_pos'].any() and not part['seq'].any()


# ---------------------------------------------------------------- consistency at a million
def test_consistency_at_a_million(require_gpu):
    case = O.load_case('S60')
    N_, n = 10 ** 6, 20
    rc, s = SR.run_c(case, N_, seed=21)
    assert rc == 0, _err()
    f = C.c_float()
    assert N.lib().mcgp_last_kernel_ms(0, C.byref(f)) == 0 and f.value > 0
    rc, t = TR.run_c(case, N_, seed=21)
    assert rc == 0, _err()
    assert np.array_equal(s['hist'], t['hist'])
    by_stops = s['stops_pos'].sum(axis=2)                                         # [n][5]
    assert np.array_equal(by_stops[:, :4], t['stops'][:, :4])
    assert np.array_equal(by_stops[:, 4], t['stops'][:, 4:].sum(axis=1))          # the capped column is the tail
    for k in range(4):                                                            # a (k + 1)-th stop: more than k stops
        assert np.array_equal(s['stop_lap'][:, k, 2:].sum(axis=1), t['stops'][:, k + 1:].sum(axis=1)), k
    _invariants(s, N_)
    assert (s['stop_lap'][:, 1:, 0] >= s['stop_lap'][:, :-1, 0]).all()


# ---------------------------------------------------------------- the surface and the CLI
def _cli_case():
    inp = F1Predictor().simulator_inputs(cli.synthetic_fixture(), 'Bahrain')
    cfg = dataclasses.asdict(inp['config'])
    return dict(config=cfg, grid_probs=inp['grid_probs'], base_pace=inp['base_pace'], tire_deg=inp['tire_deg'],
                driver_variance=inp['driver_variance'], driver_dnf_rates=inp['driver_dnf_rates'],
                track_condition=inp['track_condition'])


def _quantile_lap(counts, q):
    """The smallest lap by which at least the share q (at least one) of the stopping simulations has stopped."""
    c = counts.copy()
    c[0] = 0
    return int(np.searchsorted(np.cumsum(c), max(q * c.sum(), 1), side='left'))


def test_cli_tyres_end_to_end(require_gpu, tmp_path, capsys):
    """predict --tyres and in-race --tyres on the offline fixture: the probabilities are reference counts / N."""
    case = _cli_case()
    drivers = list(case['grid_probs'])
    m, seed = 2000, 5
    ref_run = O.Problem(case, set_pop=DEFAULT_SET_POP).run(m, rng=O.RNG_PHILOX, seed=seed, want_orders=True,
                                                           want_grids=True, n_trace=m)
    ref = SR.stint_counts(case, m, seed, ref=ref_run)
    out = tmp_path / 'tyres.json'
    assert cli.main(['predict', '--race', 'Bahrain', '--season', '2024', '--offline', '--simulations', str(m), '--seed',
                     str(seed), '--tyres', '--json', str(out)]) == 0
    text = capsys.readouterr().out
    assert 'TYRE STRATEGY' in text and 'WIN ODDS BY STOP COUNT' in text
    t = json.loads(out.read_text())['tyres']
    assert t['first_lap'] == 2
    for i, d in enumerate(drivers):
        row = t['drivers'][d]
        by_stops = ref['stops_pos'][i].sum(axis=1)
        assert row['stops'] == (by_stops / m).tolist(), d
        if ref['stop_lap'][i, 0, 1:].any():
            assert row['first_stop_window'] == [_quantile_lap(ref['stop_lap'][i, 0], q) for q in (0.1, 0.9)], d
        else:
            assert row['first_stop_window'] is None
        best = int(np.argmax(ref['seq'][i]))
        assert row['strategy']['probability'] == ref['seq'][i, best] / m
        assert [None if p is None else p for p in row['win_by_stops']] == [
            (ref['stops_pos'][i, s, 0] / by_stops[s]) if by_stops[s] else None for s in range(5)], d
    # in-race: simulation 0's state after lap 30 continued as 1 simulation is the oracle's trace of simulation 0
    k = 30
    state = RR.race_state(RR.state_arrays(ref_run, 0, k), k, RR.drs_disabled_until(case, seed, 0, k), drivers)
    path, out2 = tmp_path / 'lap30.json', tmp_path / 'inrace.json'
    path.write_text(json.dumps(state.to_json()))
    assert cli.main(['in-race', '--race', 'Bahrain', '--season', '2024', '--offline', '--state', str(path),
                     '--simulations', '1', '--seed', str(seed), '--tyres', '--json', str(out2)]) == 0
    assert 'TYRE STRATEGY' in capsys.readouterr().out
    t = json.loads(out2.read_text())[0]['tyres']
    want = SR.continued_counts(ref_run, [0], k, case, seed)
    assert t['first_lap'] == k + 1
    for i, d in enumerate(drivers):
        assert t['drivers'][d]['stops'] == want['stops_pos'][i].sum(axis=1).astype(float).tolist(), d
        laps = np.nonzero(want['stop_lap'][i, 0, 1:])[0] + 1
        assert t['drivers'][d]['first_stop_window'] == ([int(laps[0])] * 2 if len(laps) else None), d
