"""Race trace on the GPU (mcgp_run_trace / RaceSimulator.run_trace): the five count arrays equal, cell for cell, what the
numpy restatement (trace_ref) derives from the CPU oracle's per-lap trace of the same simulations; a hand computation of
the pit rule; consistency at 10^6 simulations; split, shard and staging-chunk invariance; the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
import resume_ref as RR
import trace_ref as TR
from helpers import product_run
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, _native as N

pytestmark = pytest.mark.gpu

KEYS = ('hist', 'lap_pos', 'laps_led', 'stops', 'fastest', 'events')


def _equal(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        bad = np.argwhere(a[k] != b[k])
        assert bad.size == 0, (what, k, bad[:5].tolist(), a[k][tuple(bad[0])], b[k][tuple(bad[0])])


@pytest.mark.parametrize('name,m,offset', [('S60', 1024, 0), ('S78', 512, 0), ('N10', 512, 0), ('HET', 512, 0),
                                           ('EVT', 1024, 0), ('DMP', 512, 0), ('WET', 512, 12345)])
def test_golden_cases_equal_the_oracle_trace(name, m, offset):
    case = O.load_case(name)
    rc, got = TR.run_c(case, m, seed=7, sim_offset=offset)
    assert rc == 0, N.lib().mcgp_last_error()
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_trace_kernel'
    _equal(got, TR.trace_counts(case, m, seed=7, sim_offset=offset), name)
    # the histogram is mcgp_run's
    hist, _, _ = product_run(case, m, 7, sim_offset=offset)
    assert np.array_equal(got['hist'], hist)


@pytest.mark.parametrize('n', [1, 2, 32])
def test_synthetic_fields_equal_the_oracle_trace(n):
    case = RR.field_case(n)
    rc, got = TR.run_c(case, 512, seed=3)
    assert rc == 0, N.lib().mcgp_last_error()
    _equal(got, TR.trace_counts(case, 512, seed=3), f'n={n}')


def _no_events_no_retirements():
    case = O.load_case('S60')
    cfg = dict(case['config'], sc_probability=0.0, vsc_probability=0.0, red_flag_probability=0.0,
               dnf_rates={k: 0.0 for k in case['config']['dnf_rates']})
    drivers = list(case['grid_probs'])
    n = len(drivers)
    # driver d starts from slot d (one-hot grid), so the stint plan is fixed
    grid = {d: [1.0 if j == i else 0.0 for j in range(n)] for i, d in enumerate(drivers)}
    return dict(case, config=cfg, grid_probs=grid, driver_dnf_rates={d: 0.0 for d in drivers})


def test_stop_counts_follow_the_pit_rule():
    """S60 (60 laps, every tire_deg 0.05: optimal laps SOFT 15, MEDIUM 25, HARD 40) with no events and no retirements.
    Slots 0-9 start on SOFT aged 4 (5 after lap 1): pit on lap 12 (age 16 > 15, 48 laps left -> HARD), then lap 53 (age
    41 > 40, 7 left -> SOFT): 2 stops.  Slots 10-19 start on MEDIUM aged 0: pit on lap 26 (age 26 > 25, 34 left ->
    HARD), and HARD lasts to the flag: 1 stop."""
    case = _no_events_no_retirements()
    N_ = 2048
    rc, got = TR.run_c(case, N_, seed=5)
    assert rc == 0, N.lib().mcgp_last_error()
    n, L = 20, 60
    want = np.zeros((n, L + 1), np.int64)
    want[:10, 2] = N_
    want[10:, 1] = N_
    assert np.array_equal(got['stops'], want)
    assert (got['lap_pos'][:, :, n] == 0).all()                      # nobody retires
    assert np.array_equal(got['events'][:, 0], [N_] * 3)
    assert got['fastest'].sum() == N_


def test_consistency_at_a_million():
    case = O.load_case('S60')
    N_ = 10 ** 6
    rc, t = TR.run_c(case, N_, seed=21)
    assert rc == 0, N.lib().mcgp_last_error()
    n, L = 20, 60
    assert (t['lap_pos'].sum(axis=2) == N_).all()
    assert (t['lap_pos'][L - 1][:, :n] <= t['hist']).all()
    assert (t['laps_led'] @ np.arange(L + 1) == t['lap_pos'][:, :, 0].sum(axis=0)).all()
    assert (t['laps_led'].sum(axis=1) == N_).all() and (t['stops'].sum(axis=1) == N_).all()
    assert t['fastest'].sum() <= N_
    assert (t['events'].sum(axis=1) == N_).all()
    # the histogram is mcgp_run's
    hist, _, _ = product_run(case, N_, 21)
    assert np.array_equal(t['hist'], hist)
    # the run crosses staging-chunk boundaries of the documented rule (512 MiB / (60 x 20) -> 447 232 simulations,
    # rounded down to whole rounds of the device)
    assert TR.budget_sims(n, L) == 447232
    assert 2 * TR.chunk_sims(n, L, TR.device_round()) < N_


def _sum(a, b):
    return {k: a[k] + b[k] for k in KEYS}


def test_split_equals_one_call_across_chunks():
    case = O.load_case('S60')
    rc, _ = TR.run_c(case, 10 ** 6, seed=9)             # a full launch: the device's round
    assert rc == 0
    N_ = TR.chunk_sims(20, 60, TR.device_round()) + 70001     # one call crosses a chunk boundary, the halves do not
    rc, whole = TR.run_c(case, N_, seed=9, sim_offset=100)
    assert rc == 0
    h = N_ // 2
    rc1, a = TR.run_c(case, h, seed=9, sim_offset=100)
    rc2, b = TR.run_c(case, N_ - h, seed=9, sim_offset=100 + h)
    assert rc1 == rc2 == 0
    _equal(whole, _sum(a, b), 'split')


def test_long_race_small_chunks():
    """L = 300, n = 32: 512 MiB / 9600 -> 55 808 simulations a chunk (less than a round of the device, so not rounded
    further); a run of 3 chunks and a bit equals its halves."""
    case = RR.field_case(32)
    case = dict(case, config=dict(case['config'], total_laps=300))
    rc, _ = TR.run_c(case, 10 ** 6, seed=4)
    assert rc == 0
    chunk = TR.chunk_sims(32, 300, TR.device_round())
    assert TR.budget_sims(32, 300) == 55808 and chunk <= 55808
    N_ = 3 * chunk + 1001
    rc, whole = TR.run_c(case, N_, seed=4)
    assert rc == 0, N.lib().mcgp_last_error()
    h = chunk + 17
    rc1, a = TR.run_c(case, h, seed=4)
    rc2, b = TR.run_c(case, N_ - h, seed=4, sim_offset=h)
    assert rc1 == rc2 == 0
    _equal(whole, _sum(a, b), 'long race')
    assert (whole['lap_pos'].sum(axis=2) == N_).all()
    hist, _, _ = product_run(case, N_, 4)
    assert np.array_equal(whole['hist'], hist)


def test_optional_outputs_and_the_simulator_surface():
    case = O.load_case('EVT')
    rc, full = TR.run_c(case, 4000, seed=2)
    rc2, part = TR.run_c(case, 4000, seed=2, optional=False)
    assert rc == rc2 == 0
    assert np.array_equal(full['hist'], part['hist']) and np.array_equal(full['lap_pos'], part['lap_pos'])
    assert not part['laps_led'].any() and not part['events'].any()
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=RR.SET_POP)
    res = sim.run_trace(4000, case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'],
                        case['driver_dnf_rates'], seed=2, track_condition=case['track_condition'])
    for k in KEYS:
        assert np.array_equal(getattr(res, k), full[k]), k
    probs = sim.run_monte_carlo(4000, case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'],
                                case['driver_dnf_rates'], seed=2, track_condition=case['track_condition'])
    assert res.position_probabilities == probs
    assert np.array_equal(sim.last_histogram, res.hist)
    ms = N.lib().mcgp_last_kernel_ms
    import ctypes as C
    f = C.c_float()
    sim.run_trace(4000, case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'],
                  case['driver_dnf_rates'], seed=2, track_condition=case['track_condition'])
    assert ms(0, C.byref(f)) == 0 and f.value > 0


def test_devices_all_equals_one_device():
    case = O.load_case('S60')
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    one = RaceSimulator(RaceConfig(**case['config']), device=0).run_trace(30001, *args, seed=13)
    every = RaceSimulator(RaceConfig(**case['config']), device='all').run_trace(30001, *args, seed=13)
    twice = RaceSimulator(RaceConfig(**case['config']), device=[0, 0]).run_trace(30001, *args, seed=13)
    for k in KEYS:
        assert np.array_equal(getattr(one, k), getattr(every, k)), k
        assert np.array_equal(getattr(one, k), getattr(twice, k)), k


def test_cli_predict_trace(tmp_path):
    plain, extra = tmp_path / 'plain.json', tmp_path / 'trace.json'
    base = [sys.executable, '-m', 'monte_carlo_gp_amd.cli', 'predict', '--race', 'Bahrain', '--offline',
            '--simulations', '20000', '--seed', '5']
    env = dict(os.environ, PYTHONPATH=O.ROOT)
    r1 = subprocess.run(base + ['--json', str(plain)], cwd=O.ROOT, env=env, capture_output=True, text=True, timeout=300)
    r2 = subprocess.run(base + ['--trace', '--json', str(extra)], cwd=O.ROOT, env=env, capture_output=True, text=True,
                        timeout=300)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
    for title in ('LAP LEADER', 'LAPS LED', 'FASTEST LAP', 'PIT STOPS', 'SAFETY CAR'):
        assert title in r2.stdout and title not in r1.stdout
    a, b = json.loads(plain.read_text()), json.loads(extra.read_text())
    assert {k: b[k] for k in a} == a                    # the same simulations: every existing key keeps its value
    leader = b['leader_by_lap']
    assert len(next(iter(leader.values()))) == 57
    # after the last lap the leader is the winner
    for d, p in leader.items():
        assert abs(p[-1] - a['win_probabilities'][d]) < 1e-12
    assert abs(sum(b['fastest_lap_probabilities'].values()) - 1.0) < 1e-3
