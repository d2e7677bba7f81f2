"""The comparisons of test_generic_host_build.py on the device, through the C ABI: mcgp_run_trace (race_trace_kernel and
its three counting kernels), mcgp_run_from_state (race_resume_kernel) and mcgp_run_strategies (race_strategy_kernel
<false> and <true>, strategy_count_deltas) with the host side's chunking, on the 84 fuzz configurations with their 12
corner cases, on lap times near zero, and at the limits of include/mcgp.h (1000 laps, 8 stops, 64 scenarios x 32 plans).

References, none of which shares code with the kernels: trace_ref.trace_counts and resume_ref's states from the CPU
oracle's per-lap trace, the oracle's finishing orders, and the Python restatement strategy_ref.orders.  Every comparison
is on integers, bit for bit.  The oracle side runs on the host in a pool of at most 16 threads.

Compared on the device: trace 301 simulations on 100 inputs (8 golden, 84 fuzz, 2 with tiny lap times, 6 field sizes) and
two 1000-lap runs across staging chunks; resume 16 simulations x up to 7 laps on 94 inputs and 10^5 simulations from a
state of three corner cases; strategies 16 simulations x (6 + 2) scenarios on 75 + 2 configurations, the 1000-lap and
the 64 x 32 x 8 call.  Cost on an MI355X machine: 19.9 s for this file (11.4 s of it the Python restatement of the
strategy scenarios, which is why they run the 16-simulation floor) against 8.1 s for tests/test_gpu_fuzz.py in the same
visit -- 2.5 times that file, above the factor of two aimed for."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import generic_cases as G
import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
import trace_ref as TR
from helpers import product_run
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

TRACE_SIMS, RESUME_SIMS, STRATEGY_SIMS = 301, 16, 16
KEYS = ('hist', 'lap_pos', 'laps_led', 'stops', 'fastest', 'events')


def _pool():
    return ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))


def _check(rc):
    assert rc == 0, N.lib().mcgp_last_error().decode()


def _kernel():
    return N.lib().mcgp_last_kernel_name(0).decode()


def _same_orders(got, want, what):
    bad = np.nonzero((got != want).any(axis=-1).reshape(-1))[0]
    assert bad.size == 0, f'{what}: {bad.size} finishing orders differ, first {bad[:5]}'


# ---------------------------------------------------------------- mcgp_run_trace
def test_trace_on_every_configuration(require_gpu):
    inputs = G.run_inputs()
    O.lib()
    with _pool() as pool:
        refs = list(pool.map(lambda a: TR.trace_counts(a[1], TRACE_SIMS, a[2], 3), inputs))
    done = 0
    for (name, case, seed), ref in zip(inputs, refs):
        if name == 'X_no_noise':
            assert G.smallest_lap_time_ties(RR.traced_run(case, TRACE_SIMS, seed, 3)) >= 1
        rc, got = TR.run_c(case, TRACE_SIMS, seed, sim_offset=3)
        _check(rc)
        assert _kernel() == 'mcgp::race_trace_kernel', name
        for key in KEYS:
            assert np.array_equal(got[key], ref[key]), (name, key)
        hist, _, _ = product_run(case, TRACE_SIMS, seed, sim_offset=3)
        assert np.array_equal(got['hist'], hist), name
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ


def _thousand_laps(n, dnf):
    case = RR.field_case(n)
    case = dict(case, config=dict(case['config'], total_laps=1000))
    case['driver_dnf_rates'] = {d: dnf for d in case['base_pace']}
    return case


@pytest.mark.parametrize('n', [10, 32])
def test_trace_of_a_thousand_laps_across_staging_chunks(require_gpu, n):
    """MCGP_MAX_LAPS: 1001 bins, 1000 n staging rows of which a chunk holds 512 MiB / (1000 n) simulations; a run of a
    little more than two chunks equals the sum of its halves, and a few simulations equal the oracle's trace."""
    case = _thousand_laps(n, 0.002)
    rc, got = TR.run_c(case, 40, seed=6)
    _check(rc)
    ref = TR.trace_counts(case, 40, 6)
    for key in KEYS:
        assert np.array_equal(got[key], ref[key]), key
    N_ = 2 * TR.budget_sims(n, 1000) + 1001
    rc, whole = TR.run_c(case, N_, seed=6)
    _check(rc)
    assert _kernel() == 'mcgp::race_trace_kernel'
    h = N_ // 2 + 3
    rc1, a = TR.run_c(case, h, seed=6)
    rc2, b = TR.run_c(case, N_ - h, seed=6, sim_offset=h)
    _check(rc1)
    _check(rc2)
    for key in KEYS:
        assert np.array_equal(whole[key], a[key] + b[key]), key
    assert (whole['lap_pos'].sum(axis=2) == N_).all()
    assert (whole['laps_led'].sum(axis=1) == N_).all() and (whole['events'].sum(axis=1) == N_).all()
    hist, _, _ = product_run(case, N_, 6)
    assert np.array_equal(whole['hist'], hist)


# ---------------------------------------------------------------- mcgp_run_from_state
def _resume_states(case, seed, m=RESUME_SIMS, base=40):
    ref = RR.traced_run(case, m, seed, base)
    states, offs, want = [], [], []
    for i in range(m):
        for k in G.resume_laps(case, seed, base + i):
            states.append((RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k)))
            offs.append(base + i)
            want.append(ref['orders'][i])
    return states, offs, np.array(want)


def test_resume_on_every_configuration(require_gpu):
    inputs = G.resume_inputs()
    O.lib()
    with _pool() as pool:
        prepared = list(pool.map(lambda a: _resume_states(a[1], a[2]), inputs))
    done = 0
    for (name, case, seed), (states, offs, want) in zip(inputs, prepared):
        rc, hist, orders = RR.run_c(RR.problem(case), states, 1, offs, seed)
        _check(rc)
        assert _kernel() == 'mcgp::race_resume_kernel', name
        _same_orders(orders[:, 0, :], want, name)
        for s in range(len(states)):
            assert np.array_equal(hist[s], RR.counts(orders[s], orders.shape[2])), (name, s)
        if name in G.GOLDEN:
            assert any(dd > 0 for _, _, dd in states), name
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ


@pytest.mark.parametrize('name', ['X_all_out_lap1', 'X_all_out_lap2', 'X_half_out'])
def test_many_simulations_from_a_state_with_retirements(require_gpu, name):
    """10^5 simulations from one state of a race in which cars are certain or likely to be out: the histogram is the
    count of the orders, a split over two calls sums, and the first simulations are the restatement's."""
    case = G.fuzz_cases()[name]
    seed, L, m = case['seed'], case['config']['total_laps'], 100_000
    ref = RR.traced_run(case, 1, seed, 7)
    k = G.many_from_one_lap(ref, 0, L)
    st = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, 7, k))
    prob, n = RR.problem(case), len(case['grid_probs'])
    rc, hist, orders = RR.run_c(prob, [st], m, [100], seed)
    _check(rc)
    assert _kernel() == 'mcgp::race_resume_kernel'
    assert np.array_equal(hist[0], RR.counts(orders[0], n))
    _same_orders(orders[0][:48], SR.orders(case, 48, seed, 100, state=st), name)
    a = 33_333
    rc1, h1, _ = RR.run_c(prob, [st], a, [100], seed, orders=False)
    rc2, h2, _ = RR.run_c(prob, [st], m - a, [100 + a], seed, orders=False)
    _check(rc1)
    _check(rc2)
    assert np.array_equal(h1 + h2, hist)


# ---------------------------------------------------------------- mcgp_run_strategies
def _strategy_case(name, case, seed, m=STRATEGY_SIMS):
    """Both strategy kernels on one configuration against the restatement.  (That the plans change finishing orders on
    these configurations is asserted, from the restatement alone, by test_generic_host_build.py.)"""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    prob = RR.problem(case)
    scen = G.grid_scenarios(n, L)
    traced = RR.traced_run(case, m, seed, 0)
    want = np.stack([SR.orders(case, m, seed, 0, plans=sc, grids=traced['grids']) for sc in scen])
    rc, hist, delta, orders = SR.run_c(case, scen, m, seed, prob=prob)
    _check(rc)
    assert _kernel() == 'mcgp::race_strategy_kernel', name
    _same_orders(orders, want, name + ' from the grid')
    assert np.array_equal(delta, SR.delta_counts(orders, n)), name
    for s in range(len(scen)):
        assert np.array_equal(hist[s], RR.counts(orders[s], n)), (name, s)
    run_hist, _, run_orders = product_run(case, m, seed, orders=True)
    assert np.array_equal(orders[0], run_orders) and np.array_equal(hist[0], run_hist), name       # {} is mcgp_run
    # from the oracle's state of simulation 0 after L // 2, continued as simulations 0 .. m - 1
    k = L // 2
    st = (RR.state_arrays(traced, 0, k), k, RR.drs_disabled_until(case, seed, 0, k))
    scen_k = G.state_scenarios(n, L, k)
    want_k = np.stack([SR.orders(case, m, seed, 0, plans=sc, state=st) for sc in scen_k])
    rc, hist, delta, orders = SR.run_c(case, scen_k, m, seed, state=st, prob=prob)
    _check(rc)
    assert _kernel() == 'mcgp::race_strategy_kernel', name
    _same_orders(orders, want_k, name + ' from a state')
    assert np.array_equal(delta, SR.delta_counts(orders, n)), name
    for s in range(len(scen_k)):
        assert np.array_equal(hist[s], RR.counts(orders[s], n)), (name, s)


def test_strategies_on_every_configuration_of_eight_laps_or_more(require_gpu):
    inputs = G.strategy_inputs()
    assert len(inputs) == G.N_FUZZ_STRATEGY
    for name, case, seed in inputs:
        _strategy_case(name, case, seed)


def test_strategies_with_lap_times_near_zero(require_gpu):
    _strategy_case('near_zero', G.near_zero_case(), 11)
    _strategy_case('floor', G.floor_case(), 11)


def test_strategy_of_a_thousand_laps_at_the_largest_start_age(require_gpu):
    """total_laps = 1000, start_age = 1023 - L = 23 and no stop: the tyre age ends the race at 1023."""
    case = _thousand_laps(10, 0.0003)
    scen = [{}, {0: (G.HARD, 23, [])}, {9: (G.MEDIUM, 23, [(1000, G.SOFT)])}]
    grids = RR.traced_run(case, 3, 3)['grids']
    want = np.stack([SR.orders(case, 3, 3, plans=sc, grids=grids) for sc in scen])
    rc, hist, delta, orders = SR.run_c(case, scen, 3, 3)
    _check(rc)
    assert _kernel() == 'mcgp::race_strategy_kernel'
    _same_orders(orders, want, 'L1000')
    assert np.array_equal(delta, SR.delta_counts(orders, 10))


def test_sixty_four_scenarios_of_thirty_two_plans_of_eight_stops(require_gpu):
    """Every limit of a call at once: 64 scenarios, a plan for each of 32 drivers, MCGP_MAX_PLAN_STOPS = 8 stops each,
    on consecutive laps in half of the scenarios."""
    n, m, seed = 32, 6, 13
    case = RR.field_case(n)
    L = case['config']['total_laps']
    assert L >= 2 + 8 + 7
    scen = []
    for s in range(64):
        plans = {}
        for d in range(n):
            first = 2 + (s + d) % (L - 9) if s % 2 == 0 else 2 + (s + d) % 3
            step = 1 if s % 2 == 0 else 3
            laps = [first + step * j for j in range(8)]
            assert laps[-1] <= L
            plans[d] = (-1, 0, [(lap, (lap + d + s) % 3) for lap in laps])
        scen.append(plans)
    grids = RR.traced_run(case, m, seed)['grids']
    want = np.stack([SR.orders(case, m, seed, plans=sc, grids=grids) for sc in scen])
    rc, hist, delta, orders = SR.run_c(case, scen, m, seed)
    _check(rc)
    assert _kernel() == 'mcgp::race_strategy_kernel'
    _same_orders(orders, want, '64 x 32 x 8')
    assert np.array_equal(delta, SR.delta_counts(orders, n))
    for s in range(64):
        assert np.array_equal(hist[s], RR.counts(orders[s], n)), s
