"""The generic kernel family's SOURCE -- race_kernel, race_resume_kernel, race_trace_kernel, race_strategy_kernel<false>
and <true>, i.e. run_block, start_from_grid, start_from_state, run_laps and classify_and_count -- compiled for the
host (tools/emu/emu_generic.cpp) and compared bit for bit, integers only, with references that do not share its code:
the CPU oracle's finishing orders and per-lap trace, trace_ref.trace_counts, and the Python restatement
strategy_ref.orders (pinned to the oracle on the same configurations by test_strategy_host.py).

Inputs (generic_cases.py): the 8 golden cases, the 84 fuzz configurations with their 12 corner cases, a field lapping in
5 s, synthetic fields of 1, 2, 3, 19, 31 and 32 cars, 1000-lap races.  A CPU-side net for an edit to the code five kernels
share; the counting kernels and the host-side chunking are compared on the device (test_gpu_generic_fuzz.py).  The host
build is test infrastructure: nothing under monte_carlo_gp_amd/ can reach it and the product has no CPU path.

Compared per kernel: race_kernel 100 and race_trace_kernel 32 simulations on 100 inputs (8 golden, 84 fuzz, 2 with tiny lap
times, 6 field sizes); race_resume_kernel 16 simulations x up to 7 laps on 94; both strategy kernels 32 simulations x (6 +
2) scenarios on the 75 fuzz configurations of 8 laps or more and on the 2 with tiny lap times.  Cost: 62 s on the 8-core
machine this was written on, 47 s of it the Python restatement of the strategy comparisons (the build itself: 2 s);
tests/test_kernel_host_build.py takes 96 s there, build included."""
import copy

import numpy as np
import pytest

import generic_cases as G
import kernel_host_build as K
import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
import trace_ref as TR

RUN_SIMS, TRACE_SIMS, RESUME_SIMS, STRATEGY_SIMS = 100, 32, 16, 32


def _same_orders(got, want, what):
    bad = np.nonzero((got != want).any(axis=-1).reshape(-1))[0]
    assert bad.size == 0, f'{what}: {bad.size} finishing orders differ, first {bad[:5]}'


# ---------------------------------------------------------------- race_kernel
def test_race_kernel_equals_the_oracle():
    done = 0
    for name, case, seed in G.run_inputs():
        ref = O.Problem(case).run(RUN_SIMS, rng=O.RNG_PHILOX, seed=seed, sim_offset=3, want_orders=True)
        hist, orders = K.generic_run(case, RUN_SIMS, seed, sim_offset=3)
        _same_orders(orders, ref['orders'], name)
        assert np.array_equal(hist, ref['hist']), name
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ


def test_race_kernel_takes_a_fixed_grid():
    case = O.load_case('S60')
    grid = np.arange(20, dtype=np.uint8)[::-1].copy()
    want = SR.orders(case, 24, 9, grids=[grid] * 24)            # (the oracle samples its grids: the restatement takes one)
    hist, orders = K.generic_run(case, 24, 9, fixed_grid=grid)
    _same_orders(orders, want, 'fixed grid')
    assert np.array_equal(hist, RR.counts(orders, 20))


# ---------------------------------------------------------------- race_trace_kernel
def _compare_trace(name, got, ref):
    for key in ('hist', 'lap_pos', 'laps_led', 'stops', 'fastest', 'events'):
        assert np.array_equal(got[key], ref[key]), (name, key)


def test_trace_kernel_equals_the_restated_counts():
    done = 0
    for name, case, seed in G.run_inputs():
        if name == 'X_no_noise':
            # the fastest lap's tie-break is only exercised if ties occur: asserted from the oracle's trace alone
            assert G.smallest_lap_time_ties(RR.traced_run(case, TRACE_SIMS, seed, 3)) >= 1
        got = K.generic_trace(case, TRACE_SIMS, seed, sim_offset=3)
        _compare_trace(name, got, TR.trace_counts(case, TRACE_SIMS, seed, 3))
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ


def _thousand_laps(dnf=0.002):
    case = copy.deepcopy(O.load_case('N10'))
    case['config']['total_laps'] = 1000
    case['driver_dnf_rates'] = {d: dnf for d in case['base_pace']}            # 0.002: most cars out somewhere in 1000 laps
    return case


def test_trace_of_a_thousand_lap_race():
    """MCGP_MAX_LAPS: 1000 n staging rows, event and lap counts up to 1000."""
    case = _thousand_laps()
    got, ref = K.generic_trace(case, 6, 3), TR.trace_counts(case, 6, 3)
    _compare_trace('L1000', got, ref)
    assert got['lap_pos'].shape == (1000, 10, 11) and got['events'].shape == (3, 1001)


# ---------------------------------------------------------------- race_resume_kernel
def _resume_case(name, case, seed, m=RESUME_SIMS, base=40):
    """Simulation i's state after every lap of G.resume_laps, resumed as simulation i: the oracle's order of i.  Returns
    the number of resumed states and of those with drs_disabled_until > 0."""
    ref = RR.traced_run(case, m, seed, base)
    states, offs, want = [], [], []
    for i in range(m):
        for k in G.resume_laps(case, seed, base + i):
            states.append((RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k)))
            offs.append(base + i)
            want.append(ref['orders'][i])
    hist, orders = K.generic_resume(case, states, 1, offs, seed)
    _same_orders(orders[:, 0, :], np.array(want), name)
    for s in range(len(states)):
        assert np.array_equal(hist[s], RR.counts(orders[s], orders.shape[2])), (name, s)
    return len(states), sum(dd > 0 for _, _, dd in states)


def test_resume_kernel_continues_into_the_oracle_order():
    done = 0
    for name, case, seed in G.resume_inputs():
        n_states, with_events = _resume_case(name, case, seed)
        assert n_states >= RESUME_SIMS
        if name in G.GOLDEN:
            assert with_events > 0, name           # a state whose DRS is still off after an event, in every golden case
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ


@pytest.mark.parametrize('name', ['X_half_out', 'X_all_out_lap2', 'X_all_out_lap1', 'X_no_noise', 'F05', 'F40'])
def test_resume_redraws_what_contradicts_the_state(name):
    """One state continued as MANY simulations: their own retirement draws may name a lap the state has already seen the
    car survive (redrawn: draw_retirement_lap_after), and a field rebuilt from state arrays with equal times orders by
    grid slot.  Reference: the restatement from the same state."""
    case = G.fuzz_cases()[name]
    seed, L = case['seed'], case['config']['total_laps']
    ref = RR.traced_run(case, 1, seed, 7)
    k = G.many_from_one_lap(ref, 0, L)
    st = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, 7, k))
    m = 48
    _, orders = K.generic_resume(case, [st], m, [100], seed)
    _same_orders(orders[0], SR.orders(case, m, seed, 100, state=st), name)


def test_resume_at_the_largest_tyre_age():
    """total_laps = 1000 and tire_age = 1023 - (L - lap), the largest the header admits: the age field of pk ends the race
    at 1023 (no stop in the last 5 laps) without touching the compound bits."""
    case = _thousand_laps(dnf=0.0003)
    L, k, seed = 1000, 995, 3
    ref = RR.traced_run(case, 2, seed)
    for i in range(2):
        a = RR.state_arrays(ref, i, k)
        assert (a['retired_lap'] == 0).sum() >= 5
        a['tire_age'] = np.where(a['retired_lap'] == 0, 1023 - (L - k), a['tire_age']).astype(np.int16)
        st = (a, k, RR.drs_disabled_until(case, seed, i, k))
        _, orders = K.generic_resume(case, [st], 3, [i], seed)
        _same_orders(orders[0], SR.orders(case, 3, seed, i, state=st), f'L1000 sim {i}')


# ---------------------------------------------------------------- race_strategy_kernel
def _strategy_case(name, case, seed, m=STRATEGY_SIMS):
    """Both strategy kernels on one configuration against the restatement; returns whether a plan changed a finishing
    order from the grid (decided from the restatement alone, over the 32 simulations)."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    prob = K.generic_problem(case)
    # from the grid
    scen = G.grid_scenarios(n, L)
    traced = RR.traced_run(case, m, seed, 0)
    want = np.stack([SR.orders(case, m, seed, 0, plans=sc, grids=traced['grids']) for sc in scen])
    hist, orders = K.generic_strategy(case, scen, m, seed, prob=prob)
    _same_orders(orders, want, name + ' from the grid')
    for s in range(len(scen)):
        assert np.array_equal(hist[s], RR.counts(orders[s], n)), (name, s)
    run_hist, run_orders = K.generic_run(case, m, seed, prob=prob)
    assert np.array_equal(orders[0], run_orders) and np.array_equal(hist[0], run_hist), name       # {} is mcgp_run
    bites = any((want[s] != want[0]).any() for s in range(1, len(scen)))
    # from the oracle's state of simulation 0 after L // 2, continued as simulations 0 .. m - 1
    k = L // 2
    st = (RR.state_arrays(traced, 0, k), k, RR.drs_disabled_until(case, seed, 0, k))
    scen = G.state_scenarios(n, L, k)
    want = np.stack([SR.orders(case, m, seed, 0, plans=sc, state=st) for sc in scen])
    hist, orders = K.generic_strategy(case, scen, m, seed, state=st, prob=prob)
    _same_orders(orders, want, name + ' from a state')
    res_hist, res_orders = K.generic_resume(case, [st], m, [0], seed, prob=prob)
    assert np.array_equal(orders[0], res_orders[0]) and np.array_equal(hist[0], res_hist[0]), name  # {} is a resume
    return bites


def test_strategy_kernels_equal_the_restatement():
    inputs = G.strategy_inputs()
    assert len(inputs) == G.N_FUZZ_STRATEGY
    tame = [name for name, case, seed in inputs if not _strategy_case(name, case, seed)]
    assert len(G.NO_BITE) <= 4 and set(tame) <= set(G.NO_BITE), tame


def test_strategy_kernels_with_lap_times_near_zero():
    assert _strategy_case('near_zero', G.near_zero_case(), 11)
    assert _strategy_case('floor', G.floor_case(), 11)


def test_strategy_at_the_largest_start_age():
    """total_laps = 1000, start_age = 1023 - L = 23 and no stop: the car's tyre age ends the race at 1023."""
    case = _thousand_laps(dnf=0.0003)
    scen = [{}, {0: (G.HARD, 23, [])}, {9: (G.MEDIUM, 23, [(1000, G.SOFT)])}]
    grids = RR.traced_run(case, 2, 3)['grids']
    want = np.stack([SR.orders(case, 2, 3, plans=sc, grids=grids) for sc in scen])
    _, orders = K.generic_strategy(case, scen, 2, 3)
    _same_orders(orders, want, 'L1000')
