"""race_scenario_kernel<false / true, kRuleEvents> and events_count executed on the host (tools/emu/emu_generic.cpp, through
events_host_build) against three independent references:

  1. the pinned C oracle under ANOTHER config: a single override 2..L (or k + 1..L from a state) of kind K, run under
     arbitrary non-trivial event probabilities, must give the oracle's Philox finishing orders for the same seed and ids
     under probabilities 0 / 1 that make K the outcome of every lap's chain;
  2. replay: forcing on every lap exactly what the oracle's chain drew (NONE included), under probabilities 0, must give
     the oracle's order of that simulation;
  3. the Python restatement (events_ref), under mixed scenarios.

From the grid and from states after laps 1, L // 2 and L - 1, on S60, EVT and a 32-car field.  The staged data stay inside
the chunk (guard bytes on both sides, checked by events_host_build on every call); the counting kernel's bins are the
counts of the staged data whatever its grid.

Last, the comparison of tests/test_gpu_events_fuzz.py that needs no device: the generated override sets (events_cases) from
the grid on the 100 inputs of generic_cases.run_inputs() at 8 simulations."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import events_cases as EC
import events_host_build as EH
import events_ref as ER
import generic_cases as G
import kernel_host_build as KH
import oracle_py as O
import resume_ref as RR
import strategy_ref as SR

CASES = ['S60', 'EVT', 'n32']
M, SEED, OFFSET = 40, 31, 500
ARBITRARY = (0.013, 0.21, 0.17)                     # (red, sc, vsc) of the config the overridden runs are made under
STARTS = ['grid', 'lap 1', 'lap L // 2', 'lap L - 1']
# the config under which the oracle's own chain gives kind K on every lap (where the chain never gets: ARBITRARY's)
OTHER = {ER.NONE: (0.0, 0.0, 0.0), ER.RED: (1.0, ARBITRARY[1], ARBITRARY[2]), ER.SC: (0.0, 1.0, ARBITRARY[2]),
         ER.VSC: (0.0, 0.0, 1.0)}


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


def _arbitrary(name):
    return ER.with_probabilities(_case(name), *ARBITRARY)


_traced = {}


def _ref(name, probs=ARBITRARY, m=M):
    """The oracle's traced run of the case under `probs`, computed once and shared."""
    key = (name, probs, m)
    if key not in _traced:
        _traced[key] = RR.traced_run(ER.with_probabilities(_case(name), *probs), m, SEED, OFFSET)
    return _traced[key]


def _lap_of(start, L):
    return {'lap 1': 1, 'lap L // 2': L // 2, 'lap L - 1': L - 1}[start]


def test_the_restatement_without_overrides_is_strategy_ref():
    case = _arbitrary('EVT')
    L = case['config']['total_laps']
    grids = _ref('EVT')['grids']
    for plans in ({}, {0: (-1, 0, [(8, 2)]), 1: (2, 3, [(L // 2, 1), (L - 1, 0)])}):
        got, seen = ER.orders(case, 24, SEED, OFFSET, plans=plans, grids=grids)
        assert np.array_equal(got, SR.orders(case, 24, SEED, OFFSET, plans=plans, grids=grids))
        drawn = [[sum(ER.drawn_event(case, SEED, OFFSET + i, lap)[0] == k for lap in range(2, L + 1)) for k in (1, 2, 3)]
                 for i in range(24)]
        assert np.array_equal(seen, drawn)
    assert np.array_equal(ER.orders(case, 24, SEED, OFFSET, grids=grids)[0], _ref('EVT')['orders'][:24])


# ---------------------------------------------------------------- 1. whole-race overrides against the pinned oracle
@pytest.mark.parametrize('kind', [ER.NONE, ER.RED, ER.SC, ER.VSC])
@pytest.mark.parametrize('name', CASES)
def test_whole_race_override_from_the_grid_is_the_oracle_under_another_config(name, kind):
    case = _arbitrary(name)
    L = case['config']['total_laps']
    want = _ref(name, OTHER[kind])
    got = EH.events(case, None, [[(2, L, kind)]], M, SEED, OFFSET)
    bad = [i for i in range(M) if not np.array_equal(got['orders'][0, i], want['orders'][i])]
    assert not bad, f'{len(bad)} of {M} orders differ, first sim {bad[0]}'
    assert np.array_equal(got['hist'][0], RR.counts(want['orders'], len(case['grid_probs'])))
    events = np.zeros((3, L + 1), np.int64)
    events[:, 0] = M
    if kind != ER.NONE:
        events[kind - 1, 0], events[kind - 1, L - 1] = 0, M
    assert np.array_equal(got['events'][0], events)
    # ... which is what the oracle's own chain draws under the other config
    other = ER.with_probabilities(case, *OTHER[kind])
    assert all(ER.drawn_event(other, SEED, OFFSET + i, lap)[0] == kind for i in (0, M - 1) for lap in range(2, L + 1))
    if name == 'EVT' and kind == ER.NONE:
        assert not np.array_equal(want['orders'], _ref(name)['orders'])         # the override changes this race


@pytest.mark.parametrize('start', STARTS[1:])
@pytest.mark.parametrize('name', CASES)
def test_whole_race_override_from_a_state_is_the_oracle_under_another_config(name, start):
    """The state of the oracle's simulation i after lap k under the other config, continued as simulation i under the
    arbitrary config with K forced on k + 1..L, finishes as the oracle's simulation i did."""
    case = _arbitrary(name)
    L = case['config']['total_laps']
    k = _lap_of(start, L)
    prob = KH.generic_problem(case)
    for kind in (ER.NONE, ER.RED, ER.SC, ER.VSC):
        other = ER.with_probabilities(case, *OTHER[kind])
        ref = _ref(name, OTHER[kind])
        for i in (0, 5, M - 1):
            state = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(other, SEED, OFFSET + i, k))
            got = EH.events(case, None, [[(k + 1, L, kind)]], 1, SEED, OFFSET + i, state=state, prob=prob)
            assert np.array_equal(got['orders'][0, 0], ref['orders'][i]), (kind, i)
            assert got['seen'][0, 0].tolist() == [(L - k) * (kind == j) for j in (ER.RED, ER.SC, ER.VSC)]


# ---------------------------------------------------------------- 2. replay of the oracle's own draws
def _ranges(kinds, first):
    """[(first_lap, last_lap, kind)] covering laps first.. with kinds[0], kinds[1], ...: runs of one kind merged."""
    out = []
    for j, kind in enumerate(kinds):
        if out and out[-1][2] == kind:
            out[-1] = (out[-1][0], first + j, kind)
        else:
            out.append((first + j, first + j, kind))
    return out


def test_replaying_the_drawn_events_as_forced_ones_changes_nothing():
    case = O.load_case('EVT')
    L = case['config']['total_laps']
    quiet = ER.with_probabilities(case, 0.0, 0.0, 0.0)
    n_scan = 120
    ref = RR.traced_run(case, n_scan, SEED, OFFSET)
    draws = {i: [ER.drawn_event(case, SEED, OFFSET + i, lap) for lap in range(2, L + 1)] for i in range(n_scan)}
    # simulations that between them hold every kind of event, a VSC with the tyre decrement and one without
    need = {'red': lambda d: (ER.RED, False) in d or (ER.RED, True) in d,
            'sc': lambda d: (ER.SC, False) in d or (ER.SC, True) in d,
            'vsc+': lambda d: (ER.VSC, True) in d, 'vsc-': lambda d: (ER.VSC, False) in d}
    chosen = list(range(8))
    for what, has in need.items():
        hit = [i for i in range(n_scan) if has(draws[i])]
        assert hit, f'no simulation of {n_scan} drew {what}'
        chosen += hit[:2]
    chosen = sorted(set(chosen))
    held = [pair for i in chosen for pair in draws[i]]
    assert any(k == ER.RED for k, _ in held) and any(k == ER.SC for k, _ in held)
    assert (ER.VSC, True) in held and (ER.VSC, False) in held
    prob = KH.generic_problem(quiet)
    changed = 0
    for i in chosen:
        overrides = _ranges([k for k, _ in draws[i]], 2)
        assert len(overrides) <= 64
        got = EH.events(quiet, None, [overrides, []], 1, SEED, OFFSET + i, prob=prob)
        assert np.array_equal(got['orders'][0, 0], ref['orders'][i]), i
        assert got['seen'][0, 0].tolist() == [sum(k == j for k, _ in draws[i]) for j in (1, 2, 3)]
        assert got['seen'][1, 0].tolist() == [0, 0, 0]
        changed += not np.array_equal(got['orders'][1, 0], ref['orders'][i])
    assert changed >= len(chosen) // 2                      # without the replay these races end otherwise


# ---------------------------------------------------------------- 3. the restatement
def _check(case, got, scen, m, seed, offset, **kw):
    n, L = len(case['grid_probs']), case['config']['total_laps']
    want_o, want_s = [], []
    for s, (ov, pl) in enumerate(scen):
        o, seen = ER.orders(case, m, seed, offset, plans=pl, overrides=ov, **kw)
        bad = [i for i in range(m) if not np.array_equal(got['orders'][s, i], o[i])]
        assert not bad, f'scenario {s}: {len(bad)} of {m} orders differ, first sim {bad[0]}'
        assert np.array_equal(got['seen'][s], seen), f'scenario {s}: event counts differ'
        want_o.append(o)
        want_s.append(seen)
    want_o, want_s = np.stack(want_o), np.stack(want_s)
    assert np.array_equal(got['hist'], ER.hist_counts(want_o, n))
    assert np.array_equal(got['delta'], SR.delta_counts(want_o, n))
    assert np.array_equal(got['events'], ER.event_counts(want_s, L))
    assert (got['events'].sum(axis=2) == m).all()
    return want_o, want_s


@pytest.mark.parametrize('start', STARTS)
@pytest.mark.parametrize('name', CASES)
def test_emulated_kernel_equals_the_restatement(name, start):
    case = _arbitrary(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    ref = _ref(name)
    if start == 'grid':
        state, first, kw = None, 2, dict(grids=ref['grids'])
    else:
        k = _lap_of(start, L)
        state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFFSET + 3, k))
        first, kw = k + 1, dict(state=state)
    scen = ER.scenarios(first, L, n)
    got = EH.events(case, [pl for _, pl in scen], [ov for ov, _ in scen], M, SEED, OFFSET, state=state)
    want_o, want_s = _check(case, got, scen, M, SEED, OFFSET, **kw)
    if start == 'grid':
        assert np.array_equal(want_o[0], ref['orders'])
        # the scenarios do what they are there for: the contradictions and the red flags change finishing orders; the
        # forced laps are counted
        for s in (4, 5, 7):
            assert not np.array_equal(want_o[s], want_o[0]), s
        assert (want_s[4] == 0).all() and (want_s[5] == [0, 0, L - 1]).all()
        assert (want_s[1][:, 1] >= 1).all() and (want_s[7][:, 0] >= 2).all()
        drawn = {ER.drawn_event(case, SEED, OFFSET + i, 2)[0] for i in range(M)}
        assert len(drawn - {ER.SC}) >= 1            # scenario 1 forces a safety car where the draw gave something else


def test_sixty_four_scenarios_of_sixty_four_single_lap_overrides():
    case = ER.with_probabilities(RR.field_case(3), *ARBITRARY)
    case['config'] = dict(case['config'], total_laps=70)
    scen = [([(lap, lap, (s + lap) % 4) for lap in range(2, 66)], {}) for s in range(64)]
    m = 2
    got = EH.events(case, None, [ov for ov, _ in scen], m, SEED, 9)
    _check(case, got, scen, m, SEED, 9)


def test_a_thousand_laps():
    case = ER.with_probabilities(RR.field_case(2), *ARBITRARY)
    case['config'] = dict(case['config'], total_laps=1000)
    case['driver_dnf_rates'] = {d: 0.0002 for d in case['driver_dnf_rates']}
    scen = [([], {}), ([(2, 1000, ER.VSC)], {}), ([(2, 500, ER.RED), (501, 1000, ER.SC)], {}),
            ([(1000, 1000, ER.SC)], {0: (-1, 0, [(1000, 1)])})]
    m = 2
    got = EH.events(case, [pl for _, pl in scen], [ov for ov, _ in scen], m, SEED, 1)
    _, seen = _check(case, got, scen, m, SEED, 1)
    assert (seen[1] == [0, 0, 999]).all() and (seen[2] == [499, 500, 0]).all()     # the 10-bit counters hold 999


# ---------------------------------------------------------------- identities and the counting kernel
def test_scenarios_without_overrides_are_the_strategy_kernel():
    case = _arbitrary('EVT')
    L = case['config']['total_laps']
    plans = [{}, {0: (-1, 0, [(8, 2)])}, {1: (-1, 0, [(15, 1), (L - 5, 0)]), 0: (-1, 0, [])}]
    hist, orders = KH.generic_strategy(case, plans, M, SEED, OFFSET)
    got = EH.events(case, plans, [[]] * 3, M, SEED, OFFSET)
    assert np.array_equal(got['orders'], orders) and np.array_equal(got['hist'], hist)
    assert np.array_equal(got['seen'][0], got['seen'][1])           # a plan moves no event
    ref = _ref('EVT')
    k = L // 2
    state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFFSET + 3, k))
    plans = [{}, {0: (-1, 0, [(k + 1, 2)])}]
    hist, orders = KH.generic_strategy(case, plans, M, SEED, OFFSET, state=state)
    got = EH.events(case, plans, [[]] * 2, M, SEED, OFFSET, state=state)
    assert np.array_equal(got['orders'], orders) and np.array_equal(got['hist'], hist)


@pytest.mark.parametrize('grid_x', [1, 3, 7])
def test_counting_kernel_does_not_depend_on_its_grid(grid_x):
    case = _arbitrary('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    scen = ER.scenarios(2, L, n)
    plans, ovs = [pl for _, pl in scen], [ov for ov, _ in scen]
    m = 37                                                  # no multiple of any grid
    hist, stage, evs, delta, events = EH.events_raw(case, plans, ovs, m, SEED, 11, grid_x=grid_x)
    orders, seen = EH.decode(stage, evs)
    want_d = SR.delta_counts(orders, n)
    want_d[:, :, n - 1] = 0                                 # the centre bin is the host's
    assert np.array_equal(delta, want_d) and np.array_equal(events, ER.event_counts(seen, L))
    assert np.array_equal(hist, ER.hist_counts(orders, n))
    assert (events.sum(axis=2) == m).all()
    # without the counting kernel nothing is counted
    _, stage2, evs2, d2, e2 = EH.events_raw(case, plans, ovs, m, SEED, 11, count=False)
    assert np.array_equal(stage2, stage) and np.array_equal(evs2, evs) and not d2.any() and not e2.any()


# ---------------------------------------------------------------- every input under generated override sets
FUZZ_SIMS, FUZZ_OFFSET = 8, 3


def test_emulated_kernel_on_every_input_from_the_grid():
    inputs = G.run_inputs()
    O.lib()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        refs = list(pool.map(lambda a: RR.traced_run(a[1], FUZZ_SIMS, a[2], FUZZ_OFFSET), inputs))
    done = contradicted = stops = moved = 0
    for (name, case, seed), ref in zip(inputs, refs):
        scen, c = EC.scenarios(name, case, seed, FUZZ_OFFSET, 2)
        contradicted += c > 0
        stops += len(scen) > 1 and bool(scen[1][1])
        got = EH.events(case, [pl for _, pl in scen], [ov for ov, _ in scen], FUZZ_SIMS, seed, FUZZ_OFFSET)
        want_o, _ = _check(case, got, scen, FUZZ_SIMS, seed, FUZZ_OFFSET, grids=ref['grids'])
        assert np.array_equal(want_o[0], ref['orders']), name
        moved += any(not np.array_equal(want_o[s], want_o[0]) for s in range(1, len(scen)))
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and len(inputs) == 100
    assert contradicted >= 97 and stops >= 90 and moved >= 80, (contradicted, stops, moved)
