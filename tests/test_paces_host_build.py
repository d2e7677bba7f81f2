"""race_scenario_kernel<false / true, kRulePaces> and paces_count executed on the host (tools/emu/emu_generic.cpp, through
paces_host_build) against two independent references:

  1. the pinned C oracle under ANOTHER base_pace: a LAPS offset [1, L] (or [k + 1, L] from a state) of x_d on every
     driver must give the oracle's Philox finishing orders for the same seed and ids under base_pace[d] + x_d (the sum
     formed here, the same binary64 addition); an UNTIL_STOP offset that no stop clears likewise;
  2. the Python restatement (paces_ref), under mixed scenarios.

From the grid and from states after laps 1, L // 2 and L - 1, on S60, EVT and a 32-car field.  The staged data stay inside
the chunk (guard bytes on both sides, checked by paces_host_build on every call); the counting kernel's bins are the
counts of the staged data whatever its grid.

Last, the comparison of tests/test_gpu_paces.py that needs no device: the generated offset sets (paces_cases) from the
grid on the 100 inputs of generic_cases.run_inputs() and from states on the 94 of resume_inputs(), at 8 simulations."""
import functools

import numpy as np
import pytest

import kernel_host_build as KH
import oracle_py as O
import paces_cases as PC
import paces_host_build as PH
import paces_ref as PR
import resume_ref as RR
import strategy_ref as SR

CASES = ['S60', 'EVT', 'n32']
ORACLE_CASES = ['S60', 'EVT', 'n32', 'n2', 'n1']
M, SEED, OFFSET = 40, 47, 300
STARTS = ['grid', 'lap 1', 'lap L // 2', 'lap L - 1']
X = [0.37, -0.21, 0.113, -0.57, 0.29, -0.083, 0.61]      # not round in binary, mixed signs


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


def _x(n):
    """x_d of every driver: mixed signs, exactly one 0.0 (where there are two drivers)."""
    x = [X[d % 7] + 0.001 * (d // 7) for d in range(n)]
    if n >= 2:
        x[min(2, n - 1)] = 0.0
    return x


_traced = {}


def _ref(name, shifted=False, m=M):
    """The oracle's traced run of the case, under base_pace (or base_pace[d] + x_d), computed once and shared."""
    key = (name, shifted, m)
    if key not in _traced:
        case = _case(name)
        if shifted:
            case = PR.with_base_pace(case, _x(len(case['grid_probs'])))
        _traced[key] = RR.traced_run(case, m, SEED, OFFSET)
    return _traced[key]


def _lap_of(start, L):
    return {'lap 1': 1, 'lap L // 2': L // 2, 'lap L - 1': L - 1}[start]


def test_the_restatement_without_offsets_is_strategy_ref():
    case = _case('EVT')
    L = case['config']['total_laps']
    grids = _ref('EVT')['grids']
    for plans in ({}, {0: (-1, 0, [(8, 2)]), 1: (2, 3, [(L // 2, 1), (L - 1, 0)])}):
        got, carried = PR.orders(case, 24, SEED, OFFSET, plans=plans, grids=grids)
        assert np.array_equal(got, SR.orders(case, 24, SEED, OFFSET, plans=plans, grids=grids))
        assert not carried.any()
    assert np.array_equal(PR.orders(case, 24, SEED, OFFSET, grids=grids)[0], _ref('EVT')['orders'][:24])


# ---------------------------------------------------------------- 1. whole-race offsets against the pinned oracle
@pytest.mark.parametrize('name', ORACLE_CASES)
def test_whole_race_offsets_from_the_grid_are_the_oracle_under_another_base_pace(name):
    case = _case(name)
    n, L = len(case['grid_probs']), case['config']['total_laps']
    x = _x(n)
    same, want = _ref(name), _ref(name, shifted=True)
    got = PH.paces(case, None, [[], [PR.laps(d, 1, L, x[d]) for d in range(n)]], M, SEED, OFFSET)
    for s, ref in enumerate((same, want)):
        bad = [i for i in range(M) if not np.array_equal(got['orders'][s, i], ref['orders'][i])]
        assert not bad, f'scenario {s}: {len(bad)} of {M} orders differ, first sim {bad[0]}'
        assert np.array_equal(got['hist'][s], RR.counts(ref['orders'], n))
    assert np.array_equal(got['delta'], SR.delta_counts(np.stack([same['orders'], want['orders']]), n))
    assert (got['carried'][:, :, 0] == M).all() and not got['carried'][:, :, 1:].any()
    # the offset matters: the oracle's race under the other base pace is another race
    assert not np.array_equal(want['trace']['cum'], same['trace']['cum'])
    if n >= 2:
        assert not np.array_equal(want['orders'], same['orders'])
    assert x.count(0.0) == (n >= 2) and (n < 3 or min(x) < 0 < max(x))


@pytest.mark.parametrize('start', STARTS[1:])
@pytest.mark.parametrize('name', ORACLE_CASES)
def test_whole_race_offsets_from_a_state_are_the_oracle_under_another_base_pace(name, start):
    """The state of the oracle's simulation i after lap k under base_pace[d] + x_d, continued as simulation i under the
    original case with LAPS [k + 1, L] of x_d on every driver, finishes as that oracle simulation did."""
    case = _case(name)
    n, L = len(case['grid_probs']), case['config']['total_laps']
    k = _lap_of(start, L)
    x = _x(n)
    ref = _ref(name, shifted=True)
    prob = KH.generic_problem(case)
    offs = [PR.laps(d, k + 1, L, x[d]) for d in range(n)]
    for i in (0, 5, 17, M - 1):
        state = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, SEED, OFFSET + i, k))
        got = PH.paces(case, None, [offs], 1, SEED, OFFSET + i, state=state, prob=prob)
        assert np.array_equal(got['orders'][0, 0], ref['orders'][i]), i


def test_until_stop_that_no_stop_clears_is_the_oracle_under_another_base_pace():
    """L = 5: the rule needs remaining_laps > 5, so nobody stops, and driver 0's offset from lap 1 runs to the flag."""
    case = dict(O.load_case('S60'))
    case['config'] = dict(case['config'], total_laps=5)
    case['driver_dnf_rates'] = {d: 0.05 for d in case['driver_dnf_rates']}
    n, L, x = len(case['grid_probs']), 5, 0.437
    same = RR.traced_run(case, M, SEED, OFFSET)
    want = RR.traced_run(PR.with_base_pace(case, [x] + [0.0] * (n - 1)), M, SEED, OFFSET)
    got = PH.paces(case, None, [[], [PR.until_stop(0, 1, x)]], M, SEED, OFFSET)
    assert np.array_equal(got['orders'][0], same['orders']) and np.array_equal(got['orders'][1], want['orders'])
    assert not np.array_equal(want['orders'], same['orders'])
    tr = want['trace']
    out = np.where(tr['dnf'][:, L - 1, 0] != 0, tr['dnf_lap'][:, L - 1, 0], 0)       # driver 0's retirement lap, or 0
    assert np.array_equal(got['laps'][1][:, 0], np.where(out != 0, out - 1, 5))
    assert (out != 0).any() and (out == 0).any()
    assert np.array_equal(got['carried'][1, 0], np.bincount(np.where(out != 0, out - 1, 5), minlength=L + 1))
    assert (got['carried'][0, :, 0] == M).all() and (got['carried'][1, 1:, 0] == M).all()


# ---------------------------------------------------------------- 2. the restatement
def _check(case, got, scen, m, seed, offset, **kw):
    n, L = len(case['grid_probs']), case['config']['total_laps']
    want_o, want_c = [], []
    for s, (offs, pl) in enumerate(scen):
        o, carried = PR.orders(case, m, seed, offset, plans=pl, offsets=offs, **kw)
        bad = [i for i in range(m) if not np.array_equal(got['orders'][s, i], o[i])]
        assert not bad, f'scenario {s}: {len(bad)} of {m} orders differ, first sim {bad[0]}'
        assert np.array_equal(got['laps'][s], carried), f'scenario {s}: laps carried differ'
        want_o.append(o)
        want_c.append(carried)
    want_o, want_c = np.stack(want_o), np.stack(want_c)
    assert np.array_equal(got['hist'], PR.hist_counts(want_o, n))
    assert np.array_equal(got['delta'], SR.delta_counts(want_o, n))
    assert np.array_equal(got['carried'], PR.carried_counts(want_c, L))
    assert (got['carried'].sum(axis=2) == m).all()
    return want_o, want_c


@pytest.mark.parametrize('start', STARTS)
@pytest.mark.parametrize('name', CASES)
def test_emulated_kernel_equals_the_restatement(name, start):
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    ref = _ref(name)
    if start == 'grid':
        state, first, kw = None, 1, dict(grids=ref['grids'])
    else:
        k = _lap_of(start, L)
        state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFFSET + 3, k))
        first, kw = k + 1, dict(state=state)
    scen = PR.scenarios(first, L, n)
    got = PH.paces(case, [pl for _, pl in scen], [offs for offs, _ in scen], M, SEED, OFFSET, state=state)
    want_o, want_c = _check(case, got, scen, M, SEED, OFFSET, **kw)
    if start == 'grid':
        assert np.array_equal(want_o[0], ref['orders'])
        # the scenarios do what they are there for: every one changes finishing orders; a rule stop clears scenario 4's
        # offsets in some simulation; the planned stop of scenario 5 clears its offset after one lap wherever the car
        # still runs; scenario 6's plan has no stop, so its offset is carried to the flag or to the retirement
        for s in range(1, len(scen)):
            assert not np.array_equal(want_o[s], want_o[0]), s
        assert ((want_c[4][:, n - 1] > 0) & (want_c[4][:, n - 1] < L - 5)).any()
        assert set(np.unique(want_c[5][:, 0])) <= {0, 1} and (want_c[5][:, 0] == 1).sum() > M // 2
        assert (want_c[6][:, n - 1] == L).any() and (want_c[6][:, n - 1] < L).any()


def test_offsets_of_cars_that_retire_before_and_after_their_first_lap():
    case = dict(O.load_case('S60'))
    case['driver_dnf_rates'] = {d: 0.03 for d in case['driver_dnf_rates']}
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    p = L // 2
    who = [0, 7, n - 1]
    scen = [([], {}), ([PR.until_stop(d, p, 0.45 + 0.1 * d) for d in who], {d: (-1, 0, []) for d in who})]
    got = PH.paces(case, [pl for _, pl in scen], [offs for offs, _ in scen], M, SEED, OFFSET)
    _, want_c = _check(case, got, scen, M, SEED, OFFSET)
    c = want_c[1][:, who]
    assert (c == 0).any() and ((c > 0) & (c < L - p + 1)).any() and (c == L - p + 1).any()


# ---------------------------------------------------------------- limits
def test_sixty_four_scenarios_of_sixty_four_single_lap_offsets():
    case = RR.field_case(3)
    case['config'] = dict(case['config'], total_laps=70)
    scen = [([PR.laps((s + lap) % 3, lap, lap, 0.05 * ((s + lap) % 9 - 4)) for lap in range(1, 65)], {}) for s in range(64)]
    m = 2
    got = PH.paces(case, None, [offs for offs, _ in scen], m, SEED, 9)
    _check(case, got, scen, m, SEED, 9)


def test_a_thousand_laps():
    case = RR.field_case(2)
    case['config'] = dict(case['config'], total_laps=1000, dnf_rates={t: 0.0 for t in case['config']['dnf_rates']})
    case['driver_dnf_rates'] = {d: 0.0 for d in case['driver_dnf_rates']}       # both cars see the flag
    scen = [([], {}), ([PR.until_stop(0, 1, 0.4)], {0: (-1, 0, [])}),
            ([PR.until_stop(1, 1000, -0.3), PR.laps(0, 1, 1000, 0.25)], {}),
            ([PR.laps(1, 1, 500, 0.2), PR.laps(1, 501, 1000, -0.2), PR.until_stop(1, 2, 0.1)], {1: (-1, 0, [(1000, 1)])})]
    m = 2
    got = PH.paces(case, [pl for _, pl in scen], [offs for offs, _ in scen], m, SEED, 1)
    _, want_c = _check(case, got, scen, m, SEED, 1)
    assert (want_c[1][:, 0] == 1000).all() and got['carried'][1, 0, 1000] == m      # c = L lands in column L
    assert (want_c[2][:, 1] == 1).all() and (want_c[3][:, 1] == 999).all()


def test_a_race_of_one_lap():
    case = RR.field_case(3)
    case['config'] = dict(case['config'], total_laps=1)
    scen = [([], {}), ([PR.laps(0, 1, 1, 1.7)], {}), ([PR.until_stop(1, 1, -0.9), PR.laps(1, 1, 1, -0.8)], {})]
    got = PH.paces(case, None, [offs for offs, _ in scen], M, SEED, 5)
    want_o, want_c = _check(case, got, scen, M, SEED, 5)
    assert not np.array_equal(want_o[1], want_o[0]) and not np.array_equal(want_o[2], want_o[0])
    assert set(np.unique(want_c[2][:, 1])) <= {0, 1}


# ---------------------------------------------------------------- identities and the counting kernel
def test_scenarios_without_offsets_or_with_zero_offsets_are_the_strategy_kernel():
    case = _case('EVT')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    plans = [{}, {0: (-1, 0, [(8, 2)])}, {1: (-1, 0, [(15, 1), (L - 5, 0)]), 0: (-1, 0, [])}]
    zero = [[PR.laps(d, 1, L, 0.0) for d in range(n)], [PR.until_stop(0, 1, 0.0), PR.laps(0, 3, 9, 0.0)],
            [PR.until_stop(1, 2, 0.0), PR.until_stop(n - 1, L, 0.0)]]
    hist, orders = KH.generic_strategy(case, plans, M, SEED, OFFSET)
    for offs in ([[]] * 3, zero):
        got = PH.paces(case, plans, offs, M, SEED, OFFSET)
        assert np.array_equal(got['orders'], orders) and np.array_equal(got['hist'], hist)
    ref = _ref('EVT')
    k = L // 2
    state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFFSET + 3, k))
    plans = [{}, {0: (-1, 0, [(k + 1, 2)])}]
    hist, orders = KH.generic_strategy(case, plans, M, SEED, OFFSET, state=state)
    for offs in ([[]] * 2, [[PR.laps(d, k + 1, L, 0.0) for d in range(n)], [PR.until_stop(0, k + 1, 0.0)]]):
        got = PH.paces(case, plans, offs, M, SEED, OFFSET, state=state)
        assert np.array_equal(got['orders'], orders) and np.array_equal(got['hist'], hist)


@pytest.mark.parametrize('grid_x', [1, 3, 7])
def test_counting_kernel_does_not_depend_on_its_grid(grid_x):
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    scen = PR.scenarios(1, L, n)
    plans, offs = [pl for _, pl in scen], [o for o, _ in scen]
    m = 37                                                  # no multiple of any grid
    hist, stage, car, delta, carried = PH.paces_raw(case, plans, offs, m, SEED, 11, grid_x=grid_x)
    orders, laps = PH.decode(stage, car)
    want_d = SR.delta_counts(orders, n)
    want_d[:, :, n - 1] = 0                                 # the centre bin is the host's
    want_c = PR.carried_counts(laps, L)
    want_c[:, :, 0] = 0                                     # ... and so is column 0
    assert np.array_equal(delta, want_d) and np.array_equal(carried, want_c)
    assert np.array_equal(hist, PR.hist_counts(orders, n))
    assert carried[4].any() and carried[5].any()
    # without the counting kernel nothing is counted
    _, stage2, car2, d2, c2 = PH.paces_raw(case, plans, offs, m, SEED, 11, count=False)
    assert np.array_equal(stage2, stage) and np.array_equal(car2, car) and not d2.any() and not c2.any()


# ---------------------------------------------------------------- every input under generated offset sets
@functools.lru_cache(maxsize=None)
def _fuzz_inputs():
    return PC.fuzz_inputs()


def test_emulated_kernel_on_every_input_from_the_grid():
    def compare(case, seed, scen, want_o, want_c):
        got = PH.paces(case, [pl for _, pl in scen], [offs for offs, _ in scen], PC.FUZZ_SIMS, seed, PC.FUZZ_OFFSET)
        PC.check_against(got, case, want_o, want_c, PC.FUZZ_SIMS)
        assert np.array_equal(got['laps'], want_c)

    PC.fuzz_sweep(*_fuzz_inputs(), compare)


def test_emulated_kernel_on_every_input_from_a_state():
    def compare(case, seed, scen, want_o, want_c, state):
        got = PH.paces(case, [pl for _, pl in scen], [offs for offs, _ in scen], PC.FUZZ_SIMS, seed, 0, state=state)
        PC.check_against(got, case, want_o, want_c, PC.FUZZ_SIMS)
        assert np.array_equal(got['laps'], want_c)

    PC.state_sweep(*_fuzz_inputs(), compare)
