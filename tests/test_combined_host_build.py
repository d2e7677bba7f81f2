"""race_scenario_kernel<false / true, kRuleAll> and the three counting kernels it shares with its siblings, executed on the host
(tools/emu/emu_generic.cpp, through combined_host_build), against

  1. the Python restatement (combined_ref) on the scenarios where the rule sets meet (combined_ref.meeting_scenarios),
     from the grid and from a state, on S60, EVT and a 32-car field;
  2. the emulated single-kind kernels: with at most one table non-empty the combined kernel must stage what
     race_strategy_kernel, race_penalties_kernel, race_events_kernel and race_paces_kernel stage, simulation for
     simulation, and count what they count;
  3. the restatement again, under the generated scenarios of combined_cases on every input of generic_cases.py, from the
     grid and from a state (the sweeps of tests/test_gpu_combined_fuzz.py that need no device).

The three stagings stay inside their chunks (guard fill on both sides, checked by combined_host_build on every call), and
the counting kernels' bins are the counts of the staged data whatever their grid."""
import functools

import numpy as np
import pytest

import combined_cases as CC
import combined_host_build as CH
import combined_ref as CR
import events_host_build as EH
import events_ref as ER
import kernel_host_build as KH
import oracle_py as O
import paces_host_build as PH
import paces_ref as PR
import penalties_host_build as NH
import penalties_ref as NR
import resume_ref as RR
import strategy_ref as SR

CASES = ['S60', 'EVT', 'n32']
M, SEED, OFFSET = 40, 47, 300


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


_traced = {}


def _ref(name):
    if name not in _traced:
        _traced[name] = RR.traced_run(_case(name), M, SEED, OFFSET)
    return _traced[name]


def _start(name, start):
    """(state or None, first lap with a pit step, keyword arguments of combined_ref.ref_run)."""
    case, ref = _case(name), _ref(name)
    if start == 'grid':
        return None, 2, dict(grids=ref['grids'])
    k = case['config']['total_laps'] // 2
    state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFFSET + 3, k))
    return state, k + 1, dict(state=state)


def _leader(name):
    """The driver who wins most of the oracle's simulations of the case."""
    return int(np.bincount(_ref(name)['orders'][:, 0]).argmax())


@functools.lru_cache(maxsize=None)
def _fuzz_inputs():
    return CC.fuzz_inputs()


# ---------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize('start', ['grid', 'state'])
@pytest.mark.parametrize('name', CASES)
def test_emulated_kernel_equals_the_restatement_where_the_rules_meet(name, start):
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    state, first, kw = _start(name, start)
    scen = CR.meeting_scenarios(first, L, n, _leader(name))
    got = CH.combined(case, scen, M, SEED, OFFSET, state=state)
    want = CR.ref_run(case, scen, M, SEED, OFFSET, **kw)
    CH.check_against(got, case, want, M)
    want_o, want_f, want_e, want_c = want
    assert np.array_equal(got['fates'], want_f) and np.array_equal(got['seen'], want_e)
    assert np.array_equal(got['laps'], want_c)
    if start == 'grid':
        assert np.array_equal(want_o[0], _ref(name)['orders'])
    # the scenarios do what they are there for: each changes an order; a penalty is served at a stop and one is added at
    # the flag; the stop under the safety car clears the offset after two laps, the red flag's tyre change clears nothing
    for s in range(1, len(scen)):
        assert not np.array_equal(want_o[s], want_o[0]), s
    assert (want_f == CR.FATE_SERVED).any() and (want_f == CR.FATE_FLAG).any()
    assert set(np.unique(want_c[1][:, 0])) <= {0, 1, 2} and (want_c[1][:, 0] == 2).sum() > M // 2
    assert (want_f[1][:, 0] == CR.FATE_SERVED).sum() > M // 2 and not (want_f[2][:, 0] == CR.FATE_SERVED).any()
    k = min(max((first + L) // 2, first + 1), L)
    assert (want_c[2][:, 0] > 2).any() and (want_c[2][:, 0] <= L - k + 2).all()
    assert (want_e[1][:, 1] >= 1).all() and (want_e[2][:, 0] >= 1).all() and not want_e[4].any()


# ---------------------------------------------------------------- 2. the identities, against the emulated siblings
@pytest.mark.parametrize('start', ['grid', 'state'])
def test_with_one_table_the_kernel_is_that_table_s_own_kernel(start):
    name = 'EVT'
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    state, first, _ = _start(name, start)
    trivial = lambda a: (a[:, :, 0] == M).all() and not a[:, :, 1:].any()
    # no table at all: race_strategy_kernel, whether the count arrays are NULL or zero
    plans = [{}, {0: (-1, 0, [(first + 3, 2)])}, {1: (-1, 0, [(first + 1, 1), (L - 5, 0)]), 0: (-1, 0, [])}]
    hist, orders = KH.generic_strategy(case, plans, M, SEED, OFFSET, state=state)
    drawn = EH.events(case, plans, [[]] * 3, M, SEED, OFFSET, state=state)['events']
    for null in (False, True):
        got = CH.combined(case, [CR.scenario(p) for p in plans], M, SEED, OFFSET, state=state, null_counts=null)
        assert np.array_equal(got['orders'], orders) and np.array_equal(got['hist'], hist)
        assert np.array_equal(got['delta'], SR.delta_counts(orders, n))
        assert trivial(got['fate']) and trivial(got['carried']) and np.array_equal(got['events'], drawn)
    # penalties only
    scen = NR.scenarios(first, L, n)
    pens, plans = [p for p, _ in scen], [pl for _, pl in scen]
    want = NH.penalties(case, plans, pens, M, SEED, OFFSET, state=state)
    got = CH.combined(case, [CR.scenario(pl, penalties=p) for p, pl in scen], M, SEED, OFFSET, state=state, null_counts=True)
    for k in ('orders', 'hist', 'delta', 'fate', 'fates'):
        assert np.array_equal(got[k], want[k]), k
    assert trivial(got['carried'])
    assert np.array_equal(got['events'], EH.events(case, plans, [[]] * len(scen), M, SEED, OFFSET, state=state)['events'])
    # events only
    scen = ER.scenarios(first, L, n)
    evs, plans = [e for e, _ in scen], [pl for _, pl in scen]
    want = EH.events(case, plans, evs, M, SEED, OFFSET, state=state)
    got = CH.combined(case, [CR.scenario(pl, events=e) for e, pl in scen], M, SEED, OFFSET, state=state, null_counts=True)
    for k in ('orders', 'hist', 'delta', 'events', 'seen'):
        assert np.array_equal(got[k], want[k]), k
    assert trivial(got['fate']) and trivial(got['carried'])
    # offsets only
    scen = PR.scenarios(1 if start == 'grid' else first, L, n)
    offs, plans = [o for o, _ in scen], [pl for _, pl in scen]
    want = PH.paces(case, plans, offs, M, SEED, OFFSET, state=state)
    got = CH.combined(case, [CR.scenario(pl, paces=o) for o, pl in scen], M, SEED, OFFSET, state=state, null_counts=True)
    for k in ('orders', 'hist', 'delta', 'carried', 'laps'):
        assert np.array_equal(got[k], want[k]), k
    assert trivial(got['fate'])


def test_overrides_equal_to_what_a_simulation_drew_change_nothing_for_it():
    case = _case('EVT')
    L = case['config']['total_laps']
    base = CH.combined(case, [CR.scenario()], M, SEED, OFFSET)
    for i in (0, 7, M - 1):
        evs = [(lap, lap, ER.drawn_event(case, SEED, OFFSET + i, lap)[0]) for lap in range(2, L + 1)]
        got = CH.combined(case, [CR.scenario(events=evs)], 1, SEED, OFFSET + i)
        assert np.array_equal(got['orders'][0, 0], base['orders'][0, i]) and np.array_equal(got['seen'][0, 0], base['seen'][0, i])


# ---------------------------------------------------------------- the counting kernels
@pytest.mark.parametrize('grid_x', [1, 3, 7])
def test_counting_kernels_do_not_depend_on_their_grid(grid_x):
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    scen = CR.meeting_scenarios(2, L, n, _leader('S60'))
    m = 37                                                  # no multiple of any grid
    r = CH.combined_raw(case, scen, m, SEED, 11, grid_x=grid_x)
    orders, fates, seen, laps = CH.decode(r['stage'], r['evs'], r['car'])
    want_d = SR.delta_counts(orders, n)
    want_d[:, :, n - 1] = 0                                 # the centre bin is the host's
    want_f, want_c = NR.fate_counts(fates, n), PR.carried_counts(laps, L)
    want_f[:, :, 0] = 0                                     # ... and so are the columns 0
    want_c[:, :, 0] = 0
    assert np.array_equal(r['delta'], want_d) and np.array_equal(r['fate'], want_f)
    assert np.array_equal(r['events'], ER.event_counts(seen, L)) and np.array_equal(r['carried'], want_c)
    assert np.array_equal(r['hist'], NR.hist_counts(orders, n))
    assert r['fate'][1].any() and r['carried'][1].any() and r['fate'][5].any() and r['carried'][5].any()
    # without the counting kernels nothing is counted
    r2 = CH.combined_raw(case, scen, m, SEED, 11, count=False)
    assert np.array_equal(r2['stage'], r['stage']) and np.array_equal(r2['evs'], r['evs']) and np.array_equal(r2['car'], r['car'])
    assert not (r2['delta'].any() or r2['fate'].any() or r2['events'].any() or r2['carried'].any())


# ---------------------------------------------------------------- 3. every input under generated scenarios
@pytest.mark.parametrize('start', ['grid', 'state'])
def test_emulated_kernel_on_every_input(start):
    """The comparisons of tests/test_gpu_combined_fuzz.py parts a and b that need no device: combined_cases' scenarios on
    the 100 inputs of generic_cases.run_inputs() from the grid and on the 94 of resume_inputs() from the oracle's state of
    simulation 3 after max(1, L // 2), 8 simulations each.  The generator's conditions are asserted in the sweep."""
    def compare(case, seed, scen, want, m, offset, state):
        got = CH.combined(case, scen, m, seed, offset, state=state)
        CH.check_against(got, case, want, m)
        assert np.array_equal(got['fates'], want[1]) and np.array_equal(got['seen'], want[2])
        assert np.array_equal(got['laps'], want[3])

    CC.fuzz_sweep(*_fuzz_inputs(), compare, from_state=start == 'state')
