"""race_penalties_kernel<false / true> and penalties_count executed on the host (tools/emu/emu_generic.cpp, through
penalties_host_build) against the Python restatement (penalties_ref): order for order and fate for fate, from the grid and
from states after laps 1, L // 2 and L - 1, under the scenarios of penalties_ref.scenarios; the staged bytes stay inside
the chunk; the counting kernel's bins are the counts of the staged orders and fates whatever its grid."""
import numpy as np
import pytest

import oracle_py as O
import penalties_host_build as PH
import penalties_ref as PR
import resume_ref as RR
import strategy_ref as SR
import kernel_host_build as KH

CASES = ['S60', 'EVT', 'n32']
M, SEED, OFFSET = 64, 29, 300


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


_traced = {}


def _ref(name):
    """The oracle's traced run of the case, computed once and shared."""
    if name not in _traced:
        _traced[name] = RR.traced_run(_case(name), M, SEED, OFFSET)
    return _traced[name]


@pytest.mark.parametrize('start', ['grid', 'lap 1', 'lap L // 2', 'lap L - 1'])
@pytest.mark.parametrize('name', CASES)
def test_emulated_kernel_equals_the_restatement(name, start):
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    ref = _ref(name)
    if start == 'grid':
        state, first, kw = None, 2, dict(grids=ref['grids'])
    else:
        k = {'lap 1': 1, 'lap L // 2': L // 2, 'lap L - 1': L - 1}[start]
        state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFFSET + 3, k))
        first, kw = k + 1, dict(state=state)
    scen = PR.scenarios(first, L, n)
    pens, plans = [p for p, _ in scen], [pl for _, pl in scen]
    got = PH.penalties(case, plans, pens, M, SEED, OFFSET, state=state)
    want_o, want_f = [], []
    for s, (p, pl) in enumerate(scen):
        o, f = PR.orders(case, M, SEED, OFFSET, plans=pl, penalties=p, **kw)
        bad = [i for i in range(M) if not np.array_equal(got['orders'][s, i], o[i])]
        assert not bad, f'scenario {s}: {len(bad)} of {M} orders differ, first sim {bad[0]}'
        assert np.array_equal(got['fates'][s], f), f'scenario {s}: fates differ'
        want_o.append(o)
        want_f.append(f)
    want_o, want_f = np.stack(want_o), np.stack(want_f)
    if start == 'grid':
        assert np.array_equal(want_o[0], ref['orders'])
    assert np.array_equal(got['hist'], PR.hist_counts(want_o, n))
    assert np.array_equal(got['delta'], SR.delta_counts(want_o, n))
    assert np.array_equal(got['fate'], PR.fate_counts(want_f, n))
    assert (got['fate'].sum(axis=2) == M).all()
    if start == 'grid':
        # the scenarios do what they are there for: a penalty served in the pits on lap L, one added at the flag
        assert (want_f[5][:, 0] != PR.FATE_FLAG).all() and (want_f[5][:, 0] == PR.FATE_SERVED).any()
        assert (want_f[3][:, 1 % n] != PR.FATE_SERVED).all()       # the rule never stops on lap L
        assert (want_f[2][:, 1 % n] == PR.FATE_SERVED).any()
        assert not np.array_equal(want_o[1], want_o[0]) and not np.array_equal(want_o[4], want_o[0])


def test_no_penalty_scenarios_are_the_strategy_kernel():
    case = _case('EVT')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    plans = [{}, {0: (-1, 0, [(8, 2)])}, {1: (-1, 0, [(15, 1), (L - 5, 0)]), 0: (-1, 0, [])}]
    hist, orders = KH.generic_strategy(case, plans, M, SEED, OFFSET)
    got = PH.penalties(case, plans, [[]] * 3, M, SEED, OFFSET)
    assert np.array_equal(got['orders'], orders) and np.array_equal(got['hist'], hist)
    assert (got['fates'] == 0).all() and (got['fate'][:, :, 0] == M).all()


@pytest.mark.parametrize('grid_x', [1, 2, 7, 64, 100])
def test_counting_kernel_does_not_depend_on_its_grid(grid_x):
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    scen = PR.scenarios(2, L, n)
    pens, plans = [p for p, _ in scen], [pl for _, pl in scen]
    m = 37                                                  # no multiple of any grid
    hist, stage, delta, fate = PH.penalties_raw(case, plans, pens, m, SEED, 11, grid_x=grid_x)
    orders, fates = PH.decode(stage)
    want_d, want_f = SR.delta_counts(orders, n), PR.fate_counts(fates, n)
    want_d[:, :, n - 1] = 0                                 # the centre bin and column 0 are the host's
    want_f[:, :, 0] = 0
    assert np.array_equal(delta, want_d) and np.array_equal(fate, want_f)
    assert np.array_equal(hist, PR.hist_counts(orders, n))
    # without the counting kernel nothing is counted, and either output may be left out
    _, stage2, d2, f2 = PH.penalties_raw(case, plans, pens, m, SEED, 11, count=False)
    assert np.array_equal(stage2, stage) and not d2.any() and not f2.any()
