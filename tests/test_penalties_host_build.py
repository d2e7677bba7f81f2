"""race_scenario_kernel<false / true, kRulePenalties> and penalties_count executed on the host (tools/emu/emu_generic.cpp, through
penalties_host_build) against the Python restatement (penalties_ref): order for order and fate for fate, from the grid and
from states after laps 1, L // 2 and L - 1, under the scenarios of penalties_ref.scenarios; the staged bytes stay inside
the chunk; the counting kernel's bins are the counts of the staged orders and fates whatever its grid.

Second pass, the comparisons of tests/test_gpu_penalties_fuzz.py that need no device, so that a failure there splits at
once into "kernel text" and "device build or host side": the generator's scenarios (penalties_cases.scenarios) from the
grid on the 100 inputs of generic_cases.run_inputs() at 8 simulations, and the ties at the flag by construction."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import generic_cases as G
import oracle_py as O
import penalties_cases as PC
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


# ---------------------------------------------------------------- second pass: every input, ties at the flag
FUZZ_SIMS, FUZZ_OFFSET, TIE_SIMS = 8, 3, 64


def test_emulated_kernel_on_every_input_from_the_grid():
    """Orders and fates are the restatement's (itself checked against both trace references on every input), hist, delta
    and fate their counts.  At 8 simulations the restatement shows 8 inputs on which nothing bites (NO_BITE),
    served on 89 inputs, at the flag on 94, retired on 96, a penalty served at a planned stop on its pending lap on 87
    and missed by a stop one lap early on 83."""
    inputs = G.run_inputs()
    O.lib()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        refs = list(pool.map(lambda a: RR.traced_run(a[1], FUZZ_SIMS, a[2], FUZZ_OFFSET), inputs))
    done, quiet, seen, on_lap, early = 0, set(), {f: 0 for f in (1, 2, 3)}, 0, 0
    for (name, case, seed), ref in zip(inputs, refs):
        n = len(case['grid_probs'])
        e = PC.grid_expectation(name, case, seed, ref, FUZZ_SIMS, FUZZ_OFFSET)
        if not e['bites']:
            quiet.add(name)
        for f in e['fates_seen']:
            seen[f] += 1
        on_lap, early = on_lap + e['on_lap'], early + e['early']
        got = PH.penalties(case, [pl for _, pl in e['scen']], [p for p, _ in e['scen']], FUZZ_SIMS, seed, FUZZ_OFFSET)
        bad = np.argwhere((got['orders'] != e['orders']).any(axis=2))
        assert bad.size == 0, f'{name}: {len(bad)} orders differ, first (scenario, simulation) {bad[0]}'
        assert np.array_equal(got['fates'], e['fates']), name
        assert np.array_equal(got['hist'], PR.hist_counts(e['orders'], n)), name
        assert np.array_equal(got['delta'], SR.delta_counts(e['orders'], n)), name
        assert np.array_equal(got['fate'], PR.fate_counts(e['fates'], n)), name
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and len(inputs) == 100
    assert len(PC.NO_BITE) <= 12 and quiet <= set(PC.NO_BITE), sorted(quiet)
    assert min(seen.values()) >= 70 and on_lap >= 70 and early >= 70, (seen, on_lap, early)


@pytest.mark.parametrize('name, flips, keeps', [('S60', 20, 20), ('X_no_noise', 20, 20)])
def test_emulated_ties_at_the_flag(name, flips, keeps):
    """An AT_FLAG penalty of exactly t_b - t_a on the winner a (penalties_cases.flag_tie): the kernel's second
    sort_by_time orders the tied pair by grid slot, as the restatement and the re-sorted oracle order do."""
    case = O.load_case(name) if name in G.GOLDEN else G.fuzz_cases()[name]
    seed = 42 if name in G.GOLDEN else case['seed']
    ties, n_flips, n_keeps = PC.flag_ties(case, seed, TIE_SIMS, FUZZ_OFFSET)
    assert len(ties) >= 60 and n_flips >= flips and n_keeps >= keeps, (len(ties), n_flips, n_keeps)
    prob = KH.generic_problem(case)
    for i, pens, want in ties:
        got = PH.penalties(case, [{}], [pens], 1, seed, FUZZ_OFFSET + i, prob=prob)
        assert np.array_equal(got['orders'][0, 0], want), (name, i)
