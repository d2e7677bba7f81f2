"""race_conditions_kernel<false> and <true> and conditions_count (csrc/conditions.hip.h) compiled for the host
(tools/emu/emu_generic.cpp) and compared, integers only, with a reference that does not share their code: the raw staged
order and mask of every simulation, decoded by the layout documented at the top of conditions.hip.h, bit for bit against
conditions_ref's numpy restatement of the nine facts over the CPU oracle's run; the histogram against the oracle's; the
counting kernel's counts against the restated ones.  Every compared condition is shown informative by the reference (met
by some, not by all simulations) except the deliberate always / never / empty ones.  The host build is test
infrastructure: nothing under monte_carlo_gp_amd/ can reach it and the product has no CPU path."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import conditions_host_build as CH
import conditions_ref as CR
import generic_cases as G
import oracle_py as O
import resume_ref as RR

RUN_SIMS = 64
CASES = ('S60', 'EVT', 'WET', 'HET', 'N10')
FIELD_SIZES = (1, 2, 3, 22, 32)


_conditions = CR.choose          # informative simple and eight-atom conditions, then the three constant ones


def _compare(name, got, facts, conds, hist):
    assert np.array_equal(got['orders'], facts['orders']), name
    want = CR.masks(facts, conds)
    bad = np.nonzero(got['masks'] != want)[0]
    assert bad.size == 0, f'{name}: {len(bad)} masks differ, first simulation {bad[:3].tolist()}: ' \
                          f'{[hex(int(got["masks"][i]) ^ int(want[i])) for i in bad[:3]]}'
    assert np.array_equal(got['hist'], hist), name
    ref = CR.counts(facts, conds)
    assert np.array_equal(got['count'], ref['count']), name
    if got['cond_hist'] is not None:
        assert np.array_equal(got['cond_hist'], ref['cond_hist']), name
        assert (got['cond_hist'].sum(axis=2) == got['count'][:, None]).all()      # every driver's row sums to the count


def _lap1_corner():
    """A fuzz configuration in which the oracle retires some, not all, cars on lap 1 within RUN_SIMS simulations."""
    for name, case in G.fuzz_cases().items():
        if name == 'X_all_out_lap1' or len(case['grid_probs']) < 4:
            continue
        f = CR.oracle_facts(case, RUN_SIMS, case['seed'], 3)
        lap1 = (f['out'] == 1).sum()
        if lap1 >= 8 and (f['out'] != 1).sum() >= 8:
            return name, case, case['seed']
    raise AssertionError('no fuzz configuration with lap-1 retirements')


def _grid_inputs():
    return [(name, O.load_case(name), 42) for name in CASES] + [_lap1_corner()] + \
        [(f'n{n}', RR.field_case(n), 5) for n in FIELD_SIZES]


def test_conditions_kernel_from_the_grid_equals_the_restated_masks():
    used, eight, total = set(), 0, 0
    for name, case, seed in _grid_inputs():
        n, L = len(case['grid_probs']), case['config']['total_laps']
        ref = RR.traced_run(case, RUN_SIMS, seed, 3)
        facts = CR.oracle_facts(case, RUN_SIMS, seed, 3, ref=ref)
        conds, constant = _conditions(facts, n, L, seed)
        CR.assert_informative(facts, conds, constant)
        got = CH.staged(case, conds, RUN_SIMS, seed, sim_offset=3)
        _compare(name, got, facts, conds, ref['hist'])
        k = constant[0]
        assert np.array_equal(got['cond_hist'][k], got['hist']) and np.array_equal(got['cond_hist'][k + 1], got['hist'])
        assert got['count'][k] == got['count'][k + 1] == RUN_SIMS and got['count'][k + 2] == 0
        assert not got['cond_hist'][k + 2].any()
        if name.startswith('F') or name.startswith('X'):
            assert (facts['out'] == 1).any()                            # the corner: lap-1 retirements
        used |= CR.facts_used(conds[:k])
        eight += sum(len(c) == 8 for c in conds[:k])
        total += k
        if n >= 3:
            assert k >= 20, (name, k)
    assert used == set(CR.FACT_NAMES)                                   # every fact compared somewhere, informatively
    assert eight >= 100 and total >= 300


def _grid_facts(args, ref):
    name, case, seed = args
    facts = CR.oracle_facts(case, RUN_SIMS, seed, 3, ref=ref)
    return ref, facts, _conditions(facts, len(case['grid_probs']), case['config']['total_laps'], seed)


def _pool():
    return ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1))


def test_conditions_kernel_from_the_grid_on_every_input():
    """All of generic_cases.run_inputs(): the 84 fuzz configurations with their corner cases (wet and damp tracks, two-
    and three-car fields, every car out on lap 1, no noise, every overtake attempted), lap times near zero and the field
    sizes, each with the conditions its own reference run shows informative."""
    inputs = G.run_inputs()
    O.lib()
    with _pool() as pool:                                       # the oracle's runs; the rest is Python and gains nothing
        refs = list(pool.map(lambda a: RR.traced_run(a[1], RUN_SIMS, a[2], 3), inputs))
    prepared = [_grid_facts(a, ref) for a, ref in zip(inputs, refs)]
    used, eight, total, done = set(), 0, 0, 0
    for (name, case, seed), (ref, facts, (conds, constant)) in zip(inputs, prepared):
        n = len(case['grid_probs'])
        CR.assert_informative(facts, conds, constant)
        k = constant[0]
        if n >= 3:
            assert k >= 20, (name, k)
        _compare(name, CH.staged(case, conds, RUN_SIMS, seed, sim_offset=3), facts, conds, ref['hist'])
        used |= CR.facts_used(conds[:k])
        eight += sum(len(c) == 8 for c in conds[:k])
        total += k
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and len(inputs) == 100
    assert used == set(CR.FACT_NAMES)
    assert total >= 5000 and eight >= 2500, (total, eight)


def _state_facts(args, ref, m=4, base=40):
    name, case, seed = args
    runs = CR.state_runs(case, seed, ref, range(m), base)
    parts = [CR.oracle_facts(case, 0, seed, base, ref=ref, sims=[i], lap0=k) for i, k, _ in runs]
    conds, constant = _conditions(CR.concat(parts), len(case['grid_probs']), case['config']['total_laps'], seed + 1)
    return runs, parts, conds, constant


def test_conditions_kernel_from_a_state_on_every_input():
    """All of generic_cases.resume_inputs(): four simulations' states after every lap of resume_laps, each resumed as
    itself, with the conditions informative over those states' facts."""
    inputs = G.resume_inputs()
    O.lib()
    with _pool() as pool:
        refs = list(pool.map(lambda a: RR.traced_run(a[1], 4, a[2], 40), inputs))
    prepared = [_state_facts(a, ref) for a, ref in zip(inputs, refs)]
    done = states = compared = 0
    for (name, case, seed), (runs, parts, conds, constant) in zip(inputs, prepared):
        facts = CR.concat(parts)
        CR.assert_informative(facts, conds, constant)
        want = CR.counts_each(facts, conds)
        prob, table = CH.KH.generic_problem(case), CR.c_conditions(conds)
        for s_, (i, k, st) in enumerate(runs):
            got = CH.staged(case, conds, 1, seed, sim_offset=40 + i, state=st, prob=prob, table=table)
            assert np.array_equal(got['orders'][0], facts['orders'][s_]), (name, i, k)
            assert int(got['masks'][0]) == int(want['masks'][s_]), (name, i, k, hex(int(got['masks'][0]) ^ int(want['masks'][s_])))
            for key in ('hist', 'count', 'cond_hist'):
                assert np.array_equal(got[key], want[key][s_]), (name, i, k, key)
        assert len(runs) >= 4, name
        states += len(runs)
        compared += constant[0]
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ
    assert states >= 94 * 4 * 3 and compared >= 94 * 10, (states, compared)


def test_sixty_four_conditions_of_eight_atoms():
    case, seed, m = O.load_case('EVT'), 42, 96
    n, L = len(case['grid_probs']), case['config']['total_laps']
    ref = RR.traced_run(case, m, seed)
    facts = CR.oracle_facts(case, m, seed, ref=ref)
    conds = CR.pick(facts, CR.wide_candidates(n, L, np.random.default_rng(7), 4000), 64)
    assert len(conds) == 64 and all(len(c) == 8 for c in conds)
    CR.assert_informative(facts, conds)
    assert len(np.unique(CR.masks(facts, conds))) > m // 2              # the masks tell the simulations apart
    for grid_x in (1, 5):
        _compare('EVT64', CH.staged(case, conds, m, seed, grid_x=grid_x), facts, conds, ref['hist'])
    only = CH.staged(case, conds, m, seed, cond_hist=False)             # counts without the histograms
    assert only['cond_hist'] is None and np.array_equal(only['count'], CR.counts(facts, conds)['count'])
    assert (CR.masks(facts, conds) >> np.uint64(63)).any()              # bit 63 is in use


def _resume_runs(case, seed, sims, base):
    """[(i, k, state)] of traced simulations `sims` after every lap of G.resume_laps, and the reference."""
    ref = RR.traced_run(case, max(sims) + 1, seed, base)
    runs = []
    for i in sims:
        for k in G.resume_laps(case, seed, base + i):
            runs.append((i, k, (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k))))
    return ref, runs


_concat = CR.concat


@pytest.mark.parametrize('name', CASES + ('corner', 'n1', 'n2', 'n3', 'n22', 'n32'))
def test_conditions_kernel_from_a_state_continues_the_oracle_race(name):
    """Simulation i's state after lap k, resumed as simulation i, gives simulation i's facts, events counted from lap
    k + 1; a car already out keeps the state's retirement lap (lap 1 included)."""
    if name == 'corner':
        _, case, seed = _lap1_corner()
    elif name in CASES:
        case, seed = O.load_case(name), 42
    else:
        case, seed = RR.field_case(int(name[1:])), 5
    n, L = len(case['grid_probs']), case['config']['total_laps']
    base = 40
    ref, runs = _resume_runs(case, seed, range(8), base)
    parts = [CR.oracle_facts(case, 0, seed, base, ref=ref, sims=[i], lap0=k) for i, k, _ in runs]
    facts = _concat(parts)
    conds, constant = _conditions(facts, n, L, seed + 1)
    CR.assert_informative(facts, conds, constant)
    prob = CH.KH.generic_problem(case)
    already_out = 0
    for (i, k, st), f in zip(runs, parts):
        got = CH.staged(case, conds, 1, seed, sim_offset=base + i, state=st, prob=prob)
        _compare((name, i, k), got, f, conds, RR.counts(ref['orders'][i:i + 1], n))
        already_out += int((st[0]['retired_lap'] != 0).sum())
    if name in ('S60', 'corner'):
        assert already_out > 0
    # the events before a state's lap are not part of it: some simulation's count differs between two of its states
    if name == 'EVT':
        ev = {}
        for (i, k, _), f in zip(runs, parts):
            ev.setdefault(i, set()).add(tuple(f['events'][0]))
        assert any(len(v) > 1 for v in ev.values())
