"""race_scenario_kernel<false, kRuleGrid> and grid_count executed on the host (tools/emu/emu_generic.cpp, through
grids_host_build) against the Python restatement (grids_ref), in this order: the restatement without edits is
strategy_ref; the kernel equals the restatement under the generated scenario sets (grids_cases) on the 100 inputs of
generic_cases.run_inputs() at 8 simulations; the staged data stay inside the chunk (guard bytes on both sides, checked by
grids_host_build on every call) and a staging that is not wanted is not written; the counting kernel's bins are the
counts of the staged data whatever its grid."""
import numpy as np
import pytest

import grids_cases as GC
import grids_host_build as GH
import grids_ref as GR
import kernel_host_build as KH
import oracle_py as O
import resume_ref as RR
import strategy_ref as SR

M, SEED, OFFSET = 24, 47, 300


def test_the_restatement_without_edits_is_strategy_ref():
    case = O.load_case('EVT')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    ref = RR.traced_run(case, M, SEED, OFFSET)
    for plans in ({}, {0: (-1, 0, [(8, 2)]), 1: (2, 3, [(L // 2, 1), (L - 1, 0)])}):
        got, slots = GR.orders(case, M, SEED, OFFSET, plans=plans, grids=ref['grids'])
        assert np.array_equal(got, SR.orders(case, M, SEED, OFFSET, plans=plans, grids=ref['grids']))
        assert np.array_equal(np.argsort(slots, axis=1), ref['grids'])
    assert np.array_equal(GR.orders(case, M, SEED, OFFSET, grids=ref['grids'])[0], ref['orders'])
    # ... pinning every driver where it was drawn changes nothing, and a pit-lane start does change the race
    for i in range(3):
        pins = {int(d): (GR.PIN, slot + 1, 0.0) for slot, d in enumerate(ref['grids'][i])}
        same, _ = GR.orders(case, 1, SEED, OFFSET + i, edits=pins, grids=ref['grids'][i:i + 1])
        assert np.array_equal(same[0], ref['orders'][i])
    lane, slots = GR.orders(case, M, SEED, OFFSET, edits={0: (GR.PIT_LANE, 0, 2.5)}, grids=ref['grids'])
    assert not np.array_equal(lane, ref['orders']) and (slots[:, 0] == n - 1).all()


def test_the_assignment_by_hand():
    """edited_grid on a grid of six, every rule of the header once."""
    grid = [3, 1, 4, 0, 5, 2]                               # driver on slot 0, 1, ...
    E = GR.edited_grid
    assert E(grid, {}) == grid
    assert E(grid, {3: (GR.DROP, 1, 0.0)}) == grid          # (1, 0) stays in front of (1, 1)
    assert E(grid, {3: (GR.DROP, 2, 0.0)}) == [1, 3, 4, 0, 5, 2]
    assert E(grid, {3: (GR.DROP, 5, 0.0)}) == [1, 4, 0, 5, 3, 2]        # exactly n - 1: in front of the car drawn last
    assert E(grid, {3: (GR.DROP, 255, 0.0)}) == [1, 4, 0, 5, 2, 3]
    assert E(grid, {3: (GR.DROP, 2, 0.0), 1: (GR.DROP, 1, 0.0)}) == [3, 1, 4, 0, 5, 2]     # keys 2, 2 and the third car's 2
    assert E(grid, {2: (GR.PIN, 1, 0.0)}) == [2, 3, 1, 4, 0, 5]
    assert E(grid, {3: (GR.PIN, 6, 0.0)}) == [1, 4, 0, 5, 2, 3]
    assert E(grid, {4: (GR.PIT_LANE, 0, 1.0), 3: (GR.PIT_LANE, 0, 0.0)}) == [1, 0, 5, 2, 3, 4]  # by drawn slot
    assert E(grid, {4: (GR.PIT_LANE, 0, 1.0), 3: (GR.PIN, 5, 0.0), 1: (GR.DROP, 9, 0.0)}) == [0, 5, 2, 1, 3, 4]


@pytest.mark.parametrize('part', range(GC.PARTS))
def test_emulated_kernel_on_every_input(part):
    for name, case, seed, scen, at, want_o, want_s in GC.wanted(part)[0]:
        got = GH.grids(case, [pl for _, pl in scen], [ed for ed, _ in scen], GC.FUZZ_SIMS, seed, GC.FUZZ_OFFSET,
                       prob=KH.generic_problem(case))
        GC.check_against(got, case, want_o, want_s, GC.FUZZ_SIMS)
        assert np.array_equal(got['slots'], want_s), name


def test_the_sweep_does_not_pass_empty():
    """Inputs on which an edit changed a start compound, an order moved, a pit-lane car beat a grid starter: the
    restatement's own counts, against floors a little below what it gave when the cases were written."""
    assert GC.marks() == GC.MEASURED
    GC.check_floors(GC.marks(), GC.FLOORS)


def test_a_staging_that_is_not_wanted_is_not_written():
    case = O.load_case('S60')
    n = len(case['grid_probs'])
    edits = [{}, {0: (GR.PIT_LANE, 0, 2.5), 1: (GR.DROP, 10, 0.0)}]
    hist, stage, car, start, gain = GH.grids_raw(case, None, edits, 9, SEED, 5)
    hist2, stage2, car2, start2, gain2 = GH.grids_raw(case, None, edits, 9, SEED, 5, stage_start=False)
    assert car2 is None and not start2.any() and not gain2.any()
    assert np.array_equal(hist2, hist) and np.array_equal(stage2, stage)
    assert (car[1][:, 0] == n - 1).all() and not np.array_equal(car[1], car[0])


@pytest.mark.parametrize('grid_x', [1, 3, 7])
def test_counting_kernel_does_not_depend_on_its_grid(grid_x):
    case = O.load_case('S60')
    n = len(case['grid_probs'])
    edits = [{}, {2: (GR.DROP, 10, 0.0)}, {0: (GR.PIT_LANE, 0, 2.5), n - 1: (GR.PIN, 1, 0.0)}]
    m = 37                                                  # no multiple of any grid
    hist, stage, car, start, gain = GH.grids_raw(case, None, edits, m, SEED, 11, grid_x=grid_x)
    slots, orders = car.astype(np.int64), GH.decode(stage)
    assert np.array_equal(start, GR.start_counts(slots, n)) and np.array_equal(gain, GR.gain_counts(slots, orders, n))
    assert np.array_equal(hist, GR.hist_counts(orders, n))
    assert (start.sum(axis=2) == m).all() and (start.sum(axis=1) == m).all() and (gain.sum(axis=2) == m).all()
    assert start[2, 0, n - 1] == m and start[2, n - 1, 0] == m
    # without the counting kernel nothing is counted
    _, stage2, car2, s2, g2 = GH.grids_raw(case, None, edits, m, SEED, 11, count=False)
    assert np.array_equal(stage2, stage) and np.array_equal(car2, car) and not s2.any() and not g2.any()
