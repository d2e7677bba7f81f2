"""race_scenario_kernel<false / true, kRuleWeather> and weather_count executed on the host (tools/emu/emu_generic.cpp,
through weather_host_build) against the Python restatement (weather_ref), in this order: the restatement without changes
is strategy_ref; the kernel equals the restatement under the generated scenario sets (weather_cases) from the grid on the
100 inputs of generic_cases.run_inputs() and from states after L // 2 on the 94 of resume_inputs(), at 8 simulations; the
staged data stay inside the chunk (guard bytes on both sides, checked by weather_host_build on every call) and a staging
that is not wanted is not written; the counting kernel's bins are the counts of the staged data whatever its grid."""
import numpy as np
import pytest

import kernel_host_build as KH
import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
import weather_cases as WC
import weather_host_build as WH
import weather_ref as WR

M, SEED, OFFSET = 24, 47, 300


def test_the_restatement_without_changes_is_strategy_ref():
    case = O.load_case('EVT')
    L = case['config']['total_laps']
    ref = RR.traced_run(case, M, SEED, OFFSET)
    for plans in ({}, {0: (-1, 0, [(8, 2)]), 1: (2, 3, [(L // 2, 1), (L - 1, 0)])}):
        for changes in ([], [(2, L, WR.DRY)]):
            got, wrong = WR.orders(case, M, SEED, OFFSET, plans=plans, changes=changes, grids=ref['grids'])
            assert np.array_equal(got, SR.orders(case, M, SEED, OFFSET, plans=plans, grids=ref['grids']))
            assert not wrong.any()
    assert np.array_equal(WR.orders(case, M, SEED, OFFSET, grids=ref['grids'])[0], ref['orders'])
    # ... and rain does change the race
    rain, wrong = WR.orders(case, M, SEED, OFFSET, changes=[(L // 2, L, WR.DAMP)], grids=ref['grids'])
    assert not np.array_equal(rain, ref['orders']) and wrong.any()


@pytest.mark.parametrize('part', range(WC.GRID_PARTS))
def test_emulated_kernel_on_every_input_from_the_grid(part):
    for name, case, seed, calls in WC.grid_wanted(part)[0]:
        prob = KH.generic_problem(case)
        for table, scen, want_o, want_w in calls:
            got = WH.weather(case, [pl for _, pl in scen], [ch for ch, _ in scen], table, WC.FUZZ_SIMS, seed,
                             WC.FUZZ_OFFSET, prob=prob)
            WC.check_against(got, case, want_o, want_w, WC.FUZZ_SIMS)
            assert np.array_equal(got['laps'], want_w), name


@pytest.mark.parametrize('part', range(WC.STATE_PARTS))
def test_emulated_kernel_on_every_input_from_a_state(part):
    for name, case, seed, state, calls in WC.state_wanted(part)[0]:
        prob = KH.generic_problem(case)
        for table, scen, want_o, want_w in calls:
            got = WH.weather(case, [pl for _, pl in scen], [ch for ch, _ in scen], table, WC.FUZZ_SIMS, seed, 0,
                             state=state, prob=prob)
            WC.check_against(got, case, want_o, want_w, WC.FUZZ_SIMS)
            assert np.array_equal(got['laps'], want_w), name


def test_the_sweeps_do_not_pass_empty():
    """Inputs on which a rule car crossed over, a red flag fell on a changed lap, an order moved: the restatement's own
    counts, against floors a little below what it gave when the cases were written (weather_cases.GRID_MEASURED)."""
    assert WC.grid_marks() == WC.GRID_MEASURED and WC.state_marks() == WC.STATE_MEASURED
    WC.check_floors(WC.grid_marks(), WC.GRID_FLOORS)
    WC.check_floors(WC.state_marks(), WC.STATE_FLOORS)


def test_a_staging_that_is_not_wanted_is_not_written():
    case = O.load_case('S60')
    L = case['config']['total_laps']
    changes = [[], [(L // 2, L, WR.DAMP)]]
    hist, stage, car, wrong = WH.weather_raw(case, None, changes, WC.FULL_TABLE, 9, SEED, 5)
    hist2, stage2, car2, wrong2 = WH.weather_raw(case, None, changes, WC.FULL_TABLE, 9, SEED, 5, stage_wrong=False)
    assert car2 is None and not wrong2.any()
    assert np.array_equal(hist2, hist) and np.array_equal(stage2, stage)
    assert car[1].any() and not car[0].any()


@pytest.mark.parametrize('grid_x', [1, 3, 7])
def test_counting_kernel_does_not_depend_on_its_grid(grid_x):
    case = O.load_case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    plans = [{}, {}, {0: (WR.INTER, 0, []), n - 1: (-1, 0, [])}]
    changes = [[], [(L // 2, L, WR.DAMP)], [(L - 5, L, WR.WET_TRACK)]]
    m = 37                                                  # no multiple of any grid
    hist, stage, car, wrong = WH.weather_raw(case, plans, changes, None, m, SEED, 11, grid_x=grid_x)
    want = WR.wrong_counts(car.astype(np.int64), L)
    want[:, :, 0] = 0                                       # column 0 is the host's
    assert np.array_equal(wrong, want) and np.array_equal(hist, WR.hist_counts(WH.decode(stage), n))
    assert wrong[1].any() and wrong[2].any() and not wrong[0].any()
    assert (car[2][:, 0] >= 1).sum() > m // 2               # driver 0 starts on intermediates on a dry track: lap 1 counts
    # without the counting kernel nothing is counted
    _, stage2, car2, w2 = WH.weather_raw(case, plans, changes, None, m, SEED, 11, count=False)
    assert np.array_equal(stage2, stage) and np.array_equal(car2, car) and not w2.any()
