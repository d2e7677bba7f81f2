"""race_scenario_kernel<false / true, kRuleWeather> and weather_count executed on the host (tools/emu/emu_generic.cpp,
through weather_host_build) against the Python restatement (weather_ref) on the calls of weather_limit_cases: tables with
one non-zero cell, a checkerboard and the extremes; 64 scenarios of 64 changes; 1000 laps; one lap; every car out on lap 1
on the wrong tyres; states after laps 1, L - 1 and L; F33 under 64 scenarios, where the closed form the device's
counting-loop test relies on (weather_limit_cases.trace_wrong_laps) is first checked against the restatement; and the
scenarios of the call past its staging budget, with and without the u16 staging.  What the limits are there for is asserted
from the restatement alone before the emulator runs.  tests/test_gpu_weather_grids_fuzz.py runs the same cases on the
device."""
import numpy as np
import pytest

import kernel_host_build as KH
import resume_ref as RR
import weather_cases as WC
import weather_host_build as WH
import weather_limit_cases as WL
import weather_ref as WR

SIMS, OFFSET = WL.FUZZ_SIMS, WL.FUZZ_OFFSET


def _emulated(case, table, scen, m, seed, offset, want_o, want_w, **kw):
    got = WH.weather(case, [pl for _, pl in scen], [ch for ch, _ in scen], table, m, seed, offset, **kw)
    WC.check_against(got, case, want_o, want_w, m)
    assert np.array_equal(got['laps'], want_w)
    return got


@pytest.mark.parametrize('part', range(WL.TABLE_PARTS))
def test_tables_with_one_cell_a_checkerboard_and_the_extremes(part):
    for name, case, seed, calls in WL.table_wanted(part)[0]:
        prob = KH.generic_problem(case)
        for table, scen, want_o, want_w in calls:
            _emulated(case, table, scen, SIMS, seed, OFFSET, want_o, want_w, prob=prob)


def test_the_limits_do_not_pass_empty():
    """Inputs on which a one-cell table moved an order, and cells of the limit calls in column L: the restatement's own
    counts, against floors about a tenth below what it gave when the cases were written."""
    assert WL.tables_moved() == WL.TABLES_MEASURED >= WL.TABLES_FLOOR
    assert WL.column_l_cells() == WL.COLUMN_L_MEASURED >= WL.COLUMN_L_FLOOR


@pytest.mark.parametrize('k', range(len(WL.LIMITS)))
def test_limits(k):
    label, case, seed, table, scen, m, offset, want_o, want_w = WL.limit_wanted(k)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    # what the call is there for, from the restatement alone
    if label == 'a thousand laps':
        assert (want_w[1][:, 0] == L).all() and (want_w[2][:, 0] == L - WL.MAX_CHANGES).all()      # column 1000, all 8
        assert (want_w[2][:, 1] > 0).all() and not want_w[0].any()
    elif label.startswith('one lap'):
        assert set(np.unique(want_w[1])) <= {0, 1} and (want_w[1] == 1).sum() >= m * n * 3 // 4 and not want_w[0].any()
    elif label == 'all out on lap 1':
        assert not want_w.any()
    elif label.startswith('the wrong class'):
        assert (want_w[1] == L).sum() >= m * n // 2 and not want_w[2].any()       # (a rule car starts on wet tyres here)
    else:
        assert all(not np.array_equal(want_o[s], want_o[0]) for s in range(1, WL.MAX_SCENARIOS, 2))
        assert (want_w.max(axis=(1, 2)) > 0).all()
    got = _emulated(case, table, scen, m, seed, offset, want_o, want_w)
    assert (got['wrong_laps'].sum(axis=2) == m).all()
    if label == 'a thousand laps':
        assert got['wrong_laps'][1, 0, L] == m


@pytest.mark.parametrize('part', range(WL.STATE_PARTS))
def test_states_after_the_first_and_the_last_laps(part):
    states = WL.state_wanted(part)
    assert len(states) >= 8
    for name, case, seed, k, state, calls in states:
        prob = KH.generic_problem(case)
        for table, scen, want_o, want_w in calls:
            _emulated(case, table, scen, SIMS, seed, 0, want_o, want_w, state=state, prob=prob)


def test_f33_under_64_scenarios_and_the_closed_form():
    """The call of the device's counting-loop test at its first 8 simulations: the closed form of the planned scenarios is
    the restatement's count, and the emulated kernel is the restatement."""
    case, seed = WL.f33()
    L = case['config']['total_laps']
    scen = WL.f33_scenarios()
    ref = RR.traced_run(case, SIMS, seed, OFFSET)
    want_o, want_w = WL.restate(case, seed, WL.FULL, scen, SIMS, OFFSET, grids=ref['grids'])
    closed = WL.trace_wrong_laps(ref, scen[::2], WR.DRY, L)
    assert np.array_equal(closed, want_w[::2])
    assert len(set(np.unique(closed)) - {0}) >= 5 and want_w[1::2].any()
    _emulated(case, WL.FULL, scen, SIMS, seed, OFFSET, want_o, want_w)


def test_the_scenarios_of_the_call_past_its_budget_with_and_without_the_wrong_lap_staging():
    case, seed, table, scen = WL.budget_call()
    L = case['config']['total_laps']
    want_o, want_w = WL.restate(case, seed, table, scen, SIMS, OFFSET)
    assert (want_w == L).any() and len(set(np.unique(want_w))) == L + 1
    plans, changes = [pl for _, pl in scen], [ch for ch, _ in scen]
    hist, stage, car, wrong = WH.weather_raw(case, plans, changes, table, SIMS, seed, OFFSET)
    assert np.array_equal(WH.decode(stage), want_o) and np.array_equal(car, want_w)
    want = WR.wrong_counts(want_w, L)
    want[:, :, 0] = 0                                       # column 0 is the host's
    assert np.array_equal(wrong, want)
    hist2, stage2, car2, wrong2 = WH.weather_raw(case, plans, changes, table, SIMS, seed, OFFSET, stage_wrong=False)
    assert car2 is None and not wrong2.any() and np.array_equal(hist2, hist) and np.array_equal(stage2, stage)
