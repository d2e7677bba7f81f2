"""race_scenario_kernel<false, kRuleGrid> and grid_count executed on the host (tools/emu/emu_generic.cpp, through
grids_host_build) against the Python restatement (grids_ref) under the random mixtures and whole-field edit sets of
grids_limit_cases: on the 100 inputs of generic_cases.run_inputs() at 8 simulations; on F33 under 64 scenarios, where the
expected start slots of the device's counting-loop test (edited_grid on the oracle's grids, no race run) are checked
against the restatement's; and on the 64 scenarios of the call past its staging budget, with and without the u16 staging.
The drop-only scenarios' start slots are also the reference project's own rule (grids_limit_cases.reference_rule_slots,
asserted in restate()).  tests/test_gpu_weather_grids_fuzz.py runs the same cases on the device."""
import numpy as np
import pytest

import generic_cases as G
import grids_host_build as GH
import grids_limit_cases as GL
import grids_ref as GR
import kernel_host_build as KH
import resume_ref as RR

SIMS, OFFSET = GL.FUZZ_SIMS, GL.FUZZ_OFFSET


@pytest.mark.parametrize('part', range(GL.PARTS))
def test_emulated_kernel_on_every_input(part):
    for name, case, seed, scen, want_o, want_s in GL.wanted(part)[0]:
        got = GH.grids(case, [pl for _, pl in scen], [ed for ed, _ in scen], SIMS, seed, OFFSET, prob=KH.generic_problem(case))
        GL.check_against(got, case, want_o, want_s, SIMS)
        assert np.array_equal(got['slots'], want_s), name


def test_the_mixtures_do_not_pass_empty():
    """Inputs with a simulation in which an unplaced car jumped a pin, two unplaced keys tied, an order moved: the
    restatement's own counts, against floors about a tenth below what it gave when the cases were written."""
    assert GL.marks() == GL.MEASURED
    GL.check_floors(GL.marks(), GL.FLOORS)


def test_the_generator_makes_what_the_hand_made_sets_lack():
    """From the generated edits alone, over the 100 inputs: scenarios with more than two pit-lane cars, with every driver
    edited beside pins, with free slots on both sides of a pinned one, with seconds of 0, 5e-324 and 1e6 together, and with
    a drop beside a pin."""
    lanes = everyone = holes = seconds = drop_and_pin = 0
    for name, case, _ in G.run_inputs():
        n = len(case['grid_probs'])
        for ed, _ in GL.scenarios(name, case)[1:1 + GL.MIXTURES]:
            kinds = [k for k, _, _ in ed.values()]
            lane = [sec for k, _, sec in ed.values() if k == GL.PIT_LANE]
            pins = sorted(v - 1 for k, v, _ in ed.values() if k == GL.PIN)
            front = [p for p in range(n - len(lane)) if p not in pins]
            lanes += len(lane) > 2
            everyone += len(ed) == n and len(pins) < n
            holes += any(min(front) < p < max(front) for p in pins) if front else 0
            seconds += {0.0, 5e-324, 1e6} <= set(lane)
            drop_and_pin += GL.DROP in kinds and GL.PIN in kinds
    assert lanes >= 300 and everyone >= 10 and holes >= 300 and seconds >= 100 and drop_and_pin >= 300, \
        (lanes, everyone, holes, seconds, drop_and_pin)


def test_f33_under_64_scenarios_and_the_slots_without_a_race():
    """The call of the device's counting-loop test at its first 8 simulations: the emulated kernel is the restatement,
    and the slots that test expects at every simulation (edited_grid alone) are the restatement's."""
    case = G.fuzz_cases()['F33']
    seed, n = case['seed'], len(case['grid_probs'])
    scen = GL.full_scenarios('F33', case)
    ref = RR.traced_run(case, SIMS, seed, OFFSET)
    want_o, want_s = GL.restate(case, seed, scen, ref['grids'], SIMS, OFFSET)
    assert np.array_equal(GL.edited_slots(scen, ref['grids']), want_s)
    assert sum(GL.only_drops(ed) for ed, _ in scen) == 2 and len({w.tobytes() for w in want_s}) > 50
    got = GH.grids(case, [pl for _, pl in scen], [ed for ed, _ in scen], SIMS, seed, OFFSET)
    GL.check_against(got, case, want_o, want_s, SIMS)
    assert np.array_equal(got['slots'], want_s)
    assert np.array_equal(got['start'], GR.start_counts(GL.edited_slots(scen, ref['grids']), n))


def test_the_scenarios_of_the_call_past_its_budget_with_and_without_the_start_staging():
    case = RR.field_case(32)
    case['config'] = dict(case['config'], total_laps=3)
    seed, n = 9, 32
    scen = GL.full_scenarios('n32', case)
    ref = RR.traced_run(case, SIMS, seed, OFFSET)
    want_o, want_s = GL.restate(case, seed, scen, ref['grids'], SIMS, OFFSET)
    plans, edits = [pl for _, pl in scen], [ed for ed, _ in scen]
    hist, stage, car, start, gain = GH.grids_raw(case, plans, edits, SIMS, seed, OFFSET)
    assert np.array_equal(GH.decode(stage), want_o) and np.array_equal(car, want_s)
    assert np.array_equal(start, GR.start_counts(want_s, n)) and np.array_equal(gain, GR.gain_counts(want_s, want_o, n))
    assert np.array_equal(hist, GR.hist_counts(want_o, n))
    hist2, stage2, car2, start2, gain2 = GH.grids_raw(case, plans, edits, SIMS, seed, OFFSET, stage_start=False)
    assert car2 is None and not start2.any() and not gain2.any()
    assert np.array_equal(hist2, hist) and np.array_equal(stage2, stage)
