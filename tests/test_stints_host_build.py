"""race_stints_kernel<false> and <true> (csrc/stints.hip.h) compiled for the host (tools/emu/emu_generic.cpp) and
compared, integers only, with references that do not share its code: the raw staging -- records and position bytes,
decoded by the layout documented at the top of stints.hip.h -- against stints_ref's numpy restatement over the CPU
oracle's per-lap trace (tyre age, compound, retirement) and the restated event draws; the histogram against the
oracle's.  Inputs: seven golden cases, a cap case, fields of 1, 2 and 32 cars, and a second pass over everything
generic_cases.py holds -- the 8 golden cases, the 84 fuzz configurations with their corner cases, lap times near zero
and at the overtake's floor, fields of 1, 2, 3, 19, 31 and 32 cars -- from the grid and from the states of
conditions_ref.state_runs.  The counting kernel and the host-side chunking are compared on the device
(test_gpu_stints.py, test_gpu_stints_moves_fuzz.py).  The host build is test infrastructure: nothing under
monte_carlo_gp_amd/ can reach it and the product has no CPU path."""
import numpy as np
import pytest

import conditions_ref as CR
import generic_cases as G
import oracle_py as O
import resume_ref as RR
import stints_host_build as SH
import stints_ref as SR

SIMS = 96
RUN_SIMS, STATE_SIMS, OFFSET, BASE = 32, 4, 3, 40
GOLDEN = ('S60', 'EVT', 'WET', 'N10', 'HET', 'S78', 'DMP')


def _same(name, got, ref):
    for key in SR.KEYS:
        bad = np.argwhere(got[key] != ref[key])
        assert bad.size == 0, (name, key, bad[:5].tolist())


@pytest.mark.parametrize('name', GOLDEN)
def test_golden_cases_from_the_grid(name):
    case = O.load_case(name)
    ref, t = SR.stint_counts(case, SIMS, seed=7, with_tallies=True)
    got = SH.stints(case, SIMS, seed=7)
    _same(name, got, ref)
    n = ref['hist'].shape[0]
    assert (got['stop_lap'].sum(axis=2) == SIMS).all() and (got['seq'].sum(axis=1) == SIMS).all()
    assert not got['stop_lap'][:, :, 1].any() and np.array_equal(got['stops_pos'].sum(axis=1), got['hist'])
    if name == 'WET':
        assert not t['stops'].any() and t['stints'].max() >= 3          # red-flag changes start stints without a stop
    if name == 'S60':
        assert len(np.unique(t['stops'])) == 3 and n == 20


def test_the_record_of_every_car_field_by_field():
    """The raw records against the reference's per-car tallies, not only their counts."""
    case = O.load_case('EVT')
    ref, t = SR.stint_counts(case, SIMS, seed=7, with_tallies=True)
    _, rec, pos = SH.stints_raw(case, SIMS, seed=7)
    f = SH.decode(rec)
    assert (t['stints'] > 4).any() and (t['stints'] <= 4).any()
    assert np.array_equal(f['stints'].T, np.minimum(t['stints'], 15)) and np.array_equal(f['stops'].T, np.minimum(t['stops'], 15))
    assert np.array_equal(f['laps'].transpose(1, 0, 2), t['laps'])


def test_the_cap_case():
    case = SR.cap_case()
    ref, t = SR.stint_counts(case, 64, seed=3, with_tallies=True)
    # checked on the CPU oracle: a fifth stop, stops under a red flag, many stints
    assert int((t['stops'] == 5).sum()) == 1267 and t['stops'].size == 1280
    assert t['both'] == 3168 and t['stints'].max() == 12
    got = SH.stints(case, 64, seed=3)
    _same('cap', got, ref)
    assert got['stops_pos'][:, 4].sum() >= 1267 and got['seq'][:, 0].sum() > 0


@pytest.mark.parametrize('n', [1, 2, 32])
def test_synthetic_fields(n):
    case = RR.field_case(n)
    _same(n, SH.stints(case, SIMS, seed=3), SR.stint_counts(case, SIMS, seed=3))


def test_oracle_states_continue_into_the_oracle_trace():
    """Simulation i's state after laps 1, L / 2 and L resumed as simulation i: the counts are the oracle trace's of the
    later laps; from lap L no lap is left, so every record is the start's own (one stint on the state's compound, no
    stop) -- nothing of any lap is written."""
    for name in ('S60', 'EVT', 'N10'):
        case = O.load_case(name)
        L, seed, base, m = case['config']['total_laps'], 11, 500, 4
        ref = RR.traced_run(case, m, seed, base)
        prob = SH.KH.generic_problem(case)
        for i in range(m):
            for k in (1, L // 2, L):
                st = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k))
                hist, rec, pos = SH.stints_raw(case, 1, seed, sim_offset=base + i, state=st, prob=prob)
                want = SR.continued_counts(ref, [i], k, case, seed, base)
                got = SH.counts_from_staging(rec, pos, L)
                got['hist'] = hist
                _same((name, i, k), got, want)
                if k == L:
                    comp = ref['trace']['comp'][i, L - 1].astype(np.uint64)
                    assert np.array_equal(rec[:, 0], np.uint64(1) | (comp << np.uint64(4))), (name, i)
                    assert not got['stop_lap'][:, :, 1:].any()


# ---------------------------------------------------------------- the second pass: every input of generic_cases.py
def test_stints_kernel_from_the_grid_on_every_input():
    """All of generic_cases.run_inputs() at each input's own seed: every key equals stints_ref over the oracle's trace."""
    inputs = G.run_inputs()
    done = 0
    for name, case, seed in inputs:
        ref = RR.traced_run(case, RUN_SIMS, seed, OFFSET)
        got = SH.stints(case, RUN_SIMS, seed, sim_offset=OFFSET)
        _same(name, got, SR.stint_counts(case, RUN_SIMS, seed, OFFSET, ref=ref))
        assert (got['stop_lap'].sum(axis=2) == RUN_SIMS).all() and (got['seq'].sum(axis=1) == RUN_SIMS).all(), name
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and len(inputs) == 100


def test_stints_kernel_from_a_state_on_every_input():
    """All of generic_cases.resume_inputs(): four simulations' states after every lap of resume_laps, each continued as
    itself; the records are the oracle trace's of the later laps, stint 0 on the state's compound."""
    done = states = 0
    for name, case, seed in G.resume_inputs():
        L = case['config']['total_laps']
        ref = RR.traced_run(case, STATE_SIMS, seed, BASE)
        runs = CR.state_runs(case, seed, ref, range(STATE_SIMS), BASE)
        prob = SH.KH.generic_problem(case)
        for i, k, st in runs:
            hist, rec, pos = SH.stints_raw(case, 1, seed, sim_offset=BASE + i, state=st, prob=prob)
            got = SH.counts_from_staging(rec, pos, L)
            got['hist'] = hist
            _same((name, i, k), got, SR.continued_counts(ref, [i], k, case, seed, BASE))
            assert not got['stop_lap'][:, :, 1:k + 1].any(), (name, i, k)
        assert len(runs) >= STATE_SIMS, name
        states += len(runs)
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and states >= 94 * STATE_SIMS * 3, (done, states)
