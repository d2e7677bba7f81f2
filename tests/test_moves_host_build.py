"""race_moves_kernel<false> and <true> (csrc/moves.hip.h) compiled for the host (tools/emu/emu_generic.cpp) and
compared, integers only, with a reference that does not share its code: the raw staging -- the per-lap bytes, the grid
slots and the classified positions, decoded by the layout documented at the top of moves.hip.h -- against moves_ref's
numpy restatement over the CPU oracle's per-lap trace (cumulative time, retirement, tyre age, grids, orders); the
histogram against the oracle's.  Inputs: seven golden cases, fields of 1, 2 and 32 cars, and a second pass
over everything generic_cases.py holds -- the 8 golden cases, the 84 fuzz configurations with their corner cases, lap
times near zero and at the overtake's floor, fields of 1, 2, 3, 19, 31 and 32 cars -- from the grid and from the states
of conditions_ref.state_runs.  The counting kernels and the host-side chunking are compared on the device
(test_gpu_moves.py, test_gpu_stints_moves_fuzz.py).  The host build is test infrastructure: nothing under
monte_carlo_gp_amd/ can reach it and the product has no CPU path."""
import numpy as np
import pytest

import conditions_ref as CR
import generic_cases as G
import moves_host_build as MH
import moves_ref as MR
import oracle_py as O
import resume_ref as RR

SIMS = 128
RUN_SIMS, STATE_SIMS, OFFSET, BASE = 32, 4, 3, 40
GOLDEN = ('S60', 'EVT', 'WET', 'N10', 'HET', 'S78', 'DMP')


def _same(name, got, ref, keys=MR.KEYS):
    for key in keys:
        bad = np.argwhere(got[key] != ref[key])
        assert bad.size == 0, (name, key, bad[:5].tolist())


@pytest.mark.parametrize('name', GOLDEN)
def test_golden_cases_from_the_grid(name):
    case = O.load_case(name)
    ref, t = MR.move_counts(case, SIMS, seed=7, with_tallies=True)
    got = MH.moves(case, SIMS, seed=7)
    _same(name, got, ref)
    assert np.array_equal(got['grid_fin'].sum(axis=1), got['hist'])
    assert (got['start_gain'].sum(axis=1) == SIMS).all() and (got['passes'].sum(axis=2) == SIMS).all()
    assert got['race_passes'].sum() == SIMS and not got['lap_passes'][:2].any()
    assert t['kinds'][:, :, 0].sum() == t['kinds'][:, :, 1].sum() == got['pair_passes'].sum() == got['lap_passes'][:, 0].sum()
    assert t['kinds'][:, :, 2].sum() == t['kinds'][:, :, 3].sum() == got['lap_passes'][:, 1].sum()
    if name == 'WET':
        assert not t['kinds'][:, :, 2:].any() and t['kinds'][:, :, 0].any()      # no stop on wet tyres: no pit pass
    if name == 'S60':
        assert t['kinds'][:, :, 2].any() and t['race'].min() > 100


def test_the_staged_bytes_of_every_lap():
    """The raw per-lap bytes against the reference's positions and pit stops, not only their counts."""
    case = O.load_case('EVT')
    ref = RR.traced_run(case, SIMS, 7)
    tr, slot = ref['trace'], MR.slots_of(ref['grids'])
    _, laps, s, p = MH.moves_raw(case, SIMS, seed=7)
    L, n = tr['cum'].shape[1], tr['cum'].shape[2]
    for k in range(1, L + 1):
        pos = MR.running_positions(tr['cum'][:, k - 1], tr['dnf'][:, k - 1], slot)
        pit = (pos < n) & (tr['age'][:, k - 1] == 0) & (k >= 2)
        assert np.array_equal((laps[k - 1] & MH.POS_MASK).T, pos), k
        assert np.array_equal(((laps[k - 1] & MH.PIT) != 0).T, pit), k
    assert np.array_equal(s.T, slot) and np.array_equal(p.T, MR.positions_of(ref['orders']))


@pytest.mark.parametrize('n', [1, 2, 32])
def test_synthetic_fields(n):
    case = RR.field_case(n)
    _same(n, MH.moves(case, SIMS, seed=3), MR.move_counts(case, SIMS, seed=3))


def test_oracle_states_continue_into_the_oracle_trace():
    """Simulation i's state after laps 1, L / 2 and L resumed as simulation i: the counts are the oracle trace's of the
    later laps against the baseline after the state's lap.  After lap L only the baseline, slot and position rows are
    written (moves_raw asserts that no earlier row is) and every pass count is 0."""
    for name in ('S60', 'EVT', 'N10'):
        case = O.load_case(name)
        L, seed, base, m = case['config']['total_laps'], 11, 500, 4
        ref = RR.traced_run(case, m, seed, base)
        prob = MH.KH.generic_problem(case)
        n = prob[0].n
        for i in range(m):
            for k in (1, L // 2, L):
                st = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k))
                hist, laps, slot, pos = MH.moves_raw(case, 1, seed, sim_offset=base + i, state=st, prob=prob)
                got, _ = MH.counts_from_staging(laps, slot, pos, k, False)
                got['hist'] = hist
                want = MR.continued_counts(ref, [i], k)
                _same((name, i, k), got, want)
                assert not got['start_gain'].any()
                if k == L:
                    assert got['passes'][:, :, 0].sum() == 4 * n and got['race_passes'][0] == 1
                    assert not got['lap_passes'].any() and not got['pair_passes'].any()


# ---------------------------------------------------------------- the second pass: every input of generic_cases.py
def test_moves_kernel_from_the_grid_on_every_input():
    """All of generic_cases.run_inputs() at each input's own seed: every key equals moves_ref over the oracle's trace."""
    inputs = G.run_inputs()
    done = 0
    for name, case, seed in inputs:
        ref = RR.traced_run(case, RUN_SIMS, seed, OFFSET)
        got = MH.moves(case, RUN_SIMS, seed, sim_offset=OFFSET)
        _same(name, got, MR.move_counts(case, RUN_SIMS, seed, OFFSET, ref=ref))
        assert (got['start_gain'].sum(axis=1) == RUN_SIMS).all(), name
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and len(inputs) == 100


def test_moves_kernel_from_a_state_on_every_input():
    """All of generic_cases.resume_inputs(): four simulations' states after every lap of resume_laps, each continued as
    itself; the staging's counts are the oracle trace's of the later laps against the baseline after the state's lap."""
    done = states = 0
    for name, case, seed in G.resume_inputs():
        ref = RR.traced_run(case, STATE_SIMS, seed, BASE)
        runs = CR.state_runs(case, seed, ref, range(STATE_SIMS), BASE)
        prob = MH.KH.generic_problem(case)
        for i, k, st in runs:
            hist, laps, slot, pos = MH.moves_raw(case, 1, seed, sim_offset=BASE + i, state=st, prob=prob)
            got, _ = MH.counts_from_staging(laps, slot, pos, k, False)
            got['hist'] = hist
            _same((name, i, k), got, MR.continued_counts(ref, [i], k))
            assert not got['start_gain'].any() and not got['lap_passes'][:k + 1].any(), (name, i, k)
        assert len(runs) >= STATE_SIMS, name
        states += len(runs)
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and states >= 94 * STATE_SIMS * 3, (done, states)
