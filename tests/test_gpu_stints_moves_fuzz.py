"""mcgp_run_stints and mcgp_run_moves on the device over the inputs of generic_cases.py -- the comparisons of the second
passes of test_stints_host_build.py and test_moves_host_build.py, through the C ABI: race_stints_kernel<false / true>
and race_moves_kernel<false / true> at every block shape the inputs' field sizes give, and the three counting kernels
that no host build can run (stints_count, moves_count_laps, moves_count_drivers: ballots and shuffles) -- on every
input, at sizes where their grid-stride loops iterate, and at simulation counts that leave a wave ragged.

References, none of which shares code with the kernels: stints_ref and moves_ref over the CPU oracle's per-lap trace
(resume_ref.traced_run, one run per input shared by both), the product's mcgp_run and mcgp_run_from_state for the
histograms.  Every comparison is integer equality.  What keeps the comparisons from being vacuous -- ties that decide a
pass, records past the 4-bit fields, pit passes, races without a pass, sequences of more than four stints -- is asserted
from the reference alone, before the device's result is looked at.  The oracle's runs are made in a pool of at most 16
threads; what is Python on top of them is not, as threads only slow that down.

Compared on the device: 64 simulations on 100 inputs from the grid; 4 simulations x up to 7 laps on 94 inputs from
states, accumulated into buffers of fives; F33 (20 cars) at two rounds and a ragged third of stints_count and
moves_count_drivers, F13 (3 cars) at one and a half rounds of moves_count_laps, both within one staging chunk; fields
of 31 and 3 cars at 63, 65, 129 and 257 simulations.  Cost: the device calls are milliseconds each, the file's time is
the host's references.  Wall time on an MI355X machine (256 CUs), in one visit: this file 27.9 s (15.0 s of it
the F33 references, 4.5 s the F13 ones), tests/test_gpu_generic_fuzz.py 22.5 s (the yardstick: at most twice its time,
else STATE_SIMS goes from 4 to 2 with the state floors, then the F13 size is halved).

The reference shows, at these parameters: 29 inputs with a tie that decides a pass, 62 with a pit pass, 24 with a race
without any pass (25 without one on track), 34 with a non-empty seq[:, 0]; 2 269 states, 1 488 with a pass and 882 with
a stop after the state.  The floors asserted below are conditions, set below those figures."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import conditions_ref as CR
import generic_cases as G
import moves_ref as MR
import oracle_py as O
import resume_ref as RR
import stints_ref as SR
from helpers import product_run
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

SIMS, STATE_SIMS, OFFSET, BASE = 64, 4, 3, 40
STINTS_KERNEL, MOVES_KERNEL = 'mcgp::race_stints_kernel', 'mcgp::race_moves_kernel'
COUNT_BLOCK, LAPS_BLOCK = 256, 128          # threads of a stints_count / moves_count_drivers and a moves_count_laps block


def _check(rc):
    assert rc == 0, N.lib().mcgp_last_error().decode()


def _kernel():
    return N.lib().mcgp_last_kernel_name(0).decode()


def _equal(got, want, what, keys):
    for key in keys:
        assert got[key].shape == want[key].shape, (what, key)
        bad = np.argwhere(got[key] != want[key])
        assert bad.size == 0, (what, key, len(bad), bad[:5].tolist(), got[key][tuple(bad[0])], want[key][tuple(bad[0])])


def _stints_invariants(got, m):
    assert (got['stop_lap'].sum(axis=2) == m).all() and not got['stop_lap'][:, :, 1].any()
    assert (got['seq'].sum(axis=1) == m).all()
    assert np.array_equal(got['stops_pos'].sum(axis=1), got['hist'])


def _moves_invariants(got, m, from_grid=True):
    assert np.array_equal(got['grid_fin'].sum(axis=1), got['hist'])
    assert (got['passes'].sum(axis=2) == m).all() and got['race_passes'].sum() == m
    assert not got['lap_passes'][:2].any() and not np.diag(got['pair_passes']).any()
    assert (got['start_gain'].sum(axis=1) == (m if from_grid else 0)).all()
    assert got['pair_passes'].sum() == got['lap_passes'][:, 0].sum()


@functools.lru_cache(maxsize=None)
def _traced(which):
    """The oracle's traced runs, made once and shared by the stints and the moves comparison: 'grid' of every run input,
    'states' of every resume input (the runs whose states both entry points continue).  [(name, case, seed, ref)]."""
    inputs = G.resume_inputs() if which == 'states' else G.run_inputs()
    m, offset = {'grid': (SIMS, OFFSET), 'states': (STATE_SIMS, BASE)}[which]
    O.lib()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        refs = list(pool.map(lambda a: RR.traced_run(a[1], m, a[2], offset), inputs))
    return [(name, case, seed, ref) for (name, case, seed), ref in zip(inputs, refs)]


@functools.lru_cache(maxsize=None)
def _states():
    """[(name, case, seed, ref, runs, hists)]: every resume input's states (conditions_ref.state_runs) and
    mcgp_run_from_state's histogram of each continued as itself, one batched call per input."""
    out = []
    for name, case, seed, ref in _traced('states'):
        runs = CR.state_runs(case, seed, ref, range(STATE_SIMS), BASE)
        rc, hists, _ = RR.run_c(RR.problem(case), [st for _, _, st in runs], 1, [BASE + i for i, _, _ in runs], seed,
                                orders=False)
        _check(rc)
        out.append((name, case, seed, ref, runs, hists))
    return out


def _fives(empty):
    return {key: np.full_like(v, 5, dtype=np.uint64) for key, v in empty.items()}


def _decisive_ties(ref):
    """From the oracle's trace alone: the (simulation, lap k, pair) cells with both cars running at EQUAL cumulative time
    after lap k whose order -- (time, grid slot) in the reference, `Ord` in the kernel -- differs from the pair's order a
    lap earlier or a lap later, both running there too: the tie's side decides whether a pass is counted on lap k or on
    lap k + 1 (passes are counted from lap 2 on)."""
    tr = ref['trace']
    cum, run = tr['cum'], tr['dnf'] == 0
    m, L, n = cum.shape
    if L < 2 or n < 2:
        return 0
    slot = MR.slots_of(ref['grids'])
    pos = np.stack([MR.running_positions(cum[:, k], tr['dnf'][:, k], slot) for k in range(L)], axis=1)
    both = run[:, :, :, None] & run[:, :, None, :] & np.triu(np.ones((n, n), bool), 1)
    tie = both & (cum[:, :, :, None] == cum[:, :, None, :])
    first = pos[:, :, :, None] < pos[:, :, None, :]
    flip = both[:, 1:] & both[:, :-1] & (first[:, 1:] != first[:, :-1])          # between lap j + 1 and lap j + 2
    return int(((tie[:, 1:] | tie[:, :-1]) & flip).sum())


# ---------------------------------------------------------------- a. from the grid on every input
def test_stints_from_the_grid_on_every_input(require_gpu):
    done, many_stints, many_stops, column0 = 0, set(), set(), set()
    for name, case, seed, ref in _traced('grid'):
        want, t = SR.stint_counts(case, SIMS, seed, OFFSET, ref=ref, with_tallies=True)
        if t['stints'].max() >= 16:
            many_stints.add(name)                     # the record's stint count stays at 15
        if t['stops'].max() >= 16:
            many_stops.add(name)                      # ... and its stop count
        if want['seq'][:, 0].any():
            column0.add(name)
        n, L = len(case['grid_probs']), case['config']['total_laps']
        if name == 'X_onelap':
            assert L == 1 and want['stop_lap'].shape == (n, 4, 2) and not want['stop_lap'][:, :, 1:].any()
        rc, got = SR.run_c(case, SIMS, seed, sim_offset=OFFSET)
        _check(rc)
        assert _kernel() == STINTS_KERNEL, name
        _equal(got, want, name, SR.KEYS)
        _stints_invariants(got, SIMS)
        hist, _, _ = product_run(case, SIMS, seed, sim_offset=OFFSET)
        assert np.array_equal(got['hist'], hist), name
        if name == 'X_onelap':
            assert got['stop_lap'].shape == (n, 4, 2) and got['stops_pos'].shape == (n, 5, n) and got['seq'].shape == (n, 1296)
            assert not got['stop_lap'][:, :, 1:].any()
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ
    assert {'F57', 'F66', 'X_always_red', 'X_pit_every_lap'} <= many_stints, sorted(many_stints)
    assert {'F66', 'X_pit_every_lap'} <= many_stops, sorted(many_stops)
    assert len(column0) >= 30, len(column0)


def test_moves_from_the_grid_on_every_input(require_gpu):
    done, tied, pit, quiet = 0, set(), set(), set()
    for name, case, seed, ref in _traced('grid'):
        want, t = MR.move_counts(case, SIMS, seed, OFFSET, ref=ref, with_tallies=True)
        if _decisive_ties(ref):
            tied.add(name)
        if t['kinds'][:, :, 2].any():
            pit.add(name)
        if (t['lap'].sum(axis=(1, 2)) == 0).any():
            quiet.add(name)                           # a race without any pass, on track or through the pits
        n, L = len(case['grid_probs']), case['config']['total_laps']
        assert (want['start_gain'].sum(axis=1) == SIMS).all(), name
        if name == 'X_onelap':
            assert L == 1 and want['lap_passes'].shape == (2, 2)
            assert not want['lap_passes'].any() and not want['pair_passes'].any()
        rc, got = MR.run_c(case, SIMS, seed, sim_offset=OFFSET)
        _check(rc)
        assert _kernel() == MOVES_KERNEL, name
        _equal(got, want, name, MR.KEYS)
        _moves_invariants(got, SIMS)
        assert (got['start_gain'].sum(axis=1) == SIMS).all(), name
        hist, _, _ = product_run(case, SIMS, seed, sim_offset=OFFSET)
        assert np.array_equal(got['hist'], hist), name
        if name == 'X_onelap':
            assert got['lap_passes'].shape == (2, 2) and got['pair_passes'].shape == (n, n)
            assert got['grid_fin'].shape == (n, n, n) and got['start_gain'].shape == (n, 2 * n)
            assert got['passes'].shape == (n, 4, 128) and got['race_passes'].shape == (1024,)
            assert not got['lap_passes'].any() and not got['pair_passes'].any()
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ
    assert len(tied) >= 25 and {'X_no_noise', 'X_all_attempt'} <= tied, sorted(tied)
    assert len(pit) >= 55, len(pit)
    assert len(quiet) >= 20, len(quiet)


# ---------------------------------------------------------------- b. from a state on every resume input
def test_stints_from_a_state_on_every_input(require_gpu):
    """Every state continued as itself, accumulated into buffers of fives: the counts gained are the oracle trace's of
    laps k + 1 .. L with stint 0 on the state's compound, no stop lap up to k is touched, the histogram is
    mcgp_run_from_state's."""
    done = states = with_stop = 0
    for name, case, seed, ref, runs, hists in _states():
        prob = RR.problem(case)
        n, L = prob.n, case['config']['total_laps']
        for s, (i, k, st) in enumerate(runs):
            want = SR.continued_counts(ref, [i], k, case, seed, BASE)
            with_stop += bool(want['stop_lap'][:, :, 1:].any())
            rc, got = SR.run_c(case, 1, seed, sim_offset=BASE + i, state=st, prob=prob, into=_fives(SR.empty(n, L)))
            _check(rc)
            assert _kernel() == STINTS_KERNEL, name
            assert (got['stop_lap'][:, :, 1:k + 1] == 5).all(), (name, i, k)
            got = {key: v - 5 for key, v in got.items()}
            _equal(got, want, (name, i, k), SR.KEYS)
            _stints_invariants(got, 1)
            assert np.array_equal(got['hist'], hists[s]), (name, i, k)
        assert len(runs) >= STATE_SIMS, name
        states += len(runs)
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and states >= 94 * STATE_SIMS * 3, (done, states)
    assert with_stop >= 700, with_stop


def test_moves_from_a_state_on_every_input(require_gpu):
    """Every state continued as itself, accumulated into buffers of fives: the counts gained are the oracle trace's of
    laps k + 1 .. L against the baseline after lap k, the lap rows up to k + 1 and the start gains stay five, the
    histogram is mcgp_run_from_state's."""
    done = states = with_pass = 0
    for name, case, seed, ref, runs, hists in _states():
        prob = RR.problem(case)
        n, L = prob.n, case['config']['total_laps']
        for s, (i, k, st) in enumerate(runs):
            want = MR.continued_counts(ref, [i], k)
            with_pass += bool(want['lap_passes'].any())
            rc, got = MR.run_c(case, 1, seed, sim_offset=BASE + i, state=st, prob=prob, into=_fives(MR.empty(n, L)))
            _check(rc)
            assert _kernel() == MOVES_KERNEL, name
            assert (got['lap_passes'][:k + 1] == 5).all() and (got['start_gain'] == 5).all(), (name, i, k)
            got = {key: v - 5 for key, v in got.items()}
            _equal(got, want, (name, i, k), MR.KEYS)
            _moves_invariants(got, 1, from_grid=False)
            assert np.array_equal(got['hist'], hists[s]), (name, i, k)
        assert len(runs) >= STATE_SIMS, name
        states += len(runs)
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and states >= 94 * STATE_SIMS * 3, (done, states)
    assert with_pass >= 1200, with_pass


# ---------------------------------------------------------------- c. counting loops past one round, against the oracle
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_driver_counting_loops_past_two_rounds(require_gpu):
    """stints_count and moves_count_drivers launch min(tiles, max(1, 8 CUs / n)) blocks of 256 per driver (the rule
    restated here, not read back): F33 -- 20 cars over 9 laps, stops and pit passes -- at two full passes of every block
    and a ragged third, in one staging chunk, so that the loop is the kernel's own."""
    case = G.fuzz_cases()['F33']
    seed, n, L = case['seed'], len(case['grid_probs']), case['config']['total_laps']
    assert (n, L) == (20, 9)
    one_round = max(1, 8 * _cus() // n) * COUNT_BLOCK
    m = 2 * one_round + 77
    assert m > 2 * one_round and m % COUNT_BLOCK and m % 64
    assert m < SR.budget_sims(n) and m < MR.budget_sims(n, L)
    ref = RR.traced_run(case, m, seed, OFFSET)
    moves, tm = MR.move_counts(case, m, seed, OFFSET, ref=ref, with_tallies=True)
    stints, ts = SR.stint_counts(case, m, seed, OFFSET, ref=ref, with_tallies=True)
    assert tm['kinds'][:, :, 0].sum() > 0 and tm['kinds'][:, :, 2].sum() > 0 and int((ts['stops'] == 1).sum()) > 0
    rc, got = SR.run_c(case, m, seed, sim_offset=OFFSET)
    _check(rc)
    assert _kernel() == STINTS_KERNEL
    _equal(got, stints, 'F33 stints', SR.KEYS)
    _stints_invariants(got, m)
    rc, got = MR.run_c(case, m, seed, sim_offset=OFFSET)
    _check(rc)
    assert _kernel() == MOVES_KERNEL
    _equal(got, moves, 'F33 moves', MR.KEYS)
    _moves_invariants(got, m)


def test_lap_counting_loop_past_one_round(require_gpu):
    """moves_count_laps launches min(tiles, 8 CUs) blocks of 128 (more only above 2^14 tiles per block; restated here,
    not read back), every thread keeping its simulation's tables in LDS: F13 -- 3 cars over 22 laps, pit passes and
    lap-1 retirements -- at one and a half rounds and a partial block, so that half the blocks walk a second simulation
    over the tables of the first, in one staging chunk."""
    case = G.fuzz_cases()['F13']
    seed, n, L = case['seed'], len(case['grid_probs']), case['config']['total_laps']
    assert (n, L) == (3, 22)
    blocks = 8 * _cus()
    one_round = blocks * LAPS_BLOCK
    m = 3 * blocks * LAPS_BLOCK // 2 + 77
    if m > 10 ** 6:
        pytest.skip(f'{_cus()} CUs: one and a half rounds of moves_count_laps are {m} simulations, more than 10^6')
    tiles = -(-m // LAPS_BLOCK)
    assert one_round < m < 2 * one_round and m % LAPS_BLOCK and blocks < tiles < blocks << 14
    assert m < MR.budget_sims(n, L)
    ref = RR.traced_run(case, m, seed, OFFSET)
    want, t = MR.move_counts(case, m, seed, OFFSET, ref=ref, with_tallies=True)
    assert t['kinds'][:, :, 0].sum() > 0 and t['kinds'][:, :, 2].sum() > 0 and want['start_gain'][:, -1].sum() > 0
    # the second simulation of a thread differs from its first: stale tables would show
    assert (t['kinds'][:one_round // 2] != t['kinds'][one_round:one_round + one_round // 2]).any()
    rc, got = MR.run_c(case, m, seed, sim_offset=OFFSET)
    _check(rc)
    assert _kernel() == MOVES_KERNEL
    _equal(got, want, 'F13 moves', MR.KEYS)
    _moves_invariants(got, m)


# ---------------------------------------------------------------- d. ragged waves
@pytest.mark.parametrize('n', [31, 3])
def test_ragged_waves(require_gpu, n):
    """Simulation counts that leave the last wave of the counting kernels one lane short, one lane in, or one lane past
    a wave, two waves and a block: the lanes without a simulation in wave_count's ballots and in the shuffle reduction
    of the lap sums."""
    case, seed = RR.field_case(n), 5
    for m in (63, 65, 129, 257):
        ref = RR.traced_run(case, m, seed, OFFSET)
        moves, t = MR.move_counts(case, m, seed, OFFSET, ref=ref, with_tallies=True)
        stints = SR.stint_counts(case, m, seed, OFFSET, ref=ref)
        assert t['lap'][:, :, 0].any() and stints['stop_lap'][:, 0, 2:].any()
        rc, got = SR.run_c(case, m, seed, sim_offset=OFFSET)
        _check(rc)
        _equal(got, stints, (n, m, 'stints'), SR.KEYS)
        _stints_invariants(got, m)
        rc, got = MR.run_c(case, m, seed, sim_offset=OFFSET)
        _check(rc)
        _equal(got, moves, (n, m, 'moves'), MR.KEYS)
        _moves_invariants(got, m)
