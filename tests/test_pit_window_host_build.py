"""race_window_kernel<false> and <true> (csrc/pit_window.hip.h) compiled for the host (tools/emu/emu_generic.cpp) and
compared, integers only, with a reference that does not share its code: the raw staging, decoded by the layout
documented at the top of pit_window.hip.h, against window_ref's numpy restatement over the CPU oracle's per-lap trace;
the histogram against the oracle's.  Inputs (generic_cases.py): the 8 golden cases, the 84 fuzz configurations, two
fields with tiny lap times, synthetic fields of 1, 2, 3, 19, 31 and 32 cars; window counts around the register group;
losses at which the rejoin time equals another car's, where the grid slots decide.  The counting kernel and the host-side
chunking are compared on the device (test_gpu_pit_window.py).  The host build is test infrastructure: nothing under
monte_carlo_gp_amd/ can reach it and the product has no CPU path."""
import numpy as np

import gaps_ref as GR
import generic_cases as G
import oracle_py as O
import pit_window_host_build as PH
import resume_ref as RR
import window_ref as WR

RUN_SIMS, RESUME_SIMS, TIE_SIMS = 32, 8, 48
GROUP = 8               # csrc/pit_window.hip.h: kWindowGroup


def _windows(case, n):
    """Every driver at the configured pit loss and at no loss at all, at most 64 windows."""
    return WR.every_driver(n, [float(case['config']['pit_loss']), 0.0])


def _same(name, got, ref):
    for key in WR.KEYS:
        assert np.array_equal(got[key], ref[key]), (name, key)


def _check(name, case, m, seed, offset, windows, ref=None, edges=WR.DEFAULT_EDGES):
    """The staged values and the histogram of one input against the reference -> (reference values, traced run)."""
    ref = ref or RR.traced_run(case, m, seed, offset)
    tr = ref['trace']
    want = WR.values_from_times(tr['cum'], tr['dnf'], GR.slots_of(ref['grids']), windows, edges)
    hist, got = PH.window_values(case, m, seed, sim_offset=offset, windows=windows, edges=edges)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f'{name}: {len(bad)} staged values differ, first (simulation, lap - 1, window, row) ' \
                          f'{bad[:3].tolist()}: got {[int(got[tuple(b)]) for b in bad[:3]]}, ' \
                          f'reference {[int(want[tuple(b)]) for b in bad[:3]]}'
    assert np.array_equal(hist, ref['hist']), name
    return want, ref


def test_window_kernel_from_the_grid_equals_the_restated_values():
    done, seen = 0, [set() for _ in WR.ROWS]
    for name, case, seed in G.run_inputs():
        n = len(case['grid_probs'])
        want, _ = _check(name, case, RUN_SIMS, seed, 3, _windows(case, n))
        if n == 20:
            for r in range(5):
                seen[r] |= set(np.unique(want[..., r]).tolist())
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and len(G.run_inputs()) == 100
    # the comparison is not one of constant rows: among the 20-car inputs every rejoin position and count of places
    # lost occurs, every driver is the car ahead, and so do "retired" (20 / 21), "in the lead" (20) and "no car" (B = 15)
    assert seen[0] == set(range(21)) and seen[1] >= set(range(19)) | {20} and seen[2] == set(range(22))
    assert 15 in seen[3] and 15 in seen[4] and len(seen[3]) >= 12 and len(seen[4]) >= 12


def test_window_kernel_where_the_grid_slots_decide():
    """Losses at which the rejoin time equals a running car's cumulative time, so that the grid-slot half of the key
    decides the side: no loss at all (cars the model leaves at equal times) and the run's own commonest positive time
    differences.  That such cells exist is asserted from the reference alone, before comparing."""
    tied = {}
    for name in ('X_no_noise', 'X_all_attempt', 'S60', 'N10', 'EVT'):
        case = G.fuzz_cases()[name] if name.startswith('X_') else O.load_case(name)
        seed = case.get('seed', 42)
        n = len(case['grid_probs'])
        ref = RR.traced_run(case, TIE_SIMS, seed, 3)
        tr = ref['trace']
        losses = [0.0] + WR.own_losses(tr['cum'], tr['dnf'])
        cells = [WR.tie_cells(tr['cum'], tr['dnf'], x) for x in losses]
        tied[name] = sum(cells)
        windows = WR.every_driver(n, losses)
        want, _ = _check(name, case, TIE_SIMS, seed, 3, windows, ref=ref)
        assert WR.tie_cells(tr['cum'], tr['dnf'], float(case['config']['pit_loss'])) == 0, name      # (the configured loss ties nowhere)
        # where the reference decides a tie by slot, the car ahead is the one at the rejoin time itself: its gap is 0
        if sum(cells[1:]):
            assert (want[..., 3] == 0).any(), name
    assert tied['X_no_noise'] > 100 and tied['S60'] > 100 and all(v > 0 for v in tied.values()), tied


def _resume_case(name, case, seed, m=RESUME_SIMS, base=40):
    """Simulation i's state after every lap of G.resume_laps, resumed as simulation i: rows k + 1 .. L of the staging are
    the oracle trace's of i, the histogram its finishing order."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    windows = _windows(case, n)[:2 * GROUP + 1]
    ref = RR.traced_run(case, m, seed, base)
    tr = ref['trace']
    want = WR.values_from_times(tr['cum'], tr['dnf'], GR.slots_of(ref['grids']), windows)
    prob = PH.KH.generic_problem(case)
    states = 0
    for i in range(m):
        for k in G.resume_laps(case, seed, base + i):
            st = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k))
            hist, got = PH.window_values(case, 1, seed, sim_offset=base + i, windows=windows, state=st, prob=prob)
            assert got.shape == (1, L - k, len(windows), 5)               # (nothing at all is staged from lap L)
            assert np.array_equal(got[0], want[i, k:]), (name, i, k)
            assert np.array_equal(hist, RR.counts(ref['orders'][i:i + 1], n)), (name, i, k)
            states += 1
    return states


def test_window_kernel_from_a_state_continues_the_oracle_trace():
    done = 0
    for name, case, seed in G.resume_inputs():
        assert _resume_case(name, case, seed) >= RESUME_SIMS
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ


def test_field_sizes_at_the_limits():
    """1, 2, 3, 31 and 32 cars, from the grid and from a state; a field of one always rejoins in the lead with nobody
    behind and loses no place."""
    for n in (1, 2, 3, 31, 32):
        case = RR.field_case(n)
        windows = _windows(case, n)
        ref = RR.traced_run(case, 16, 5)
        _same(n, PH.windows_run(case, 16, 5, windows=windows), WR.window_counts(case, 16, 5, windows=windows, ref=ref))
        k = 12
        st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, 5, 2, k))
        _same((n, 'state'), PH.windows_run(case, 1, 5, sim_offset=2, windows=windows, state=st),
              WR.continued_counts(ref, [2], k, windows))
    one = PH.windows_run(RR.field_case(1), 16, 5, windows=[(0, 21.0)])
    B = len(WR.DEFAULT_EDGES) + 1
    assert (one['rejoin'][:, 0, 0] + one['rejoin'][:, 0, 1] == 16).all()           # in the lead, or out
    assert (one['lost'][:, 0, 0] == one['rejoin'][:, 0, 0]).all() and (one['ahead'][:, 0, 1] == one['rejoin'][:, 0, 0]).all()
    assert (one['gap_ahead'][:, 0, B] == 16).all() and (one['gap_behind'][:, 0, B] == 16).all()


def test_window_counts_around_the_register_group():
    """1 window, one fewer than a group, a group, one more, and the limit with one fewer: the padded last group is
    computed and never written, and window w's values do not depend on the windows beside it."""
    case = O.load_case('S60')
    ref = RR.traced_run(case, 24, 7)
    tr = ref['trace']
    every = WR.every_driver(20, [21.0, 0.5, 11.0, 0.0])[:64]
    full = WR.values_from_times(tr['cum'], tr['dnf'], GR.slots_of(ref['grids']), every)
    for W in (1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP - 1, 2 * GROUP + 1, 63, 64):
        hist, got = PH.window_values(case, 24, 7, windows=every[:W])
        assert got.shape == (24, 60, W, 5) and np.array_equal(got, full[:, :, :W]), W
        assert np.array_equal(hist, ref['hist'])


def test_one_edge_and_sixty_three_edges():
    case = O.load_case('S60')
    ref = RR.traced_run(case, 48, 7)
    fine = tuple(float(x) for x in np.concatenate([np.arange(1, 41) * 0.25, np.arange(1, 24) * 5.0 + 10.0]))
    assert len(fine) == 63 and (np.diff(fine) > 0).all()
    windows = WR.every_driver(20, [21.0])
    for edges in ((4.0,), fine):
        got = PH.windows_run(case, 48, 7, windows=windows, edges=edges)
        _same(len(edges), got, WR.window_counts(case, 48, 7, windows=windows, edges=edges, ref=ref))
        assert got['gap_ahead'].shape[2] == got['gap_behind'].shape[2] == len(edges) + 2
    assert (got['gap_ahead'][29].sum(axis=0) > 0).sum() > 30          # the fine edges spread the gaps over the bins


def test_a_huge_loss_rejoins_last_with_nobody_behind():
    case = O.load_case('S60')
    m = 24
    ref = RR.traced_run(case, m, 7)
    windows = WR.every_driver(20, [1e6])
    got = PH.windows_run(case, m, 7, windows=windows)
    _same('1e6', got, WR.window_counts(case, m, 7, windows=windows, ref=ref))
    B = len(WR.DEFAULT_EDGES) + 1
    running = (ref['trace']['dnf'] == 0).sum(axis=2)                  # [m][L]
    for lap in (1, 30, 60):
        r = running[:, lap - 1]
        sims_with = np.bincount(r[r > 0] - 1, minlength=20)           # [p]: simulations with p + 1 cars running
        for w in range(20):
            out = got['rejoin'][lap - 1, w, 20]
            assert got['gap_behind'][lap - 1, w, B] == m and got['gap_behind'][lap - 1, w, :B].sum() == 0
            assert got['gap_ahead'][lap - 1, w, B - 1] + got['gap_ahead'][lap - 1, w, B] == m        # over 120 s, or none
            assert got['rejoin'][lap - 1, w, :20].sum() == m - out
        # every running car rejoins behind all the others: position p is taken by the p + 1 runners of such a simulation
        assert np.array_equal(got['rejoin'][lap - 1, :, :20].sum(axis=0), sims_with * np.arange(1, 21)), lap
