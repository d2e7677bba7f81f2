"""race_gaps_kernel<false> and <true> (csrc/gaps.hip.h) compiled for the host (tools/emu/emu_generic.cpp) and compared,
integers only, with references that do not share its code: the raw staging, decoded by the layout documented at the top
of gaps.hip.h, against gaps_ref's numpy restatement over the CPU oracle's per-lap trace; the histogram against the
oracle's.  Inputs (generic_cases.py): the 8 golden cases, the 84 fuzz configurations, two fields with tiny lap times,
synthetic fields of 1, 2, 3, 19, 31 and 32 cars, a 1000-lap race; all of them a second time at edges and pairs taken
from the oracle's own trace: gaps it shows as edges, the next doubles above them, and pairs it shows tied.  The counting
kernel and the host-side chunking are compared on the device (test_gpu_gaps.py, test_gpu_gaps_conditions_fuzz.py).  The
host build is test infrastructure: nothing under monte_carlo_gp_amd/ can reach it and the product has no CPU path."""
import copy

import numpy as np

import gaps_host_build as GH
import gaps_ref as GR
import generic_cases as G
import oracle_py as O
import resume_ref as RR

RUN_SIMS, RESUME_SIMS, OWN_SIMS = 32, 8, 48
KEYS = ('hist', 'lap_gap', 'lead', 'pair')


_pairs = GR.few_pairs


def _same(name, got, ref):
    for key in KEYS:
        assert np.array_equal(got[key], ref[key]), (name, key)


def test_gaps_kernel_from_the_grid_equals_the_restated_counts():
    done, filled = 0, 0
    for name, case, seed in G.run_inputs():
        n = len(case['grid_probs'])
        pairs = _pairs(n)
        ref = RR.traced_run(case, RUN_SIMS, seed, 3)
        tr = ref['trace']
        want = GR.values_from_times(tr['cum'], tr['dnf'], GR.slots_of(ref['grids']), pairs=pairs)
        hist, got = GH.gaps_values(case, RUN_SIMS, seed, sim_offset=3, pairs=pairs)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f'{name}: {len(bad)} staged values differ, first (simulation, lap - 1, row) {bad[:3].tolist()}'
        assert np.array_equal(hist, ref['hist']), name
        _same(name, GH.gaps(case, RUN_SIMS, seed, sim_offset=3, pairs=pairs),
              GR.gap_counts(case, RUN_SIMS, seed, 3, pairs=pairs, ref=ref))
        filled += len(np.unique(want[:, :, :n]))
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and len(G.run_inputs()) == 100
    assert filled > 100 * 8            # (the comparison is not one of constant rows)


def _own(args):
    """One input's traced run, the call it decides (gaps_ref.own_call) and the reference's staged values at the own edges
    and at the next doubles above them."""
    name, case, seed = args
    ref = RR.traced_run(case, OWN_SIMS, seed, 3)
    call = GR.own_call(ref)
    tr, slot = ref['trace'], GR.slots_of(ref['grids'])
    want = [GR.values_from_times(tr['cum'], tr['dnf'], slot, edges=e, pairs=call['pairs']) for e in (call['edges'], call['up'])]
    return ref, call, want


def test_gaps_kernel_at_the_oracles_own_gaps_and_ties():
    """Every input at edges that are gaps the oracle's trace shows (63 of them, at evenly spaced ranks of the distinct
    positive ones) and at the next double above each, with the pairs the trace shows at equal cumulative times: a time
    off by an ulp, `<` for `<=` in the bin, or a tie decided otherwise than by grid slot moves a staged value here on
    nearly every input.  (At the default edges and four fixed pairs above, `<` for `<=` shows on 31 inputs -- the model
    does produce gaps equal to a default edge --, a reversed slot comparison on 5; here on 98 and on 31.)  What makes
    that so is asserted from the reference alone."""
    inputs = G.run_inputs()
    full, tied, done = 0, set(), 0
    for name, case, seed in inputs:
        ref, call, (want, want_up) = _own((name, case, seed))
        n = len(case['grid_probs'])
        if call['own']:
            moved = int((want != want_up).sum())
            assert moved >= len(call['edges']), (name, moved)         # every edge decides a cell of the reference
        else:
            assert name in ('X_all_out_lap1', 'n1'), name              # no positive gap: nobody runs, or one car
        full += call['own'] and len(call['edges']) == 63
        if call['cells']:
            tied.add(name)
            a, b = call['pairs'][0]
            assert call['pairs'][1] == (b, a)
        for edges, ref_vals in ((call['edges'], want), (call['up'], want_up)):
            hist, got = GH.gaps_values(case, OWN_SIMS, seed, sim_offset=3, edges=edges, pairs=call['pairs'])
            bad = np.argwhere(got != ref_vals)
            assert bad.size == 0, f'{name}: {len(bad)} staged values differ, first (simulation, lap - 1, row) ' \
                                  f'{bad[:3].tolist()} of {n} drivers, 1 lead, pairs {call["pairs"][:4]}'
            assert np.array_equal(hist, ref['hist']), name
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and len(inputs) == 100
    assert full >= 98, full
    assert len(tied) >= 25 and {'X_no_noise', 'X_all_attempt'} <= tied, sorted(tied)


def _resume_case(name, case, seed, m=RESUME_SIMS, base=40):
    """Simulation i's state after every lap of G.resume_laps, resumed as simulation i: rows k + 1 .. L of the staging are
    the oracle trace's of i, the histogram its finishing order.  Returns (states, those with drs_disabled_until > 0)."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    pairs = _pairs(n)
    ref = RR.traced_run(case, m, seed, base)
    tr = ref['trace']
    want = GR.values_from_times(tr['cum'], tr['dnf'], GR.slots_of(ref['grids']), pairs=pairs)
    prob = GH.KH.generic_problem(case)
    states = with_dd = 0
    for i in range(m):
        for k in G.resume_laps(case, seed, base + i):
            dd = RR.drs_disabled_until(case, seed, base + i, k)
            st = (RR.state_arrays(ref, i, k), k, dd)
            hist, got = GH.gaps_values(case, 1, seed, sim_offset=base + i, pairs=pairs, state=st, prob=prob)
            assert got.shape == (1, L - k, n + 1 + len(pairs))
            assert np.array_equal(got[0], want[i, k:]), (name, i, k)
            assert np.array_equal(hist, RR.counts(ref['orders'][i:i + 1], n)), (name, i, k)
            states += 1
            with_dd += dd > 0
    return states, with_dd


def test_gaps_kernel_from_a_state_continues_the_oracle_trace():
    done = 0
    for name, case, seed in G.resume_inputs():
        states, with_dd = _resume_case(name, case, seed)
        assert states >= RESUME_SIMS
        if name in G.GOLDEN:
            assert with_dd > 0, name           # a state whose DRS is still off after an event, in every golden case
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ


def test_field_sizes_at_the_limits():
    """1, 2, 3, 31 and 32 cars, from the grid and from a state; a field of one has no second car and no pair."""
    for n in (1, 2, 3, 31, 32):
        case = RR.field_case(n)
        pairs = _pairs(n)
        ref = RR.traced_run(case, 16, 5)
        _same(n, GH.gaps(case, 16, 5, pairs=pairs), GR.gap_counts(case, 16, 5, pairs=pairs, ref=ref))
        k = 12
        st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, 5, 2, k))
        _same((n, 'state'), GH.gaps(case, 1, 5, sim_offset=2, pairs=pairs, state=st),
              GR.continued_counts(ref, [2], k, pairs=pairs))
    one = GH.gaps(RR.field_case(1), 16, 5)
    B = len(GR.DEFAULT_EDGES) + 1
    assert (one['lead'][:, B] == 16).all() and not one['lead'][:, :B].any()
    assert (one['lap_gap'][:, 0, 0] + one['lap_gap'][:, 0, B] == 16).all()        # leading, or out


def _thousand_laps(dnf=0.002):
    case = copy.deepcopy(O.load_case('N10'))
    case['config']['total_laps'] = 1000
    case['driver_dnf_rates'] = {d: dnf for d in case['base_pace']}            # 0.002: most cars out somewhere in 1000 laps
    return case


def test_a_thousand_lap_race():
    """MCGP_MAX_LAPS: 1000 (n + 1 + P) staging rows, from the grid and from lap 999 and lap 1000."""
    case = _thousand_laps()
    pairs = [(0, 1), (9, 0)]
    ref = RR.traced_run(case, 6, 3)
    got = GH.gaps(case, 6, 3, pairs=pairs)
    _same('L1000', got, GR.gap_counts(case, 6, 3, pairs=pairs, ref=ref))
    assert got['lap_gap'].shape == (1000, 10, 16) and got['pair'].shape == (1000, 2, 31)
    for k in (999, 1000):
        st = (RR.state_arrays(ref, 1, k), k, RR.drs_disabled_until(case, 3, 1, k))
        _same(('L1000', k), GH.gaps(case, 1, 3, sim_offset=1, pairs=pairs, state=st),
              GR.continued_counts(ref, [1], k, pairs=pairs))


def test_one_edge_and_sixty_three_edges():
    case = O.load_case('S60')
    ref = RR.traced_run(case, 48, 7)
    fine = tuple(float(x) for x in np.concatenate([np.arange(1, 41) * 0.25, np.arange(1, 24) * 5.0 + 10.0]))
    assert len(fine) == 63 and (np.diff(fine) > 0).all()
    for edges in ((4.0,), fine):
        pairs = [(0, 1), (1, 0)]
        got = GH.gaps(case, 48, 7, edges=edges, pairs=pairs)
        _same(len(edges), got, GR.gap_counts(case, 48, 7, edges=edges, pairs=pairs, ref=ref))
        assert got['pair'].shape[2] == 2 * (len(edges) + 1) + 1
    assert (got['lap_gap'][59].sum(axis=0) > 0).sum() > 40            # the fine edges spread the finishers over the bins


def test_no_pair_and_sixty_four_pairs():
    case = O.load_case('S60')
    ref = RR.traced_run(case, 32, 7)
    none = GH.gaps(case, 32, 7)
    _same('P0', none, GR.gap_counts(case, 32, 7, ref=ref))
    assert none['pair'].shape == (60, 0, 31)
    pairs = [(a, b) for a in range(8) for b in range(8) if a < b] + [(b, a) for a in range(8) for b in range(8) if a < b]
    pairs += [(19, 0), (0, 19), (18, 19), (19, 18), (10, 12), (12, 10), (5, 15), (15, 5)]
    assert len(pairs) == 64 and len(set(pairs)) == 64
    got = GH.gaps(case, 32, 7, pairs=pairs)
    _same('P64', got, GR.gap_counts(case, 32, 7, pairs=pairs, ref=ref))
    B = len(GR.DEFAULT_EDGES) + 1
    for p, (a, b) in enumerate(pairs):                                # (a, b) and (b, a) mirror each other
        q = pairs.index((b, a))
        assert np.array_equal(got['pair'][:, p, :B], got['pair'][:, q, B:2 * B])
        assert np.array_equal(got['pair'][:, p, 2 * B], got['pair'][:, q, 2 * B])


def test_a_value_equal_to_an_edge_goes_up():
    """The edge rule, decided from the reference alone: a gap g that the oracle's trace shows for some (simulation, lap,
    driver), taken as an edge, puts that cell in the upper bin (edge <= g); the next double above g as the edge puts it
    in the lower one -- in the reference and in the host build alike."""
    case = O.load_case('S60')
    m, seed = 16, 7
    ref = RR.traced_run(case, m, seed)
    tr = ref['trace']
    i, k = 5, 30                                      # simulation 5 after lap 31
    running = np.nonzero(tr['dnf'][i, k] == 0)[0]
    t = tr['cum'][i, k]
    order = running[np.argsort(t[running], kind='stable')]
    leader, d = order[0], order[3]
    g = float(t[d] - t[leader])
    assert g > 0
    up = np.nextafter(g, np.inf)
    slot = GR.slots_of(ref['grids'])
    for edges, want_bin in (((g,), 1), ((up,), 0), ((g / 2, g, 2 * g), 2), ((g / 2, up, 2 * g), 1)):
        want = GR.values_from_times(tr['cum'], tr['dnf'], slot, edges=edges)
        assert want[i, k, d] == want_bin
        hist, got = GH.gaps_values(case, m, seed, edges=edges)
        assert got[i, k, d] == want_bin and np.array_equal(got, want)
