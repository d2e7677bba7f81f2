"""mcgp_run_combined on the device over the inputs of generic_cases.py and at the limits of include/mcgp.h, through the C
ABI: race_combined_kernel<false / true> at every block shape the inputs' field sizes give, penalties_count, events_count
and paces_count at sizes where their grid-stride loops iterate, and the host side's packing and chunking.  Scenarios come
from combined_cases.py.

References: the Python restatement combined_ref (which shares no code with the kernels); the CPU oracle's finishing
orders and mcgp_run_from_state for the empty scenario; and, for scenarios in which two kinds meet, references that share
nothing with combined_ref either -- the call itself without offsets on a case under another base pace, the sibling calls
mcgp_run_penalties and mcgp_run_events on that case (their kernels have references of their own), the oracle's trace
(penalties_cases.trace_fates, flag_tie; the laps carried of part g).  Every comparison is integer equality, and after
every call mcgp_last_kernel_name is mcgp::race_combined_kernel.  What keeps the comparisons from being vacuous is asserted
from the references alone, before the device's result is looked at (for parts a and b in combined_cases.fuzz_sweep,
whose figures are in combined_cases' docstring).  The oracle's runs of parts a and b are made in a pool of at most 16
threads.

a. From the grid, 8 simulations on the 100 inputs of run_inputs() under the generator's scenarios: orders, fate, events
   and carried are the restatement's, hist and delta the counts of those orders, every row sums to m.
b. From the oracle's state of simulation OFFSET after max(1, L // 2) on the 94 inputs of resume_inputs(), continued as
   simulations 0 .. 7; on the 8 golden and the 12 X_ cases also after laps 1, L - 1 and L.  Accumulated into buffers of
   fives.  Scenario 0 against mcgp_run_from_state.
c. S60, EVT, n32 and n3, from the grid and from a state: scenarios with whole-race LAPS offsets x_d on every driver beside
   plans, penalties and overrides are the same call without offsets under base_pace[d] + x_d, cell for cell; without
   their overrides they are mcgp_run_penalties, without their penalties mcgp_run_events, on that case; overrides equal to
   what a simulation drew change nothing for it beside penalties and offsets.
d. Ties at the flag by construction (penalties_cases.flag_tie on the oracle's trace under the offset pace) on S60 and
   X_no_noise with a whole-race offset on a third driver, 64 calls of one simulation each: the restatement's order, which
   has the tied pair in grid-slot order.
e. 64 scenarios x (32 plans of 8 stops, 256 penalties, 64 overrides, 64 offsets) on 32 cars over 70 laps; a 1000-lap
   race; a one-lap race; penalty seconds of 1e6, 2^-30 and 5e-324 beside offsets of +-3 s: the restatement.
f. Fields of 31 and 3 cars at 1, 63, 65, 129 and 257 simulations under scenario lists with ragged counts, the empty
   tables passed as zero counts and as NULL: the restatement up to 65 simulations, beyond that the counts of the returned
   orders and the sum of split calls.
g. F33, 64 scenarios, two rounds and a ragged third of penalties_count's and events_count's blocks and as many more of
   paces_count's as its one block per (scenario, driver) takes, in one staging chunk: hist and delta against the counts of
   the returned orders, fate and carried against the oracle's trace, all against the sum of split calls, the first 8 ids
   against the restatement.
h. Staging chunks from a state with ev_stage, carried or both NULL: the unchunked call.  One call just past the call's
   own staging budget (64 scenarios x 32 cars x 3 laps, n + 4 + 2n bytes per scenario and simulation, no orders): the sum
   of two single-chunk calls.

Cost: the device calls are milliseconds each, the file's time is the restatement's.  Wall time on an MI355X machine
(256 CUs), in one visit: this file 18.1 s (a 5.6 s, b 2.7 s and 1.4 s for the first and last laps, f 1.9 s, g 1.4 s, the
64 full scenarios 1.2 s) against 28.2 s for tests/test_gpu_stints_moves_fuzz.py, the family's yardstick, which it should
not exceed."""
import functools

import numpy as np
import pytest
import torch        # for _cus(); here and not there: once the library has initialised HIP, loading torch's takes 10 s more

import combined_cases as CC
import combined_host_build as CH
import combined_ref as CR
import events_ref as ER
import generic_cases as G
import oracle_py as O
import paces_ref as PR
import penalties_cases as NC
import penalties_ref as NR
import resume_ref as RR
import strategy_ref as SR
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

SIMS, OFFSET, TIE_SIMS = CC.FUZZ_SIMS, CC.FUZZ_OFFSET, 64
KERNEL = 'mcgp::race_combined_kernel'
COUNT_BLOCK, MAX_SCENARIOS, STAGE_BYTES = 256, 64, 256 << 20
KEYS = ('hist', 'delta', 'fate', 'events', 'carried', 'orders')
COUNTS = KEYS[:-1]
SERVE, FLAG, LAP = CR.SERVE, CR.FLAG, CR.LAP
CORNERS = tuple(G.GOLDEN) + tuple(name for name in G.fuzz_cases() if name.startswith('X_'))
X = [0.37, -0.21, 0.113, -0.57, 0.29, -0.083, 0.61]      # test_gpu_paces' offsets: not round in binary, mixed signs


def _run(case, scen, m, seed, off=0, fill=0, **kw):
    """mcgp_run_combined under scenario() dicts -> dict(hist, delta, fate, events, carried, orders), the counts less
    what the buffers held before the call."""
    rc, *out = CR.run_c(case, scen, m, seed, sim_offset=off, fill=fill, **kw)
    assert rc == 0, N.lib().mcgp_last_error().decode()
    assert N.lib().mcgp_last_kernel_name(0).decode() == KERNEL
    got = dict(zip(KEYS, out))
    for k in COUNTS:
        got[k] = got[k] - fill
    return got


def _same(a, b, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k)


def _sum(a, b):
    return {k: a[k] + b[k] for k in COUNTS}


def _counts_of_orders(got, n, m, what):
    """hist and delta are the counts of the returned orders; every fate, events and carried row sums to m."""
    assert np.array_equal(got['hist'], NR.hist_counts(got['orders'], n)), what
    assert np.array_equal(got['delta'], SR.delta_counts(got['orders'], n)), what
    for k in ('fate', 'events', 'carried'):
        assert (got[k].sum(axis=2) == m).all(), (what, k)


def _against_the_restatement(case, scen, m, seed, off=0, state=None, **kw):
    want = CR.ref_run(case, scen, m, seed, off, state=state)
    got = _run(case, scen, m, seed, off, state=state, **kw)
    CH.check_against(got, case, want, m)
    return want


def _case(name):
    if name[0] == 'n':
        return RR.field_case(int(name[1:])), 5
    if name in G.GOLDEN:
        return O.load_case(name), 42
    case = G.fuzz_cases()[name]
    return case, case['seed']


@functools.lru_cache(maxsize=None)
def _inputs():
    return CC.fuzz_inputs()


# ---------------------------------------------------------------- a. from the grid on every input
def test_from_the_grid_on_every_input(require_gpu):
    def compare(case, seed, scen, want, m, offset, state):
        CH.check_against(_run(case, scen, m, seed, offset), case, want, m)

    CC.fuzz_sweep(*_inputs(), compare)


# ---------------------------------------------------------------- b. from a state on every resume input
def _compare_from_a_state(case, seed, scen, want, m, offset, state):
    """The gains of buffers of fives are the restatement's counts; scenario 0 is mcgp_run_from_state."""
    prob = RR.problem(case)
    got = _run(case, scen, m, seed, offset, state=state, prob=prob, fill=5)
    CH.check_against(got, case, want, m)
    rc, hist, orders = RR.run_c(prob, [state], m, [offset], seed)
    assert rc == 0
    assert np.array_equal(got['orders'][0], orders[0]) and np.array_equal(got['hist'][0], hist[0])


def test_from_a_state_on_every_input(require_gpu):
    CC.fuzz_sweep(*_inputs(), _compare_from_a_state, from_state=True)


def test_from_states_after_the_first_and_the_last_laps(require_gpu):
    """The golden and the X_ cases from the states after laps 1, L - 1 and L (after L: FLAG penalties only, nothing is
    raced)."""
    states = at_the_flag = served = cleared = 0
    for (name, case, seed), ref in zip(*_inputs()):
        if name not in CORNERS:
            continue
        L = case['config']['total_laps']
        for k in sorted({1, max(1, L - 1), L} - {max(1, L // 2)}):
            e = CC.expectation(name, case, seed, ref, k)
            if k == L:
                assert len(e['scen']) == 2 and not any(e['scen'][1][t] for t in ('plans', 'events', 'paces'))
                assert all(kind == FLAG for _, kind, _, _ in e['scen'][1]['penalties'])
                at_the_flag += 1
            served += e['shows']['served']
            cleared += e['shows']['cleared']
            _compare_from_a_state(case, seed, e['scen'], e['want'], SIMS, e['offset'], e['state'])
            states += 1
    # (55 states; X_onelap's only state is part b's)
    assert states >= 50 and at_the_flag == 19 and served >= 15 and cleared >= 15, (states, at_the_flag, served, cleared)


# ---------------------------------------------------------------- c. a second reference for mixed scenarios
def _x(n):
    x = [X[d % 7] + 0.001 * (d // 7) for d in range(n)]
    if n >= 2:
        x[min(2, n - 1)] = 0.0
    return x


@pytest.mark.parametrize('start', ['grid', 'state'])
@pytest.mark.parametrize('name', ['S60', 'EVT', 'n32', 'n3'])
def test_whole_race_offsets_beside_the_other_kinds_are_the_race_under_another_base_pace(require_gpu, name, start):
    """base_pace[d] + x_d formed here is the binary64 addition the kernel makes (the header's identity, which
    test_gpu_paces proves against the oracle for offsets alone).  From a state: the oracle's state under the other base
    pace, continued under the original case with the offsets on every lap left."""
    case, _ = _case(name)
    seed, off, m = 47, 300, 40
    n, L = len(case['grid_probs']), case['config']['total_laps']
    x = _x(n)
    shifted = PR.with_base_pace(case, x)
    if start == 'grid':
        state, first, pace_first = None, 2, 1
    else:
        k = L // 2
        ref = RR.traced_run(shifted, 4, seed, off)
        state, first, pace_first = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, seed, off + 3, k)), k + 1, k + 1
    whole = [PR.laps(d, pace_first, L, x[d]) for d in range(n)]
    bare = [dict(sc, paces=[]) for sc in CR.meeting_scenarios(first, L, n)]
    assert sum(bool(sc['plans']) + bool(sc['penalties']) + bool(sc['events']) >= 2 for sc in bare) >= 4
    offset = [dict(sc, paces=whole) for sc in bare]
    want = _run(shifted, bare, m, seed, off, state=state)
    got = _run(case, offset, m, seed, off, state=state)
    _same(got, want, name)
    assert (got['carried'][:, :, 0] == m).all() and (got['fate'][:, :, 1:] > 0).any()
    assert not np.array_equal(got['orders'], _run(case, bare, m, seed, off, state=state)['orders'])    # the offsets matter
    # without the overrides: mcgp_run_penalties on the shifted case, and mcgp_run_events' counts of the race as drawn
    plans, pens, evs = ([sc[t] for sc in bare] for t in ('plans', 'penalties', 'events'))
    got = _run(case, [dict(sc, events=[]) for sc in offset], m, seed, off, state=state)
    rc, h, dl, ft, o = NR.run_c(shifted, plans, pens, m, seed, sim_offset=off, state=state)
    assert rc == 0
    _same(got, dict(hist=h, delta=dl, fate=ft, orders=o), name, ('hist', 'delta', 'fate', 'orders'))
    rc, _, _, ev, _ = ER.run_c(shifted, plans, [[]] * len(bare), m, seed, sim_offset=off, state=state)
    assert rc == 0 and np.array_equal(got['events'], ev)
    # without the penalties: mcgp_run_events on the shifted case
    got = _run(case, [dict(sc, penalties=[]) for sc in offset], m, seed, off, state=state)
    rc, h, dl, ev, o = ER.run_c(shifted, plans, evs, m, seed, sim_offset=off, state=state)
    assert rc == 0
    _same(got, dict(hist=h, delta=dl, events=ev, orders=o), name, ('hist', 'delta', 'events', 'orders'))
    assert (got['fate'][:, :, 0] == m).all()


def test_overrides_equal_to_what_a_simulation_drew_change_nothing_beside_penalties_and_offsets(require_gpu):
    case, _ = _case('EVT')
    seed, off = 47, 300
    n, L = len(case['grid_probs']), case['config']['total_laps']
    z = n - 1
    sc = CR.scenario({0: (-1, 0, [(L // 2, 2)])},
                     [(0, SERVE, L // 2 - 1, 5.0), (z, SERVE, 2, 10.0), (z, FLAG, 0, 3.0), (1, LAP, L // 2, 2.0), (z, LAP, L // 2, 1.5)],
                     [], [PR.laps(z, 1, L, 0.25), PR.until_stop(z, 2, 0.35), PR.until_stop(0, L // 2 - 1, 0.2)])
    kinds = set()
    for i in (0, 7, 39):
        evs = [(lap, lap, ER.drawn_event(case, seed, off + i, lap)[0]) for lap in range(2, L + 1)]
        kinds |= {kind for _, _, kind in evs}
        got = _run(case, [sc, dict(sc, events=evs)], 1, seed, off + i)
        for k in KEYS:
            assert np.array_equal(got[k][0], got[k][1]) or k == 'delta', (i, k)
        assert not got['delta'][1, :, :n - 1].any() and not got['delta'][1, :, n:].any()
    assert len(kinds) >= 2


# ---------------------------------------------------------------- d. ties at the flag under offsets
@pytest.mark.parametrize('name', ['S60', 'X_no_noise'])
def test_ties_at_the_flag_under_offsets(require_gpu, name):
    """An AT_FLAG penalty of exactly t_b - t_a on the winner a of the oracle's race under base_pace[c] + x, run with a
    whole-race LAPS offset of x on c, a third driver: the tied pair is ordered by grid slot."""
    case, seed = _case(name)
    n, L = len(case['grid_probs']), case['config']['total_laps']
    c, x = n // 2, X[0]
    ref = RR.traced_run(PR.with_base_pace(case, [x * (d == c) for d in range(n)]), TIE_SIMS, seed, OFFSET)
    offs = [PR.laps(c, 1, L, x)]
    ties, flips = [], 0
    for i in range(TIE_SIMS):
        tie = NC.flag_tie(ref, i)
        if tie is None or c in tie[:2]:
            continue
        a, b, delta, flip = tie
        end = ref['trace']['cum'][i, -1]
        if ((end == end[b]) & (ref['trace']['dnf'][i, -1] == 0)).sum() > 1:
            continue                                        # (a third car at b's time: X_no_noise has such)
        pens = [(a, FLAG, 0, delta)]
        want = CR.orders(case, 1, seed, OFFSET + i, penalties=pens, offsets=offs, grids=ref['grids'][i:i + 1])[0][0]
        assert tuple(want[:2]) == ((b, a) if flip else (a, b)), i
        ties.append((i, pens, want))
        flips += flip
    assert len(ties) >= 40 and flips >= 10 and len(ties) - flips >= 10, (len(ties), flips)
    prob = RR.problem(case)
    for i, pens, want in ties:
        got = _run(case, [CR.scenario(penalties=pens, paces=offs)], 1, seed, OFFSET + i, prob=prob)
        assert np.array_equal(got['orders'][0, 0], want), (name, i, got['orders'][0, 0][:3], want[:3])
        assert np.array_equal(got['hist'][0], RR.counts(got['orders'][0], n))


# ---------------------------------------------------------------- e. the limits together
def _full_scenario(s, n, L):
    """32 plans of 8 stops, 256 penalties (a serve and a flag penalty on every driver, four laps with an addition on all 32
    drivers, 32 laps with one on driver 31 and one more), 64 single-lap overrides and 64 offsets (an UNTIL_STOP offset and a
    LAPS range on every driver); everything rotates with s."""
    plans = {d: (-1, 0, [(2 + (d + s) % 5 + 8 * j, (d + s + j) % 3) for j in range(8)]) for d in range(n)}
    pens = [(d, SERVE, 2 + (d + 2 * s) % (L - 1), 5.0 + d / 8 + s / 1024) for d in range(n)]
    pens += [(d, FLAG, 0, 1.0 + ((d + s) % n) / 16) for d in range(n)]
    sec = lambda lap, d: 0.25 + (lap * 32 + (d + s) % 32) / 4096
    full = [2 + (s + 17 * j) % (L - 1) for j in range(4)]
    rest = [lap for lap in range(2, L + 1) if lap not in full][:32]
    for lap in full:
        pens += [(d, LAP, lap, sec(lap, d)) for d in range(n)]
    for lap in rest:
        pens += [(d, LAP, lap, sec(lap, d)) for d in (31, (lap + s) % 31)]
    evs = [(lap, lap, (lap + s) % 4) for lap in range(2, L + 1) if (lap + s) % (L - 1) >= 5]
    offs = [PR.until_stop(d, 1 + (3 * d + s) % L, 0.05 * ((d + s) % 9 + 1)) for d in range(n)]
    offs += [PR.laps(d, 1 + (d + s) % 30, 31 + (5 * d + s) % 40, 0.05 * ((d + 2 * s) % 9 - 4)) for d in range(n)]
    return CR.scenario(plans, pens, evs, offs)


def test_sixty_four_scenarios_at_every_table_s_limit(require_gpu):
    n, m, seed = 32, 2, 13
    case = RR.field_case(n)
    case['config'] = dict(case['config'], total_laps=70)
    L = 70
    scen = [_full_scenario(s, n, L) for s in range(MAX_SCENARIOS)]
    for sc in scen:
        assert len(sc['plans']) == 32 and all(len(p[2]) == 8 and p[2][-1][0] <= L for p in sc['plans'].values())
        assert len(sc['penalties']) == 256 and len({(d, k, lap) for d, k, lap, _ in sc['penalties']}) == 256
        assert len(sc['events']) == 64 and len(sc['paces']) == 64
        assert sum(sum(1 for _, k, l, _ in sc['penalties'] if k == LAP and l == lap) == 32 for lap in range(2, L + 1)) == 4
    assert scen[0] != scen[1] and scen[0] != scen[32]
    o, f, e, c = _against_the_restatement(case, scen, m, seed)
    assert (f == CR.FATE_SERVED).any() and (c > 0).any() and len({x.tobytes() for x in o}) > 32


def test_a_thousand_laps(require_gpu):
    """MCGP_MAX_LAPS: a serve penalty pending from lap 1000, served at a planned stop on lap 1000 or added at the flag; an
    UNTIL_STOP offset from lap 1 under a plan without stops, carried 1000 laps (column L); a forced event on lap 1000."""
    case = RR.field_case(2)
    case['config'] = dict(case['config'], total_laps=1000, dnf_rates={t: 0.0 for t in case['config']['dnf_rates']})
    case['driver_dnf_rates'] = {d: 0.0 for d in case['driver_dnf_rates']}       # both cars see the flag
    m, seed, L = 2, 47, 1000
    scen = [CR.scenario(),
            CR.scenario({0: (-1, 0, [(L, 1)]), 1: (-1, 0, [])}, [(0, SERVE, L, 5.0), (1, LAP, L, 2.5)], [(L, L, CR.SC)],
                        [PR.until_stop(1, 1, 0.4), PR.until_stop(0, L, -0.3)]),
            CR.scenario({1: (-1, 0, [])}, [(1, SERVE, L, 10.0), (0, FLAG, 0, 1.0)], [(L, L, CR.RED), (2, 999, CR.NONE)],
                        [PR.until_stop(1, 1, 0.1), PR.laps(0, 1, L, 0.25)])]
    o, f, e, c = _against_the_restatement(case, scen, m, seed, 1)
    assert (f[1][:, 0] == CR.FATE_SERVED).all() and (f[2][:, 1] == CR.FATE_FLAG).all()
    assert (c[1][:, 1] == L).all() and (c[1][:, 0] == 1).all() and (c[2][:, 1] == L).all()
    assert (e[1][:, 1] >= 1).all() and (e[2] == [1, 0, 0]).all()
    got = _run(case, scen, m, seed, 1)
    assert got['carried'][1, 1, L] == m and got['events'][2, 0, 1] == m        # c = L lands in column L


def test_a_race_of_one_lap(require_gpu):
    name, m = 'n3', 40
    case, seed = _case(name)
    case['config'] = dict(case['config'], total_laps=1)
    scen = CC.scenarios(name, case, 2, 1)
    assert len(scen) == 2 and scen[1]['paces'] and scen[1]['penalties'] and not scen[1]['plans'] and not scen[1]['events']
    o, f, e, c = _against_the_restatement(case, scen, m, seed, 5)
    assert not np.array_equal(o[1], o[0]) and not e.any() and not f.any() and set(np.unique(c)) <= {0, 1}


def test_seconds_at_both_ends_of_the_range(require_gpu):
    """1e6, 2^-30 and 5e-324 s as a serve, a flag and a lap penalty of one driver beside offsets of +-3 s a lap: the last
    is absorbed by every time it is added to, so its orders are those under the offsets alone."""
    case, seed = _case('S60')
    m, d = 32, 3
    L = case['config']['total_laps']
    offs = [PR.laps(d, 1, L, 3.0), PR.laps(5, 1, L, -3.0), PR.until_stop(7, 4, 3.0), PR.until_stop(d, 6, -3.0)]
    scen = [CR.scenario(), CR.scenario(paces=offs)]
    scen += [CR.scenario(penalties=[(d, SERVE, 10, sec), (d, FLAG, 0, sec), (d, LAP, L // 2, sec)], paces=offs)
             for sec in (1e6, 2.0 ** -30, 5e-324)]
    o, f, e, c = _against_the_restatement(case, scen, m, seed)
    assert np.array_equal(o[4], o[1]) and (o[2] != o[1]).any() and (o[1] != o[0]).any()
    assert np.array_equal(f[4], f[2]) and (f[4][:, d] == CR.FATE_SERVED).any() and (f[4][:, d] != CR.FATE_NONE).all()
    assert np.array_equal(c[4], c[1]) and c[1][:, d].any() and c[1][:, 7].any()


# ---------------------------------------------------------------- f. ragged sizes
@pytest.mark.parametrize('n', [31, 3])
def test_ragged_counts(require_gpu, n):
    """Simulation counts one short of, one past and far from a wave, two waves and a counting block, under a list whose
    scenarios have tables of different lengths, some empty; then a list in which two tables are empty everywhere, passed
    as zero counts and as NULL."""
    name = f'n{n}'
    case, seed = _case(name)
    L = case['config']['total_laps']
    full = CC.scenarios(name, case, 2, 1)
    assert len(full) == 4
    scen = full + [CR.scenario(penalties=full[1]['penalties']), CR.scenario(events=full[1]['events']),
                   CR.scenario(full[2]['plans'], paces=full[2]['paces'])]
    assert sorted({len(sc[t]) for sc in scen for t in ('penalties', 'events', 'paces')})[0] == 0
    assert all(len({len(sc[t]) for sc in scen}) >= 3 for t in ('penalties', 'events', 'paces'))
    lone = [CR.scenario(), CR.scenario(full[2]['plans'], penalties=full[2]['penalties']), CR.scenario()]
    grids = RR.traced_run(case, 65, seed, OFFSET)['grids']
    want = {id(sl): CR.ref_run(case, sl, 65, seed, OFFSET, grids=grids) for sl in (scen, lone)}     # made once, cut to m
    for m in (1, 63, 65, 129, 257):
        got = _run(case, scen, m, seed, OFFSET)
        _counts_of_orders(got, n, m, (n, m))
        if m <= 65:
            CH.check_against(got, case, tuple(w[:, :m] for w in want[id(scen)]), m)
        else:
            a = m // 2 + 1
            lo, hi = _run(case, scen, a, seed, OFFSET), _run(case, scen, m - a, seed, OFFSET + a)
            _same(got, _sum(lo, hi), (n, m), COUNTS)
            assert np.array_equal(got['orders'], np.concatenate([lo['orders'], hi['orders']], axis=1))
        zero = _run(case, lone, m, seed, OFFSET, null_counts=False)
        null = _run(case, lone, m, seed, OFFSET, null_counts=True)
        _same(zero, null, (n, m, 'NULL'))
        _counts_of_orders(null, n, m, (n, m, 'NULL'))
        assert (null['carried'][:, :, 0] == m).all() and np.array_equal(null['orders'][0], got['orders'][0])
        if m <= 65:
            CH.check_against(null, case, tuple(w[:, :m] for w in want[id(lone)]), m)


# ---------------------------------------------------------------- g. counting loops past two rounds
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _f33_scenarios(n, L):
    """Scenario 0 empty; odd: flag penalties, LAPS offsets and single-lap overrides; even: planned stops on lap 5 for half
    the field (in nine laps the rule stops on lap 3 or never, and the forced event comes after it), a serve penalty and an
    UNTIL_STOP offset on every driver from laps on both sides of the stop, lap additions on lap 5, a forced safety car on
    it."""
    scen = [CR.scenario()]
    for s in range(1, MAX_SCENARIOS):
        if s % 2:
            pens = [(d, FLAG, 0, NC.SECONDS[(d + s) % 4] + 0.125 * ((d * s) % 8)) for d in range(n) if (d + s) % 3]
            offs = [PR.laps(d, 1 + (d + s) % L, L, 0.1 * ((d + s) % 7 - 3)) for d in range(n) if (d + s) % 4]
            scen.append(CR.scenario({}, pens, [(2 + s % (L - 1), 2 + s % (L - 1), 1 + s % 3)], offs))
        else:
            plans = {d: (-1, 0, [(5, G.MEDIUM)]) for d in range(n) if (d + s // 2) % 2 == 0}
            pens = [(d, SERVE, 2 + (d + s) % 8, 5.0 + 0.25 * d) for d in range(n)]
            pens += [(d, LAP, 5, 0.5 + 0.125 * d) for d in range(n) if (d + s) % 5 < 3]
            offs = [PR.until_stop(d, 1 + (d + s // 2) % L, 0.1 * ((d + s) % 5 + 1)) for d in range(n)]
            scen.append(CR.scenario(plans, pens, [(5, 5, CR.SC)], offs))
    return scen


def _trace_carried(ref, offsets, plans, L):
    """laps carried [m][n] of a scenario from the grid, from the oracle's trace of the same simulations alone: as
    penalties_cases.trace_fates reads the fate of a serve penalty (retirement laps are shared by all scenarios; a planned
    car stops on its planned laps, any other where the trace has it running on tyres of age 0 after a lap >= 2), for a
    scenario whose overrides move no rule stop."""
    tr = ref['trace']
    run, age = tr['dnf'] == 0, tr['age']
    out_lap = np.where(tr['dnf'][:, L - 1, :] != 0, tr['dnf_lap'][:, L - 1, :], 0)         # [m][n], 0: runs to the flag
    carried = np.zeros(out_lap.shape, np.int64)
    for d, kind, p, _, _ in offsets:
        if kind != PR.UNTIL_STOP:
            continue
        r = out_lap[:, d]
        if d in plans:
            stops = [lap for lap, _ in plans[d][2] if lap >= p]
            q = np.full(len(r), stops[0] if stops else 0)
            stopped = run[:, stops[0] - 1, d] if stops else np.zeros(len(r), bool)
        else:
            hit = run[:, :, d] & (age[:, :, d] == 0)
            hit[:, :max(p, 2) - 1] = False
            stopped, q = hit.any(axis=1), hit.argmax(axis=1) + 1
        carried[:, d] = np.where(stopped, q - p + 1, np.where(r != 0, np.maximum(r - p, 0), L - p + 1))
    return carried


def test_counting_loops_past_two_rounds(require_gpu):
    """penalties_count and events_count launch min(tiles, max(1, 8 CUs / S)) blocks of 256 per scenario, paces_count
    min(tiles, max(1, 8 CUs / (S (1 + n)))) per scenario and driver (the rules restated here, not read back): F33 under 64
    scenarios at two full passes of the first two's blocks and a ragged third, in one staging chunk of n + 4 + 2n bytes per
    scenario and simulation."""
    case, seed = _case('F33')
    n, L, S = len(case['grid_probs']), case['config']['total_laps'], MAX_SCENARIOS
    assert (n, L) == (20, 9)
    one_round = max(1, 8 * _cus() // S) * COUNT_BLOCK
    paces_round = max(1, 8 * _cus() // (S * (1 + n))) * COUNT_BLOCK
    m = 2 * one_round + 77
    assert m > 2 * one_round >= 2 * paces_round and m % COUNT_BLOCK and m % 64
    assert m < STAGE_BYTES // (S * (3 * n + 4)) // 256 * 256
    scen = _f33_scenarios(n, L)
    ref = RR.traced_run(case, m, seed, OFFSET)
    fates = np.stack([NC.trace_fates(ref, sc['penalties'], sc['plans']) for sc in scen])
    laps = np.stack([_trace_carried(ref, sc['paces'], sc['plans'], L) for sc in scen])
    want_fate, want_carried = NR.fate_counts(fates, n), PR.carried_counts(laps, L)
    assert all((want_fate[2::2, :, f] > 0).any() for f in (1, 2, 3)) and (want_carried[2::2, :, 1:] > 0).sum() > 500
    got = _run(case, scen, m, seed, OFFSET)
    assert np.array_equal(got['orders'][0], ref['orders'])
    _counts_of_orders(got, n, m, 'F33')
    assert np.array_equal(got['fate'], want_fate) and np.array_equal(got['carried'], want_carried)
    assert (got['events'][2::2, 1, 0] == 0).all() and all(got['events'][s, s % 3, 0] == 0 for s in range(1, S, 2))
    a = one_round + 31
    lo, hi = _run(case, scen, a, seed, OFFSET, orders=False), _run(case, scen, m - a, seed, OFFSET + a, orders=False)
    _same(got, _sum(lo, hi), 'F33 split', COUNTS)
    first = _run(case, scen, 8, seed, OFFSET)
    assert np.array_equal(first['orders'], got['orders'][:, :8])
    CH.check_against(first, case, CR.ref_run(case, scen, 8, seed, OFFSET, grids=ref['grids'][:8]), 8)


# ---------------------------------------------------------------- h. chunks
def test_chunks_from_a_state_with_a_staging_buffer_missing(require_gpu, monkeypatch):
    """ev_stage is NULL without events_out, carried without carried_out: 200 simulations under a cap of 64 per launch are
    four chunks with a short last one."""
    name = 'S60'
    case, seed = _case(name)
    n, L, m = len(case['grid_probs']), case['config']['total_laps'], 200
    k = L // 2
    state = CC.state_after(case, seed, RR.traced_run(case, 1, seed, OFFSET), k)
    scen = CC.scenarios(name, case, k + 1, k + 1, True)
    assert len(scen) == 4
    whole = _run(case, scen, m, seed, 5, state=state)
    _counts_of_orders(whole, n, m, name)
    assert (whole['fate'][:, :, 1:] > 0).any() and (whole['carried'][:, :, 1:] > 0).any() and (whole['events'][:, :, 1:] > 0).any()
    subsets = [dict(events=False), dict(carried=False), dict(events=False, carried=False, delta=False),
               dict(events=False, fate=False, orders=False), dict(carried=False, delta=False, fate=False, orders=False),
               dict(delta=False, fate=False, events=False, carried=False, orders=False)]
    monkeypatch.setenv('MCGP_MAX_SIMS_PER_LAUNCH', '64')
    chunked = [_run(case, scen, m, seed, 5, state=state, **kw) for kw in subsets]
    monkeypatch.delenv('MCGP_MAX_SIMS_PER_LAUNCH')
    for kw, got in zip(subsets, chunked):
        for key in KEYS:
            if kw.get(key, True):
                assert np.array_equal(got[key], whole[key]), (kw, key)
            else:
                assert got[key] is None or not got[key].any(), (kw, key)


def test_a_call_just_past_its_staging_budget(require_gpu):
    """64 scenarios of 32 cars with events_out and carried_out wanted stage 64 (n + 4 + 2n) = 6400 bytes per simulation
    (include/mcgp.h), so a chunk of the 256 MiB budget holds 41 943 simulations, in whole blocks of 256 41 728."""
    n, S, seed = 32, MAX_SCENARIOS, 9
    case = RR.field_case(n)
    case['config'] = dict(case['config'], total_laps=3)
    chunk = STAGE_BYTES // (S * (n + 4 + 2 * n)) // 256 * 256
    assert chunk == 41728
    m = chunk + 77
    scen = [CR.scenario()]
    for s in range(1, S):
        d = s % n
        scen.append(CR.scenario({d: (-1, 0, [(2 + s % 2, s % 3)])}, [(d, SERVE, 2, 5.0), ((d + 1) % n, FLAG, 0, 3.0), ((d + 2) % n, LAP, 3, 2.0)],
                                [(2 + s % 2, 2 + s % 2, 1 + s % 3)], [PR.until_stop(d, 1 + s % 3, 0.3), PR.laps((d + 3) % n, 1, 3, -0.4)]))
    one = _run(case, scen, m, seed, 3, orders=False)
    lo, hi = _run(case, scen, chunk, seed, 3, orders=False), _run(case, scen, m - chunk, seed, 3 + chunk, orders=False)
    _same(one, _sum(lo, hi), 'budget', COUNTS)
    for k in ('fate', 'events', 'carried'):
        assert (one[k].sum(axis=2) == m).all(), k
    assert (one['hist'].sum(axis=2) == m).all() and (one['fate'][1:, :, 1:] > 0).any() and (one['carried'][1:, :, 1:] > 0).any()
