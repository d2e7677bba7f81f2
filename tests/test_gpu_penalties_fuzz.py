"""mcgp_run_penalties on the device over the inputs of generic_cases.py and at the limits of include/mcgp.h, through the
C ABI: race_penalties_kernel<false / true> at every block shape the inputs' field sizes give, penalties_count at sizes
where its grid-stride loop iterates, and the host side's packing and chunking.  Scenarios come from penalties_cases.py.

References, none of which shares code with the kernels: the Python restatement penalties_ref.orders; the CPU oracle's
finishing orders for a scenario without penalties; and two readings of the oracle's per-lap trace that share nothing
with the restatement either -- penalties_cases.trace_fates (reference 1: the fate of every serve penalty) and
penalties_cases.flag_orders (reference 2: the orders under flag penalties only).  Every comparison is integer equality,
and after every call mcgp_last_kernel_name is mcgp::race_penalties_kernel.  What keeps the comparisons from being vacuous
is asserted from the references alone, before the device's result is looked at.  The oracle's runs of parts a and b are
made in a pool of at most 16 threads.

a. From the grid, SIMS = 16 simulations on the 100 inputs of run_inputs() under the generator's scenarios (empty,
   sparse, dense, and with L >= 8 dense beside plans; a one-lap race: flag penalties only): orders and fate counts are
   the restatement's, hist and delta the counts of those orders, scenario 0 is mcgp_run, every fate row sums to m.  The
   restatement is itself checked against references 1 and 2 on every input (penalties_cases.grid_expectation).
b. From the oracle's state of simulation OFFSET after max(1, L // 2) on the 94 inputs of resume_inputs(), continued as
   simulations 0 .. STATE_SIMS - 1 (8); on the 8 golden and the 12 X_ cases also after laps 1, L - 1 and L (after L:
   flag penalties only, nothing is raced): 149 states, 20 of them after lap L.  Accumulated into buffers of fives.
   Penalised scenarios against the restatement, scenario 0 against mcgp_run_from_state.
c. Ties at the flag by construction (penalties_cases.flag_tie) on S60 and X_no_noise, 64 simulations each, one call of
   one simulation each: the order is the restatement's, which is reference 2's.
d. F33, 64 scenarios, two rounds and a ragged third of penalties_count's blocks (16 461 simulations on 256 CUs), in one
   staging chunk: the oracle, reference 2 and reference 1.
e. Fields of 31 and 3 cars at 1, 63, 65, 129 and 257 simulations: references 1 and 2, the restatement up to 65.
f. 64 scenarios x 256 penalties x 32 plans; a 1000-lap race; seconds of 1e6, 2^-30 and 5e-324: the restatement.
g. Staging chunks from a state: the unchunked call.

The references show, at these parameters: 7 inputs on which nothing bites (all in penalties_cases.NO_BITE); a penalty
served on 89 inputs, added at the flag on 94, retired with on 99 (47 664 fates of serve penalties: 11 754 served, 22 188
at the flag, 13 722 retired); a penalty served at a planned stop on exactly its pending lap on 89 inputs, left unserved
by a stop one lap early on 83; a car that never stops running through a red flag after its pending lap, unserved, on 23
inputs, X_always_red among them; ties: all 64 simulations usable on both cases, S60 29 swap and 35 keep, X_no_noise 34
and 30; F33's even scenarios: 1 983 087 served, 5 239 073 at the flag, 2 983 660 retired.  The floors asserted below are
conditions, set below those figures.

Cost: the device calls are milliseconds each, the file's time is the restatement's.  Wall time on an MI355X machine
(256 CUs), in one visit: at 16 simulations in both a and b this file took 30.8 s against 19.9 s for
tests/test_gpu_stints_moves_fuzz.py, the family's yardstick, which it should not exceed -- 10 s of that were torch's
libraries, loaded for the CU count after the library had initialised HIP, hence the import at the top.  With that and
with b halved to 8 simulations: this file 16.9 s (a 7.4 s, b 2.8 s, d 1.2 s), the yardstick 27.7 s in the same visit
(19.8 s in the visit before).  b stays at 8: at 16 it adds about 3 s, which the yardstick's better visit does not leave."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch        # for _cus(); here and not there: once the library has initialised HIP, loading torch's takes 10 s more

import generic_cases as G
import oracle_py as O
import penalties_cases as PC
import penalties_ref as PR
import resume_ref as RR
import strategy_ref as SR
from helpers import product_run
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

SIMS, STATE_SIMS, OFFSET, TIE_SIMS = 16, 8, 3, 64
KERNEL = 'mcgp::race_penalties_kernel'
COUNT_BLOCK, MAX_SCENARIOS, STAGE_BYTES = 256, 64, 256 << 20
SERVE, FLAG, LAP = PC.SERVE, PC.FLAG, PC.LAP
CORNERS = tuple(G.GOLDEN) + tuple(name for name in G.fuzz_cases() if name.startswith('X_'))


def _run(case, scen, m, seed, off=0, **kw):
    """mcgp_run_penalties under [(penalties, plans)] -> (hist, delta, fate, orders)."""
    rc, h, dl, ft, o = PR.run_c(case, [pl for _, pl in scen], [p for p, _ in scen], m, seed, sim_offset=off, **kw)
    assert rc == 0, N.lib().mcgp_last_error().decode()
    assert N.lib().mcgp_last_kernel_name(0).decode() == KERNEL
    return h, dl, ft, o


def _same_orders(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=-1).reshape(-1))[0]
    assert bad.size == 0, f'{what}: {bad.size} finishing orders differ, first {bad[:5]}'


def _same_counts(h, dl, ft, orders, fates, n, what):
    """hist, delta and fate against the counts of reference orders [S][m][n] and fates [S][m][n]."""
    assert np.array_equal(h, PR.hist_counts(orders, n)), what
    assert np.array_equal(dl, SR.delta_counts(orders, n)), what
    assert np.array_equal(ft, PR.fate_counts(fates, n)), what
    assert (ft.sum(axis=2) == orders.shape[1]).all(), what


@functools.lru_cache(maxsize=None)
def _traced():
    """The oracle's traced run of every run input, made once: [(name, case, seed, ref)]."""
    inputs = G.run_inputs()
    O.lib()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        refs = list(pool.map(lambda a: RR.traced_run(a[1], SIMS, a[2], OFFSET), inputs))
    return [(name, case, seed, ref) for (name, case, seed), ref in zip(inputs, refs)]


# ---------------------------------------------------------------- a. from the grid on every input
def test_from_the_grid_on_every_input(require_gpu):
    expected = [PC.grid_expectation(name, case, seed, ref, SIMS, OFFSET) for name, case, seed, ref in _traced()]
    names = [name for name, _, _, _ in _traced()]
    assert len(names) == 100 and sum(name in G.fuzz_cases() for name in names) == G.N_FUZZ
    quiet = {name for name, e in zip(names, expected) if not e['bites']}
    assert len(PC.NO_BITE) <= 12 and quiet <= set(PC.NO_BITE), sorted(quiet)
    for fate in (PC.FATE_SERVED, PC.FATE_FLAG, PC.FATE_RETIRED):
        seen = sum(fate in e['fates_seen'] for e in expected)
        assert seen >= 80, (fate, seen)
    assert sum(e['on_lap'] for e in expected) >= 70 and sum(e['early'] for e in expected) >= 70
    assert expected[names.index('X_always_red')]['red'] and sum(e['red'] for e in expected) >= 15
    assert len(expected[names.index('X_onelap')]['scen']) == 3
    for (name, case, seed, ref), e in zip(_traced(), expected):
        n = len(case['grid_probs'])
        h, dl, ft, o = _run(case, e['scen'], SIMS, seed, OFFSET)
        _same_orders(o, e['orders'], name)
        _same_counts(h, dl, ft, e['orders'], e['fates'], n, name)
        hist, _, orders = product_run(case, SIMS, seed, sim_offset=OFFSET, orders=True)
        assert np.array_equal(o[0], orders) and np.array_equal(h[0], hist), name


# ---------------------------------------------------------------- b. from a state on every resume input
def _state_laps(name, L):
    laps = {max(1, L // 2)}
    if name in CORNERS:
        laps |= {1, max(1, L - 1), L}
    return sorted(laps)


def test_from_a_state_on_every_input(require_gpu):
    """The gains of buffers of fives are the restatement's counts; scenario 0 is mcgp_run_from_state."""
    resume = {name for name, _, _ in G.resume_inputs()}
    done = states = at_the_flag = 0
    for name, case, seed, ref in _traced():
        if name not in resume:
            continue
        n, L = len(case['grid_probs']), case['config']['total_laps']
        prob, m = RR.problem(case), STATE_SIMS
        for k in _state_laps(name, L):
            st = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, OFFSET, k))
            scen = PC.scenarios(name, n, L, k + 1, from_state=True)
            assert scen[0] == ([], {})
            if k == L:
                assert all(kind == FLAG for pens, _ in scen for _, kind, _, _ in pens)
                at_the_flag += 1
            want = [PR.orders(case, m, seed, 0, plans=plans, penalties=pens, state=st) for pens, plans in scen[1:]]
            h, dl, ft, o = _run(case, scen, m, seed, 0, state=st, prob=prob, fill=5)
            rc, hist, orders = RR.run_c(prob, [st], m, [0], seed)
            assert rc == 0, name
            assert np.array_equal(o[0], orders[0]) and np.array_equal(h[0] - 5, hist[0]), (name, k)
            orders = np.stack([orders[0]] + [w[0] for w in want])
            fates = np.stack([np.zeros((m, n), np.uint8)] + [w[1] for w in want])
            _same_orders(o, orders, (name, k))
            _same_counts(h - 5, dl - 5, ft - 5, orders, fates, n, (name, k))
            states += 1
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and states >= 94 + 3 * 17 and at_the_flag >= 20, (done, states, at_the_flag)


# ---------------------------------------------------------------- c. ties at the flag
@pytest.mark.parametrize('name, flips, keeps', [('S60', 20, 20), ('X_no_noise', 20, 20)])
def test_ties_at_the_flag(require_gpu, name, flips, keeps):
    """An AT_FLAG penalty of exactly t_b - t_a on the winner a: the tied pair is ordered by grid slot."""
    case = O.load_case(name) if name in G.GOLDEN else G.fuzz_cases()[name]
    seed = 42 if name in G.GOLDEN else case['seed']
    ties, n_flips, n_keeps = PC.flag_ties(case, seed, TIE_SIMS, OFFSET)
    assert len(ties) >= 60 and n_flips >= flips and n_keeps >= keeps, (len(ties), n_flips, n_keeps)
    prob = RR.problem(case)
    for i, pens, want in ties:
        h, dl, ft, o = _run(case, [(pens, {})], 1, seed, OFFSET + i, prob=prob)
        assert np.array_equal(o[0, 0], want), (name, i, o[0, 0][:3], want[:3])
        assert np.array_equal(h[0], RR.counts(o[0], len(want)))


# ---------------------------------------------------------------- d. counting and batch loops past two rounds
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _f33_scenarios(n):
    scen = [([], {})]
    for s in range(1, MAX_SCENARIOS):
        if s % 2:
            scen.append(([(d, FLAG, 0, PC.SECONDS[(d + s) % 4] + 0.125 * ((d * s) % 8)) for d in range(n) if (d + s) % 3], {}))
        else:
            plans = {d: (-1, 0, [(5, G.MEDIUM)]) for d in range(n) if (d + s // 2) % 2 == 0}
            scen.append(([(d, SERVE, 2 + (d + s) % 8, 5.0 + 0.25 * d) for d in range(n)], plans))
    return scen


def test_counting_and_batch_loops_past_two_rounds(require_gpu):
    """penalties_count launches min(tiles, max(1, 8 CUs / S)) blocks of 256 per scenario (the rule restated here, not
    read back): F33 under 64 scenarios at two full passes of every block and a ragged third, in one staging chunk; the
    race kernel's batch loop runs with gridDim.y = 64.  Scenario 0 against the oracle, the odd scenarios (flag penalties)
    against reference 2, every fate against reference 1; the even scenarios (serve penalties, planned stops on lap 5 --
    the rule never stops in nine laps) have hist and delta equal to the counts of their returned orders."""
    case = G.fuzz_cases()['F33']
    seed, n, L, S = case['seed'], len(case['grid_probs']), case['config']['total_laps'], MAX_SCENARIOS
    assert (n, L) == (20, 9)
    one_round = max(1, 8 * _cus() // S) * COUNT_BLOCK
    m = 2 * one_round + 77
    assert m > 2 * one_round and m % COUNT_BLOCK and m % 64 and m < STAGE_BYTES // (S * n) // 256 * 256
    scen = _f33_scenarios(n)
    ref = RR.traced_run(case, m, seed, OFFSET)
    odd = list(range(1, S, 2))
    want_odd = PC.flag_orders(ref, np.stack([PC.flag_seconds(scen[s][0], n) for s in odd]))
    fates = np.stack([PC.trace_fates(ref, pens, plans) for pens, plans in scen])
    want_fate = PR.fate_counts(fates, n)
    assert all((want_fate[2::2, :, f] > 0).any() for f in (1, 2, 3)), want_fate[2::2].sum(axis=(0, 1))
    assert all((want_odd[j] != ref['orders']).any() for j in range(len(odd)))
    h, dl, ft, o = _run(case, scen, m, seed, OFFSET)
    _same_orders(o[0], ref['orders'], 'F33 scenario 0')
    _same_orders(o[1::2], want_odd, 'F33 flag penalties')
    assert np.array_equal(ft, want_fate) and (ft.sum(axis=2) == m).all()
    want_odd = np.concatenate([ref['orders'][None], want_odd])
    assert np.array_equal(h[1::2], PR.hist_counts(want_odd[1:], n))
    assert np.array_equal(dl[1::2], SR.delta_counts(want_odd, n)[1:])
    assert np.array_equal(h, PR.hist_counts(o, n)) and np.array_equal(dl, SR.delta_counts(o, n))


# ---------------------------------------------------------------- e. ragged counts
@pytest.mark.parametrize('n', [31, 3])
def test_ragged_counts(require_gpu, n):
    """Simulation counts one short of, one past and far from a wave, two waves and a counting block: fates against
    reference 1 and the flag-only scenario against reference 2 at every count, the rest against the restatement up to
    65 simulations."""
    name, seed = f'n{n}', 5
    case = RR.field_case(n)
    L = case['config']['total_laps']
    scen = PC.scenarios(name, n, L, 2) + [(PC.flag_scenario(name, n), {})]
    assert len(scen) == 5
    for m in (1, 63, 65, 129, 257):
        ref = RR.traced_run(case, m, seed, OFFSET)
        fates = np.stack([PC.trace_fates(ref, pens, plans) for pens, plans in scen])
        flagged = PC.flag_orders(ref, PC.flag_seconds(scen[4][0], n))
        assert m == 1 or (flagged != ref['orders']).any()
        h, dl, ft, o = _run(case, scen, m, seed, OFFSET)
        _same_orders(o[0], ref['orders'], (n, m))
        _same_orders(o[4], flagged, (n, m))
        assert np.array_equal(ft, PR.fate_counts(fates, n)) and (ft.sum(axis=2) == m).all(), (n, m)
        assert np.array_equal(h, PR.hist_counts(o, n)) and np.array_equal(dl, SR.delta_counts(o, n)), (n, m)
        if m <= 65:
            for s in (1, 2, 3):
                want, f = PR.orders(case, m, seed, OFFSET, plans=scen[s][1], penalties=scen[s][0], grids=ref['grids'])
                _same_orders(o[s], want, (n, m, s))
                assert np.array_equal(f, fates[s]), (n, m, s)


# ---------------------------------------------------------------- f. limits
def _against_the_restatement(case, scen, m, seed, what, **kw):
    n = len(case['grid_probs'])
    grids = RR.traced_run(case, m, seed)['grids']
    want = [PR.orders(case, m, seed, plans=plans, penalties=pens, grids=grids) for pens, plans in scen]
    orders, fates = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    h, dl, ft, o = _run(case, scen, m, seed, **kw)
    _same_orders(o, orders, what)
    _same_counts(h, dl, ft, orders, fates, n, what)
    return orders, fates


def _full_scenario(s, n, L):
    """256 penalties and 32 plans: a serve and a flag penalty on every driver; four laps with a lap addition on all 32
    drivers; on each of the other 20 laps driver 31 and two or three more.  Seconds distinct per (lap, driver);
    everything rotates with s."""
    pens = [(d, SERVE, 2 + (d + 2 * s) % (L - 1), 5.0 + d / 8 + s / 1024) for d in range(n)]
    pens += [(d, FLAG, 0, 1.0 + ((d + s) % n) / 16) for d in range(n)]
    sec = lambda lap, d: 0.25 + (lap * 32 + (d + s) % 32) / 1024
    full = [2 + (s + 6 * j) % (L - 1) for j in range(4)]
    rest = [lap for lap in range(2, L + 1) if lap not in full]
    for lap in full:
        pens += [(d, LAP, lap, sec(lap, d)) for d in range(n)]
    for j, lap in enumerate(rest):
        who = {31} | {(lap + s + 11 * i) % 31 for i in range(3 if j < 4 else 2)}
        pens += [(d, LAP, lap, sec(lap, d)) for d in sorted(who)]
    plans = {d: (-1, 0, [(2 + (d + s) % (L - 1), (d + s) % 3)]) for d in range(n)}
    return pens, plans


def test_sixty_four_scenarios_of_256_penalties_and_32_plans(require_gpu):
    n, m, seed = 32, 4, 13
    case = RR.field_case(n)
    L = case['config']['total_laps']
    assert L == 25
    scen = [_full_scenario(s, n, L) for s in range(MAX_SCENARIOS)]
    for pens, plans in scen:
        assert len(pens) == 256 and len(plans) == 32 and len(set((d, k, lap) for d, k, lap, _ in pens)) == 256
        laps = {lap for _, kind, lap, _ in pens if kind == LAP}
        assert laps == set(range(2, L + 1)) and all((31, LAP, lap) in {(d, k, l) for d, k, l, _ in pens} for lap in laps)
        assert sum(sum(1 for _, k, l, _ in pens if k == LAP and l == lap) == 32 for lap in laps) == 4
        assert len({(lap, sec) for _, k, lap, sec in pens if k == LAP}) == 192
    assert scen[0] != scen[1] and scen[0] != scen[32]
    orders, fates = _against_the_restatement(case, scen, m, seed, '64 x 256 x 32')
    assert (fates == PC.FATE_SERVED).any() and len({o.tobytes() for o in orders}) > 32


def _thousand_laps(n, dnf):
    case = RR.field_case(n)
    case = dict(case, config=dict(case['config'], total_laps=1000))
    case['driver_dnf_rates'] = {d: dnf for d in case['base_pace']}
    return case


def test_a_thousand_laps(require_gpu):
    """MCGP_MAX_LAPS: serve_from of 999 and 1000 in a uint16_t, a lap addition on lap 1000, PenaltyLap[1001] per
    scenario with `first` running up to 255 over laps 2 .. 1000."""
    n, m, seed, L = 10, 3, 3, 1000
    case = _thousand_laps(n, 0.0003)
    case['base_pace'] = {d: 90.0 for d in case['base_pace']}       # a close field: every second added shows in the order
    late = [(0, SERVE, 999, 5.0), (1, SERVE, 1000, 10.0), (2, LAP, 1000, 7.5), (9, LAP, 1000, 0.5), (3, SERVE, 999, 4.0)]
    spread = [(j % n, LAP, 2 + j * 998 // 255, 0.5 + (j * 37 % 256) / 8) for j in range(256)]
    assert spread[0][2] == 2 and spread[-1][2] == L and len({(d, lap) for d, _, lap, _ in spread}) == 256
    scen = [([], {}), (late, {1: (-1, 0, [(1000, G.SOFT)]), 3: (-1, 0, [(998, G.SOFT)])}), (spread, {})]
    orders, fates = _against_the_restatement(case, scen, m, seed, 'L1000')
    running = fates[1][:, 1] != PC.FATE_RETIRED
    assert running.any() and (fates[1][running, 1] == PC.FATE_SERVED).all() and (fates[1][:, [0, 3]] != PC.FATE_SERVED).all()
    assert (orders[1] != orders[0]).any() and (orders[2] != orders[0]).any()


def test_seconds_at_both_ends_of_the_range(require_gpu):
    """1e6, 2^-30 and 5e-324 s as a serve, a flag and a lap penalty of one driver: the last is absorbed by every time it
    is added to, so every order is scenario 0's, and the fates are still reported."""
    case, seed, m, d = O.load_case('S60'), 42, 32, 3
    L = case['config']['total_laps']
    scen = [([], {})] + [([(d, SERVE, 10, sec), (d, FLAG, 0, sec), (d, LAP, L // 2, sec)], {}) for sec in (1e6, 2.0 ** -30, 5e-324)]
    orders, fates = _against_the_restatement(case, scen, m, seed, 'seconds')
    assert np.array_equal(orders[3], orders[0]) and (orders[1] != orders[0]).any()
    assert np.array_equal(fates[3], fates[1]) and (fates[3][:, d] == PC.FATE_SERVED).any()
    assert (fates[3][:, d] != PC.FATE_NONE).all()


# ---------------------------------------------------------------- g. chunks from a state
def test_chunks_from_a_state(require_gpu, monkeypatch):
    case, seed, m = O.load_case('S60'), 42, 2500
    n, L = len(case['grid_probs']), case['config']['total_laps']
    k = L // 2
    ref = RR.traced_run(case, 1, seed, OFFSET)
    st = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, OFFSET, k))
    scen = PC.scenarios('S60', n, L, k + 1, from_state=True)
    assert len(scen) == 4 and scen[3][1] and {kind for _, kind, _, _ in scen[3][0]} == {SERVE, FLAG, LAP}
    whole = _run(case, scen, m, seed, 5, state=st)
    monkeypatch.setenv('MCGP_MAX_SIMS_PER_LAUNCH', '1000')
    chunked = _run(case, scen, m, seed, 5, state=st)
    monkeypatch.delenv('MCGP_MAX_SIMS_PER_LAUNCH')
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)
    h, dl, ft, o = whole
    assert np.array_equal(h, PR.hist_counts(o, n)) and np.array_equal(dl, SR.delta_counts(o, n))
    assert (ft.sum(axis=2) == m).all() and (ft[2:, :, 1:] > 0).any(axis=(0, 1)).all() and (o[1:] != o[0]).any()
