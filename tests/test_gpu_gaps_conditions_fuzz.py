"""mcgp_run_gaps and mcgp_run_conditions on the device over the inputs of generic_cases.py -- the comparisons of the second
passes of test_gaps_host_build.py and test_conditions_host_build.py, through the C ABI: race_gaps_kernel<false / true>
with its scalar edge loads from the +inf-padded table, gaps_count_rows and the host side's chunking; race_conditions_kernel
<false / true> and conditions_count.

Gaps are binned at edges that are gaps the oracle's own trace shows (gaps_ref.own_edges: a time off by an ulp, or `<`
for `<=`, moves a count) and at the next double above each; the pairs are those the trace shows at EQUAL cumulative times
(gaps_ref.tied_pairs: the column is then decided by grid slot alone), then a few others.  Conditions are the ones each
input's own reference run shows informative (conditions_ref.choose).  What keeps the comparisons from being vacuous is
asserted from the reference alone, before anything is compared.

References, none of which shares code with the kernels: gaps_ref and conditions_ref over the CPU oracle's per-lap trace
(resume_ref.traced_run), the product's mcgp_run and mcgp_run_from_state for the histograms.  Every comparison is integer
equality.  The oracle's runs are made in a pool of at most 16 threads; what is Python on top of them is not, as threads
only slow that down.

Compared on the device: gaps 48 simulations x 2 edge sets on 100 inputs, 4 simulations x up to 7 laps on 94 inputs from
states, seven edge counts around the groups of eight, and the 1000-lap x 32-car x 63-edge x 64-pair call across staging
chunks; conditions 64 simulations on 100 inputs with and without the histograms, and the same states.  Cost: the
host's share (the references, the choice of edges, pairs and conditions) is most of it; wall time on an MI355X machine,
in one visit: this file 14.3 s, tests/test_gpu_generic_fuzz.py 22.5 s (the yardstick: at most twice its time, else
STATE_SIMS goes from 4 to 2)."""
import ctypes as C
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import conditions_ref as CR
import gaps_ref as GR
import generic_cases as G
import oracle_py as O
import resume_ref as RR
from helpers import product_run
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

GAPS_SIMS, CONDITIONS_SIMS, STATE_SIMS, OFFSET, BASE = 48, 64, 4, 3, 40
KEYS = ('hist', 'lap_gap', 'lead', 'pair')
COUNTS = ('lap_gap', 'lead', 'pair')


def _check(rc):
    assert rc == 0, N.lib().mcgp_last_error().decode()


def _kernel():
    return N.lib().mcgp_last_kernel_name(0).decode()


def _equal(got, want, what, keys=KEYS):
    for key in keys:
        assert got[key].shape == want[key].shape, (what, key)
        bad = np.argwhere(got[key] != want[key])
        assert bad.size == 0, (what, key, len(bad), bad[:5].tolist(), got[key][tuple(bad[0])], want[key][tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def _traced(which):
    """The oracle's traced runs, made once and shared: 'gaps' and 'conditions' of every run input from the grid, 'states'
    of every resume input (the runs whose states both entry points continue).  [(name, case, seed, ref)]."""
    inputs = G.resume_inputs() if which == 'states' else G.run_inputs()
    m, offset = {'gaps': (GAPS_SIMS, OFFSET), 'conditions': (CONDITIONS_SIMS, OFFSET), 'states': (STATE_SIMS, BASE)}[which]
    O.lib()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        refs = list(pool.map(lambda a: RR.traced_run(a[1], m, a[2], offset), inputs))
    return [(name, case, seed, ref) for (name, case, seed), ref in zip(inputs, refs)]


def _values(ref, edges, pairs):
    tr = ref['trace']
    return GR.values_from_times(tr['cum'], tr['dnf'], GR.slots_of(ref['grids']), edges=edges, pairs=pairs)


def _states(case, seed, ref):
    return CR.state_runs(case, seed, ref, range(STATE_SIMS), BASE)


def _resumed_hists(case, seed, runs):
    """mcgp_run_from_state's histogram of every state continued as itself, in one call."""
    rc, hist, _ = RR.run_c(RR.problem(case), [st for _, _, st in runs], 1, [BASE + i for i, _, _ in runs], seed, orders=False)
    _check(rc)
    return hist


# ---------------------------------------------------------------- mcgp_run_gaps
def test_gaps_from_the_grid_on_every_input(require_gpu):
    full, tied, done = 0, set(), 0
    for name, case, seed, ref in _traced('gaps'):
        call = GR.own_call(ref)
        want, want_up = _values(ref, call['edges'], call['pairs']), _values(ref, call['up'], call['pairs'])
        if call['own']:
            moved = int((want != want_up).sum())
            assert moved >= len(call['edges']), (name, moved)         # every edge decides a cell of the reference
        else:
            assert name in ('X_all_out_lap1', 'n1'), name              # no positive gap: nobody runs, or one car
        full += call['own'] and len(call['edges']) == 63
        if call['cells']:
            tied.add(name)
        hist, _, _ = product_run(case, GAPS_SIMS, seed, sim_offset=OFFSET)
        for edges, vals in ((call['edges'], want), (call['up'], want_up)):
            rc, got = GR.run_c(case, GAPS_SIMS, seed, sim_offset=OFFSET, edges=edges, pairs=call['pairs'])
            _check(rc)
            assert _kernel() == 'mcgp::race_gaps_kernel', name
            _equal(got, GR.gap_counts(case, GAPS_SIMS, seed, OFFSET, edges, call['pairs'], ref=ref, vals=vals), name)
            assert np.array_equal(got['hist'], hist), name
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ
    assert full >= 98, full
    assert len(tied) >= 25 and {'X_no_noise', 'X_all_attempt'} <= tied, sorted(tied)


def test_gaps_from_a_state_on_every_input(require_gpu):
    """Every state continued as itself, accumulated into buffers of fives: rows k + 1 .. L gain the oracle trace's counts
    at the run's own edges and tied pairs, the rows before stay five, the histogram is mcgp_run_from_state's."""
    done = states = 0
    for name, case, seed, ref in _traced('states'):
        call = GR.own_call(ref)
        edges, pairs = call['edges'], call['pairs']
        vals = _values(ref, edges, pairs)
        runs = _states(case, seed, ref)
        hists = _resumed_hists(case, seed, runs)
        prob = RR.problem(case)
        n, L = prob.n, case['config']['total_laps']
        for s, (i, k, st) in enumerate(runs):
            into = {key: np.full_like(v, 5, dtype=np.uint64) for key, v in GR.empty(n, L, len(edges), len(pairs)).items()}
            rc, got = GR.run_c(case, 1, seed, sim_offset=BASE + i, edges=edges, pairs=pairs, state=st, prob=prob, into=into)
            _check(rc)
            assert _kernel() == 'mcgp::race_gaps_kernel', name
            for key in COUNTS:
                assert (got[key][:k] == 5).all(), (name, i, k, key)
            got = {key: v - 5 for key, v in got.items()}
            _equal(got, GR.continued_counts(ref, [i], k, edges, pairs, vals=vals), (name, i, k))
            assert np.array_equal(got['hist'], hists[s]), (name, i, k)
        assert len(runs) >= STATE_SIMS, name
        states += len(runs)
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and states >= 94 * STATE_SIMS * 3


def test_edge_counts_around_the_groups_of_eight(require_gpu):
    """The device reads its edge table eight at a time and the host pads it with +inf to 64: 7, 8, 9, 16, 17, 56 and 57
    own edges, the values above the last of which all fall into the last bin."""
    case, seed, m = O.load_case('S60'), 7, 256
    ref = RR.traced_run(case, m, seed)
    call = GR.own_call(ref)
    assert call['own'] and len(call['edges']) == 63 and call['cells'] > 0
    for n_edges in (7, 8, 9, 16, 17, 56, 57):
        for edges in (call['edges'][:n_edges], call['up'][:n_edges]):
            want = GR.gap_counts(case, m, seed, edges=edges, pairs=call['pairs'], ref=ref)
            assert (want['lap_gap'][:, :, :n_edges + 1].sum(axis=(0, 1)) > 0).all()          # every bin is in use
            rc, got = GR.run_c(case, m, seed, edges=edges, pairs=call['pairs'])
            _check(rc)
            _equal(got, want, n_edges)


def _launch_info():
    g, b, l = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert N.lib().mcgp_last_launch_info(0, C.byref(g), C.byref(b), C.byref(l)) == 0
    return g.value, b.value


@functools.lru_cache(maxsize=None)
def _limits():
    """32 cars over 1000 laps, most of them out somewhere; the 63 edges and 64 pairs a 40-simulation trace decides."""
    n, m, seed = 32, 40, 6
    case = RR.field_case(n)
    case = dict(case, config=dict(case['config'], total_laps=1000))
    case['driver_dnf_rates'] = {d: 0.002 for d in case['base_pace']}
    ref = RR.traced_run(case, m, seed)
    more = [(a, b) for a in range(n) for b in (n - 1 - a, (a + 1) % n) if a != b]
    call = GR.own_call(ref, more_pairs=more)
    assert len(call['edges']) == 63 and call['own'] and len(call['pairs']) == 64 == len(set(call['pairs']))
    return case, seed, m, ref, call


def test_every_limit_of_a_gaps_call_at_once(require_gpu):
    """MCGP_MAX_LAPS x (32 + 1 + 64) = 97 000 staged rows through the grid-stride loop of gaps_count_rows at its widest
    LDS (129 values), a chunk of 512 MiB / 97 000 simulations -- less than one round of the device: 40 simulations equal
    the oracle, and a run of a little more than two chunks equals the sum of its parts and loses no simulation."""
    case, seed, m, ref, call = _limits()
    edges, pairs = call['edges'], call['pairs']
    rc, got = GR.run_c(case, m, seed, edges=edges, pairs=pairs)
    _check(rc)
    assert _kernel() == 'mcgp::race_gaps_kernel'
    _equal(got, GR.gap_counts(case, m, seed, edges=edges, pairs=pairs, ref=ref), 'limits')
    assert got['lap_gap'].shape == (1000, 32, 65) and got['pair'].shape == (1000, 64, 129)
    chunk = GR.budget_sims(32, 1000, 64)
    assert chunk == (512 << 20) // 97000 // 256 * 256
    N_ = 2 * chunk + 1001
    rc, whole = GR.run_c(case, N_, seed, edges=edges, pairs=pairs)
    _check(rc)
    grid, block = _launch_info()
    assert grid == -(-chunk // block)                       # the first chunk held the budget: less than a device round
    h = N_ // 2 + 3
    rc1, a = GR.run_c(case, h, seed, edges=edges, pairs=pairs)
    rc2, b = GR.run_c(case, N_ - h, seed, sim_offset=h, edges=edges, pairs=pairs)
    _check(rc1)
    _check(rc2)
    _equal(whole, {key: a[key] + b[key] for key in KEYS}, 'split')
    assert (whole['lap_gap'].sum(axis=2) == N_).all() and (whole['lead'].sum(axis=1) == N_).all()
    assert (whole['pair'].sum(axis=2) == N_).all()
    hist, _, _ = product_run(case, N_, seed)
    assert np.array_equal(whole['hist'], hist)


def test_every_limit_of_a_gaps_call_from_a_state_after_lap_999(require_gpu):
    """The same call from a state: one recorded lap, row 999 of 1000.  Traced simulations continued as themselves equal
    the oracle's last lap, and N simulations from one state equal the sum of two parts, every row of lap 1000 summing to
    N and the 999 rows before it untouched."""
    case, seed, m, ref, call = _limits()
    edges, pairs = call['edges'], call['pairs']
    vals = _values(ref, edges, pairs)
    prob, k = RR.problem(case), 999
    running = (ref['trace']['dnf'][:, k - 1] == 0).sum(axis=1)
    sims = [int(i) for i in np.argsort(-running, kind='stable')[:4]]
    assert running[sims[0]] >= 2
    states = {i: (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, i, k)) for i in sims}
    for i in sims:
        rc, got = GR.run_c(case, 1, seed, sim_offset=i, edges=edges, pairs=pairs, state=states[i], prob=prob)
        _check(rc)
        _equal(got, GR.continued_counts(ref, [i], k, edges, pairs, vals=vals), ('limits', i))
    st = states[sims[0]]
    N_ = 2 * GR.budget_sims(32, 1000, 64) + 1001
    rc, whole = GR.run_c(case, N_, seed, edges=edges, pairs=pairs, state=st, prob=prob)
    _check(rc)
    assert _kernel() == 'mcgp::race_gaps_kernel'
    h = N_ // 2 + 3
    rc1, a = GR.run_c(case, h, seed, edges=edges, pairs=pairs, state=st, prob=prob)
    rc2, b = GR.run_c(case, N_ - h, seed, sim_offset=h, edges=edges, pairs=pairs, state=st, prob=prob)
    _check(rc1)
    _check(rc2)
    _equal(whole, {key: a[key] + b[key] for key in KEYS}, 'state split')
    for key in COUNTS:
        assert not whole[key][:k].any(), key
    assert (whole['lap_gap'][k].sum(axis=1) == N_).all() and whole['lead'][k].sum() == N_
    assert (whole['pair'][k].sum(axis=1) == N_).all()
    rc, hist, _ = RR.run_c(prob, [st], N_, [0], seed, orders=False)
    _check(rc)
    assert np.array_equal(whole['hist'], hist[0])


# ---------------------------------------------------------------- mcgp_run_conditions
def test_conditions_from_the_grid_on_every_input(require_gpu):
    used, eight, total, done = set(), 0, 0, 0
    for name, case, seed, ref in _traced('conditions'):
        n, L = len(case['grid_probs']), case['config']['total_laps']
        facts = CR.oracle_facts(case, CONDITIONS_SIMS, seed, OFFSET, ref=ref)
        conds, constant = CR.choose(facts, n, L, seed)
        CR.assert_informative(facts, conds, constant)
        k = constant[0]
        if n >= 3:
            assert k >= 20, (name, k)
        want = CR.counts(facts, conds)
        assert np.array_equal(want['hist'], ref['hist'])
        rc, got = CR.run_c(case, conds, CONDITIONS_SIMS, seed, sim_offset=OFFSET)
        _check(rc)
        assert _kernel() == 'mcgp::race_conditions_kernel', name
        _equal(got, want, name, keys=('hist', 'count', 'cond_hist'))
        rc, only = CR.run_c(case, conds, CONDITIONS_SIMS, seed, sim_offset=OFFSET, cond_hist=False)      # cond_hist_out NULL
        _check(rc)
        _equal(only, want, (name, 'counts only'), keys=('hist', 'count'))
        assert not only['cond_hist'].any()
        used |= CR.facts_used(conds[:k])
        eight += sum(len(c) == 8 for c in conds[:k])
        total += k
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ
    assert used == set(CR.FACT_NAMES)
    assert total >= 5000 and eight >= 2500, (total, eight)


def test_conditions_from_a_state_on_every_input(require_gpu):
    """Every state continued as itself gives that simulation's facts, events counted from the state's lap on; the
    histogram is mcgp_run_from_state's."""
    done = states = 0
    for name, case, seed, ref in _traced('states'):
        n, L = len(case['grid_probs']), case['config']['total_laps']
        runs = _states(case, seed, ref)
        facts = CR.concat([CR.oracle_facts(case, 0, seed, BASE, ref=ref, sims=[i], lap0=k) for i, k, _ in runs])
        conds, constant = CR.choose(facts, n, L, seed + 1)
        CR.assert_informative(facts, conds, constant)
        want = CR.counts_each(facts, conds)
        hists = _resumed_hists(case, seed, runs)
        prob, table = RR.problem(case), CR.c_conditions(conds)
        for s, (i, k, st) in enumerate(runs):
            rc, got = CR.run_c(case, conds, 1, seed, sim_offset=BASE + i, state=st, prob=prob, table=table)
            _check(rc)
            assert _kernel() == 'mcgp::race_conditions_kernel', name
            _equal(got, {key: want[key][s] for key in ('hist', 'count', 'cond_hist')}, (name, i, k),
                   keys=('hist', 'count', 'cond_hist'))
            assert np.array_equal(got['hist'], hists[s]), (name, i, k)
        states += len(runs)
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and states >= 94 * STATE_SIMS * 3
