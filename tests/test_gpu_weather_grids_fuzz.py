"""mcgp_run_grids and mcgp_run_weather on the device at the limits of include/mcgp.h, through the C ABI:
race_scenario_kernel<false, kRuleGrid> and <false / true, kRuleWeather> at every block shape the inputs' field sizes give,
grid_count and weather_count at sizes where their grid-stride loops iterate, and the host side's chunking.  The cases come
from grids_limit_cases.py and weather_limit_cases.py, and tests/test_grids_limits_host_build.py and
tests/test_weather_limits_host_build.py run them on the host build of the same kernel text.

References: the Python restatements grids_ref and weather_ref (which share no code with the kernels); the CPU oracle's
finishing orders for the empty scenario; for the start slots of drop-only scenarios the reference project's own rule
(grids_limit_cases.reference_rule_slots, asserted where the restatement is made); for the counting loops edited_grid on the
oracle's drawn grids and a closed form of the laps on the wrong tyres from the oracle's trace.  Every comparison is
integer equality, and after every call mcgp_last_kernel_name is mcgp::race_grids_kernel or mcgp::race_weather_kernel.  What
keeps the comparisons from being vacuous is asserted from the references alone (the MEASURED figures and floors of the two
case modules, and in the host tests).

1. Grid edits: 8 simulations at sim_offset 3 on the 100 inputs of run_inputs() under the empty scenario, six random
   mixtures of drops, pins and pit-lane starts and the five whole-field sets, into buffers of sevens: orders, hist, delta,
   start and gain are the restatement's, every row sums to m.
2. Weather: the 8 golden and 12 X_ inputs under 17 tables (one non-zero cell each, a checkerboard, 60.0 beside 5e-324); 64
   scenarios of 64 changes on 32 cars; 1000 laps (column 1000 holds all 8 simulations); one lap; all out on lap 1 on the
   wrong tyres; the wrong class on every lap (column L); states after laps 1, L - 1 and L.
3. F33 under 64 scenarios at two rounds and a ragged third of grid_count's and weather_count's one block per (scenario,
   driver), in one staging chunk: start against edited_grid on the oracle's grids, gain against those slots and the
   returned orders; wrong_laps of the planned scenarios against the closed form; hist and delta against the counts of the
   returned orders; all against the sum of split calls; the first 8 ids against the restatements.
4. Staging chunks (200 simulations under a cap of 64 per launch) with every subset of the optional outputs wanted: the
   unchunked call, the unwanted buffers untouched.  One call of each kind just past its staging budget (64 scenarios x 32
   cars x 3 laps, 3n bytes per scenario and simulation): the sum of two single-chunk calls.
5. RaceSimulator.run_weather(device='all') gives device 0's counts.

Cost: the device calls are milliseconds each, the file's time is the restatements'.  Wall time on an MI355X machine (256
CUs), in one visit: this file 21.5 s (part 1 8.8 s, the tables 5.8 s, the states 2.3 s, the limits 0.9 s, part 3 0.9 s,
parts 4 and 5 0.5 s) against 27.4 s for tests/test_gpu_stints_moves_fuzz.py, the family's yardstick, which it should not
exceed.  (strategy_ref keeps the Philox words of a counter, which the scenarios of a call share, and the tables' sweep
runs a scenario once per distinct content of the table rows its laps read; before both, and with the empty scenario
under every table as well, the file took 40.1 s.)"""
import itertools

import numpy as np
import pytest
import torch        # for _cus(); here and not there: once the library has initialised HIP, loading torch's takes 10 s more

import generic_cases as G
import grids_limit_cases as GL
import grids_ref as GR
import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
import weather_cases as WC
import weather_limit_cases as WL
import weather_ref as WR
from monte_carlo_gp_amd import PitPlan, RaceConfig, TrackChange
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, RaceSimulator

pytestmark = pytest.mark.gpu

SIMS, OFFSET = GL.FUZZ_SIMS, GL.FUZZ_OFFSET
GRIDS_KERNEL, WEATHER_KERNEL = 'mcgp::race_grids_kernel', 'mcgp::race_weather_kernel'
COUNT_BLOCK, MAX_SCENARIOS, STAGE_BYTES = 256, 64, 256 << 20
FILL = 7
GRID_COUNTS, WEATHER_COUNTS = ('hist', 'delta', 'start', 'gain'), ('hist', 'delta', 'wrong_laps')


def _grids(case, scen, m, seed, off=0, fill=0, **kw):
    """mcgp_run_grids under [(edits, plans)] -> dict(hist, delta, start, gain, orders), the counts less what the buffers
    held before the call."""
    rc, h, dl, st, gn, o = GR.run_c(case, [pl for _, pl in scen], [ed for ed, _ in scen], m, seed, sim_offset=off, fill=fill,
                                    **kw)
    assert rc == 0, N.lib().mcgp_last_error().decode()
    assert N.lib().mcgp_last_kernel_name(0).decode() == GRIDS_KERNEL
    return dict(hist=h - fill, delta=dl - fill, start=st - fill, gain=gn - fill, orders=o)


def _weather(case, table, scen, m, seed, off=0, fill=0, **kw):
    """mcgp_run_weather under [(changes, plans)] -> dict(hist, delta, wrong_laps, orders), likewise."""
    rc, h, dl, wl, o = WR.run_c(case, [pl for _, pl in scen], [ch for ch, _ in scen], table, m, seed, sim_offset=off,
                                fill=fill, **kw)
    assert rc == 0, N.lib().mcgp_last_error().decode()
    assert N.lib().mcgp_last_kernel_name(0).decode() == WEATHER_KERNEL
    return dict(hist=h - fill, delta=dl - fill, wrong_laps=wl - fill, orders=o)


def _sum(a, b, keys):
    return {k: a[k] + b[k] for k in keys}


def _same(a, b, what, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------- 1. grid edits: random mixtures
@pytest.mark.parametrize('part', range(GL.PARTS))
def test_grid_mixtures_on_every_input(require_gpu, part):
    for name, case, seed, scen, want_o, want_s in GL.wanted(part)[0]:
        got = _grids(case, scen, SIMS, seed, OFFSET, fill=FILL)
        GL.check_against(got, case, want_o, want_s, SIMS)
        assert (got['start'].sum(axis=2) == SIMS).all() and (got['start'].sum(axis=1) == SIMS).all(), name
        assert (got['gain'].sum(axis=2) == SIMS).all(), name


def test_the_mixtures_do_not_pass_empty(require_gpu):
    GL.check_floors(GL.marks(), GL.FLOORS)


# ---------------------------------------------------------------- 2. weather: tables, limits, first and last laps
@pytest.mark.parametrize('part', range(WL.TABLE_PARTS))
def test_weather_tables_with_one_cell_a_checkerboard_and_the_extremes(require_gpu, part):
    for name, case, seed, calls in WL.table_wanted(part)[0]:
        prob = RR.problem(case)
        for table, scen, want_o, want_w in calls:
            got = _weather(case, table, scen, SIMS, seed, OFFSET, fill=FILL, prob=prob)
            WC.check_against(got, case, want_o, want_w, SIMS)


@pytest.mark.parametrize('k', range(len(WL.LIMITS)))
def test_weather_limits(require_gpu, k):
    label, case, seed, table, scen, m, offset, want_o, want_w = WL.limit_wanted(k)
    L = case['config']['total_laps']
    if label == 'a thousand laps':
        assert (want_w[1][:, 0] == L).all()                 # from the restatement first
    got = _weather(case, table, scen, m, seed, offset, fill=FILL)
    WC.check_against(got, case, want_o, want_w, m)
    assert (got['wrong_laps'].sum(axis=2) == m).all()
    if label == 'a thousand laps':
        assert got['wrong_laps'][1, 0, L] == m
    if label == 'all out on lap 1':
        assert (got['wrong_laps'][:, :, 0] == m).all()


@pytest.mark.parametrize('part', range(WL.STATE_PARTS))
def test_weather_from_states_after_the_first_and_the_last_laps(require_gpu, part):
    for name, case, seed, k, state, calls in WL.state_wanted(part):
        prob = RR.problem(case)
        for table, scen, want_o, want_w in calls:
            got = _weather(case, table, scen, SIMS, seed, 0, fill=FILL, state=state, prob=prob)
            WC.check_against(got, case, want_o, want_w, SIMS)


def test_the_weather_limits_do_not_pass_empty(require_gpu):
    assert WL.tables_moved() >= WL.TABLES_FLOOR and WL.column_l_cells() >= WL.COLUMN_L_FLOOR


# ---------------------------------------------------------------- 3. counting loops past two rounds
def _two_rounds_and_a_ragged_third(n):
    """grid_count and weather_count launch min(tiles, max(1, 8 CUs / (S n))) blocks of 256 per scenario and driver (the
    rule restated here, not read back): m is two full passes of those blocks and a ragged third, in one staging chunk of
    3n bytes per scenario and simulation."""
    one_round = max(1, 8 * _cus() // (MAX_SCENARIOS * n)) * COUNT_BLOCK
    m = 2 * one_round + 77
    assert m % COUNT_BLOCK and m % 64
    assert m < STAGE_BYTES // (MAX_SCENARIOS * 3 * n) // 256 * 256
    return one_round, m


def test_grid_counting_loops_past_two_rounds(require_gpu):
    case = G.fuzz_cases()['F33']
    seed, n, L = case['seed'], len(case['grid_probs']), case['config']['total_laps']
    assert (n, L) == (20, 9)
    one_round, m = _two_rounds_and_a_ragged_third(n)
    scen = GL.full_scenarios('F33', case)
    ref = RR.traced_run(case, m, seed, OFFSET)
    slots = GL.edited_slots(scen, ref['grids'])                                 # no race is run
    want_start = GR.start_counts(slots, n)
    assert (want_start.sum(axis=2) == m).all() and (want_start > 0).sum(axis=2).max() > 10
    got = _grids(case, scen, m, seed, OFFSET)
    assert np.array_equal(got['orders'][0], ref['orders'])
    assert np.array_equal(got['start'], want_start)
    assert np.array_equal(got['gain'], GR.gain_counts(slots, got['orders'], n))
    assert np.array_equal(got['hist'], GR.hist_counts(got['orders'], n))
    assert np.array_equal(got['delta'], SR.delta_counts(got['orders'], n))
    a = one_round + 31
    lo, hi = _grids(case, scen, a, seed, OFFSET, orders=False), _grids(case, scen, m - a, seed, OFFSET + a, orders=False)
    _same(got, _sum(lo, hi, GRID_COUNTS), 'F33 split', GRID_COUNTS)
    first = _grids(case, scen, SIMS, seed, OFFSET)
    assert np.array_equal(first['orders'], got['orders'][:, :SIMS])
    GL.check_against(first, case, *GL.restate(case, seed, scen, ref['grids'][:SIMS], SIMS, OFFSET), SIMS)


def test_weather_counting_loops_past_two_rounds(require_gpu):
    case, seed = WL.f33()
    n, L = len(case['grid_probs']), case['config']['total_laps']
    one_round, m = _two_rounds_and_a_ragged_third(n)
    scen = WL.f33_scenarios(n, L)
    ref = RR.traced_run(case, m, seed, OFFSET)
    want_even = WR.wrong_counts(WL.trace_wrong_laps(ref, scen[::2], WR.DRY, L), L)
    assert ((want_even[:, :, 1:] > 0).any(axis=(0, 1))).sum() >= 5              # five distinct columns above 0
    got = _weather(case, WL.FULL, scen, m, seed, OFFSET)
    assert np.array_equal(got['wrong_laps'][::2], want_even)
    assert (got['wrong_laps'].sum(axis=2) == m).all() and (got['wrong_laps'][1::2, :, 1:] > 0).any()
    assert np.array_equal(got['hist'], WR.hist_counts(got['orders'], n))
    assert np.array_equal(got['delta'], SR.delta_counts(got['orders'], n))
    a = one_round + 31
    lo = _weather(case, WL.FULL, scen, a, seed, OFFSET, orders=False)
    hi = _weather(case, WL.FULL, scen, m - a, seed, OFFSET + a, orders=False)
    _same(got, _sum(lo, hi, WEATHER_COUNTS), 'F33 split', WEATHER_COUNTS)
    first = _weather(case, WL.FULL, scen, SIMS, seed, OFFSET)
    assert np.array_equal(first['orders'], got['orders'][:, :SIMS])
    WC.check_against(first, case, *WL.restate(case, seed, WL.FULL, scen, SIMS, OFFSET, grids=ref['grids'][:SIMS]), SIMS)


# ---------------------------------------------------------------- 4. chunks
def _subsets(names):
    return [dict(zip(names, wanted)) for wanted in itertools.product((True, False), repeat=len(names))]


def _chunked_is_unchunked(run, keys, optional, monkeypatch):
    """200 simulations under a cap of 64 per launch are four chunks with a short last one: every wanted output is the
    unchunked call's, every unwanted buffer keeps its sevens."""
    whole = run(fill=FILL)
    subsets = _subsets(optional)
    monkeypatch.setenv('MCGP_MAX_SIMS_PER_LAUNCH', '64')
    chunked = [run(fill=FILL, **kw) for kw in subsets]
    monkeypatch.delenv('MCGP_MAX_SIMS_PER_LAUNCH')
    for kw, got in zip(subsets, chunked):
        for key in keys:
            if kw.get(key, True):
                assert np.array_equal(got[key], whole[key]), (kw, key)
            else:
                assert got[key] is None or not got[key].any(), (kw, key)    # (the sevens, taken off again)
    return whole


def test_grid_chunks_with_every_subset_of_the_outputs(require_gpu, monkeypatch):
    case = O.load_case('S60')
    n, m = len(case['grid_probs']), 200
    scen = GL.scenarios('S60', case)
    whole = _chunked_is_unchunked(lambda **kw: _grids(case, scen, m, 42, 5, **kw), GRID_COUNTS + ('orders',),
                                  ('delta', 'start', 'gain', 'orders'), monkeypatch)
    assert np.array_equal(whole['hist'], GR.hist_counts(whole['orders'], n))
    assert (whole['start'].sum(axis=2) == m).all() and (whole['gain'].sum(axis=2) == m).all()
    assert not np.array_equal(whole['start'][1], whole['start'][0])


def test_weather_chunks_from_a_state_with_every_subset_of_the_outputs(require_gpu, monkeypatch):
    case = O.load_case('S60')
    n, L, m, seed = len(case['grid_probs']), case['config']['total_laps'], 200, 42
    k = L // 2
    ref = RR.traced_run(case, 1, seed, OFFSET)
    state = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, OFFSET, k))
    scen = WC.scenarios('S60', case, first=k + 1)[0][1]
    assert len(scen) >= 6
    whole = _chunked_is_unchunked(lambda **kw: _weather(case, WL.FULL, scen, m, seed, 5, state=state, **kw),
                                  WEATHER_COUNTS + ('orders',), ('delta', 'wrong_laps', 'orders'), monkeypatch)
    assert np.array_equal(whole['hist'], WR.hist_counts(whole['orders'], n))
    assert (whole['wrong_laps'].sum(axis=2) == m).all() and (whole['wrong_laps'][1:, :, 1:] > 0).any()


def _budget_chunk(n):
    """64 scenarios of 32 cars with the u16 staging wanted stage 64 x 3n = 6144 bytes per simulation (include/mcgp.h), so a
    chunk of the 256 MiB budget holds 43 690 simulations, in whole blocks of 256 43 520."""
    chunk = STAGE_BYTES // (MAX_SCENARIOS * 3 * n) // 256 * 256
    assert chunk == 43520
    return chunk


def test_a_grids_call_just_past_its_staging_budget(require_gpu):
    n, seed = 32, 9
    case = RR.field_case(n)
    case['config'] = dict(case['config'], total_laps=3)
    chunk = _budget_chunk(n)
    m = chunk + 77
    scen = GL.full_scenarios('n32', case)
    one = _grids(case, scen, m, seed, 3, orders=False)
    lo, hi = _grids(case, scen, chunk, seed, 3, orders=False), _grids(case, scen, m - chunk, seed, 3 + chunk, orders=False)
    _same(one, _sum(lo, hi, GRID_COUNTS), 'budget', GRID_COUNTS)
    for k in GRID_COUNTS:
        assert (one[k].sum(axis=2) == m).all(), k
    assert (one['start'].sum(axis=1) == m).all() and not np.array_equal(one['hist'][1], one['hist'][0])


def test_a_weather_call_just_past_its_staging_budget(require_gpu):
    case, seed, table, scen = WL.budget_call()
    n, L = len(case['grid_probs']), case['config']['total_laps']
    chunk = _budget_chunk(n)
    m = chunk + 77
    one = _weather(case, table, scen, m, seed, 3, orders=False)
    lo = _weather(case, table, scen, chunk, seed, 3, orders=False)
    hi = _weather(case, table, scen, m - chunk, seed, 3 + chunk, orders=False)
    _same(one, _sum(lo, hi, WEATHER_COUNTS), 'budget', WEATHER_COUNTS)
    for k in WEATHER_COUNTS:
        assert (one[k].sum(axis=2) == m).all(), k
    assert (one['wrong_laps'][:, :, L] > 0).any() and (one['wrong_laps'][0, :, 0] == m).all()


# ---------------------------------------------------------------- 5. every device
def test_run_weather_on_all_devices_gives_device_0s_counts(require_gpu):
    c = O.load_case('S60')
    d, L = list(c['grid_probs']), c['config']['total_laps']
    args = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    changes = {'forecast': [], 'rain': [TrackChange(30, L, 'damp')], 'shower': [TrackChange(20, 30, 'wet')]}
    plans = {'rain': [PitPlan(d[0], [(30, 'INTERMEDIATE')]), PitPlan(d[1], [])]}
    res = {}
    for device in (0, 'all'):
        sim = RaceSimulator(RaceConfig(**c['config']), set_pop=DEFAULT_SET_POP, device=device)
        res[device] = sim.run_weather(3000, changes, plans, None, *args, grid_probs=c['grid_probs'], seed=9, return_orders=True)
    one, every = res[0], res['all']
    for k in ('hist', 'delta', 'wrong_laps', 'orders'):
        assert np.array_equal(getattr(one, k), getattr(every, k)), k
    assert one.names == ['forecast', 'rain', 'shower'] and (one.wrong_laps.sum(axis=2) == 3000).all()
    assert (one.wrong_laps[0, :, 0] == 3000).all()
    assert one.expected_wrong_tyre_laps('rain', d[1]) > one.expected_wrong_tyre_laps('rain', d[0]) > 0
