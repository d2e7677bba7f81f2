"""Grid scenarios on the device (mcgp_run_grids, through the C ABI) against the Python restatement (grids_ref) under the
generated scenario sets of grids_cases -- the 100 inputs of generic_cases.run_inputs() at 8 simulations with sim_offset 3
(n = 1, 2, 3, 19, 31, 32, L from 1 up, DMP, WET, EVT and the red-flag-heavy fuzz cases among them), into pre-filled
buffers: finishing orders, hist, delta, start and gain -- and against the device's own mcgp_run for scenario 0 and
mcgp_simulate_race for the scenario that pins every driver, and against itself: a split by sim_offset sums to the one call,
and device='all' gives device 0's counts.

The sweep does not pass empty.  By grids_ref alone, on this project's CPU reference: an edit changed a start compound on
49 of the 100 inputs (the dry ones with 11 cars or more), a finishing order moved on 94, and a pit-lane car was classified
ahead of a car that started from the grid on 97.  The floors (grids_cases.FLOORS) are a little below: 44, 88, 90.

Left to tests/test_gpu_weather_grids_fuzz.py: random mixtures of edits and the whole field edited at once, grid_count past
one step of its loop against a reference, staging chunks, and a call past the staging budget."""
import ctypes as C

import numpy as np
import pytest

import grids_cases as GC
import grids_ref as GR
import oracle_py as O
import resume_ref as RR
from monte_carlo_gp_amd import GridEdit, RaceConfig
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, RaceSimulator

pytestmark = pytest.mark.gpu

KERNEL = 'mcgp::race_grids_kernel'
FILL = 7


def _run(case, scen, m, seed, off=0, fill=0, **kw):
    """mcgp_run_grids under [(edits, plans)] -> dict(hist, delta, start, gain, orders), the pre-filled `fill` taken off the
    accumulated counts."""
    rc, h, dl, st, gn, o = GR.run_c(case, [pl for _, pl in scen], [ed for ed, _ in scen], m, seed, sim_offset=off, fill=fill,
                                    **kw)
    assert rc == 0, N.lib().mcgp_last_error().decode()
    assert N.lib().mcgp_last_kernel_name(0).decode() == KERNEL
    return dict(hist=h - fill, delta=dl - fill, start=st - fill, gain=gn - fill, orders=o)


def _mcgp_run(case, prob, m, seed, off):
    g = np.ascontiguousarray(O.Problem(case).grid_probs, np.float64)
    h, o = np.zeros((prob.n, prob.n), np.uint64), np.zeros((m, prob.n), np.uint8)
    N.check(N.lib().mcgp_run(C.byref(prob.cfg), C.byref(prob.drv), g.ctypes.data_as(C.POINTER(C.c_double)), prob.n, m,
                             off, seed, 0, h.ctypes.data_as(C.POINTER(C.c_uint64)), o.ctypes.data_as(C.POINTER(C.c_uint8))))
    return h.astype(np.int64), o


def _simulate_race(prob, grid, seed, sim_id):
    fg, o = np.ascontiguousarray(grid, np.uint8), np.zeros(prob.n, np.uint8)
    N.check(N.lib().mcgp_simulate_race(C.byref(prob.cfg), C.byref(prob.drv), fg.ctypes.data_as(C.POINTER(C.c_uint8)), prob.n,
                                       sim_id, seed, 0, o.ctypes.data_as(C.POINTER(C.c_uint8))))
    return o


@pytest.mark.parametrize('part', range(GC.PARTS))
def test_device_on_every_input(require_gpu, part):
    m, off = GC.FUZZ_SIMS, GC.FUZZ_OFFSET
    for name, case, seed, scen, at, want_o, want_s in GC.wanted(part)[0]:
        prob = RR.problem(case)
        n = prob.n
        got = _run(case, scen, m, seed, off, fill=FILL, prob=prob)
        GC.check_against(got, case, want_o, want_s, m)
        assert (got['start'].sum(axis=2) == m).all() and (got['start'].sum(axis=1) == m).all(), name
        assert (got['gain'].sum(axis=2) == m).all(), name
        # scenario 0 is mcgp_run's race
        hist, orders = _mcgp_run(case, prob, m, seed, off)
        assert np.array_equal(got['orders'][0], orders) and np.array_equal(got['hist'][0], hist), name
        # the scenario that pins every driver is mcgp_simulate_race with that grid, simulation by simulation
        s = at[GC.ALL_PINNED]
        grid = [0] * n
        for d, (_, slot, _) in scen[s][0].items():
            grid[slot - 1] = d
        for i in range(m):
            assert np.array_equal(got['orders'][s, i], _simulate_race(prob, grid, seed, off + i)), (name, i)


def test_the_sweep_does_not_pass_empty(require_gpu):
    GC.check_floors(GC.marks(), GC.FLOORS)


def test_a_split_by_sim_offset_sums_to_one_call(require_gpu):
    case = O.load_case('S60')
    n = len(case['grid_probs'])
    scen = [({}, {}), ({0: (GR.DROP, 10, 0.0)}, {}),
            ({n - 1: (GR.PIT_LANE, 0, 2.5), 1: (GR.PIN, 1, 0.0)}, {n - 1: (2, 0, [(30, 1)])})]
    m, cut = 1000, 333                                      # neither a multiple of a wave or of a counting block
    whole = _run(case, scen, m, 11, 5)
    a = _run(case, scen, cut, 11, 5)
    b = _run(case, scen, m - cut, 11, 5 + cut)
    for k in ('hist', 'delta', 'start', 'gain'):
        assert np.array_equal(a[k] + b[k], whole[k]), k
    assert np.array_equal(np.concatenate([a['orders'], b['orders']], axis=1), whole['orders'])
    # the counts are those of the returned orders, and the edits bite
    assert np.array_equal(whole['hist'], GR.hist_counts(whole['orders'], n))
    assert (whole['start'].sum(axis=2) == m).all() and (whole['start'].sum(axis=1) == m).all()
    assert (whole['gain'].sum(axis=2) == m).all()
    assert whole['start'][2, n - 1, n - 1] == m and whole['start'][2, 1, 0] == m
    assert not np.array_equal(whole['orders'][1], whole['orders'][0])
    assert not np.array_equal(whole['orders'][2], whole['orders'][0])
    # the gains are the start slots against the returned orders
    pos = np.argsort(whole['orders'], axis=2)
    for s in range(3):
        mean_gain = (whole['gain'][s] @ np.arange(-(n - 1), n)) / m
        mean_start = (whole['start'][s] @ np.arange(n)) / m
        assert np.allclose(mean_gain, mean_start - pos[s].mean(axis=0))
    # without the optional outputs the histogram is the same
    rc, h, _, _, _, _ = GR.run_c(case, [pl for _, pl in scen], [ed for ed, _ in scen], m, 11, 5, orders=False, delta=False,
                                 start=False, gain=False)
    assert rc == 0 and np.array_equal(h, whole['hist'])


def test_run_grids_on_all_devices_gives_device_0s_counts(require_gpu):
    c = O.load_case('S60')
    d = list(c['grid_probs'])
    args = (c['base_pace'], c['tire_deg'], c['driver_variance'], c['driver_dnf_rates'])
    edits = {'forecast': [], 'new engine': [GridEdit.drop(d[0], 'engine')], 'pit lane': [GridEdit.pit_lane(d[0])]}
    res = {}
    for device in (0, 'all'):
        sim = RaceSimulator(RaceConfig(**c['config']), set_pop=DEFAULT_SET_POP, device=device)
        res[device] = sim.run_grids(3000, edits, None, *args, grid_probs=c['grid_probs'], seed=9, return_orders=True)
    one, every = res[0], res['all']
    for k in ('hist', 'delta', 'start', 'gain', 'orders'):
        assert np.array_equal(getattr(one, k), getattr(every, k)), k
    assert one.names == ['forecast', 'new engine', 'pit lane'] and (one.start.sum(axis=2) == 3000).all()
    assert one.expected_start('pit lane')[d[0]] == len(d) and one.expected_start('new engine')[d[0]] > one.expected_start('forecast')[d[0]]
    assert one.compare('pit lane', d[0])['mean_gain'] < 0
