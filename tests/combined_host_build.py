"""Host DEBUGGING build of csrc/scenario.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_scenario_kernel<false / true, kRuleAll> and the three rule sets' counting kernels on the CPU and decode the raw stagings
by the layouts documented at the top of scenario.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never
imports this and has no CPU path."""
import ctypes as C

import numpy as np

import combined_ref as CR
import events_ref as ER
import kernel_host_build as KH
import paces_host_build as PH
import paces_ref as PR
import penalties_ref as NR
import resume_ref as RR
import strategy_ref as SR

STAGE_FILL = 0xEE           # what the staging holds before the kernel runs (no staged byte has bit 7 set)
EV_FILL = 0xEEEEEEEE        # ... the staged event counts (bits 30-31 are never set)
CAR_FILL = 0xEEEE           # ... and the staged laps carried (no race has 0xEEEE laps)
PAD = 4096                  # bytes (u32s, u16s) of fill kept around the chunk


def lib():
    L = KH.generic_lib()
    L.emu_combined_run.restype = C.c_int
    return L


def combined_raw(case, scen, n_sims, seed, sim_offset=0, state=None, prob=None, grid_x=3, count=True, null_counts=False):
    """race_scenario_kernel with all three rule sets (and penalties_count, events_count, paces_count as blocks of one thread) on the host -> dict:
    hist [S][n][n], stage [S][n_sims][n], evs [S][n_sims], car [S][n_sims][n], delta [S][n][2n-1] without its derived
    centre bin, fate [S][n][4] and carried [S][n][L+1] without their derived column 0, events [S][3][L+1]; after checking
    that nothing is written before or past any of the three chunks, nor at a driver without an UNTIL_STOP offset."""
    p, g = prob or KH.generic_problem(case)
    n, S, L = p.n, len(scen), int(p.cfg.total_laps)
    counts, c_plans = SR.c_plans([sc['plans'] for sc in scen])
    tables = [NR.c_penalties([sc['penalties'] for sc in scen]), ER.c_events([sc['events'] for sc in scen]),
              PR.c_paces([sc['paces'] for sc in scen])]
    if null_counts:
        tables = [t if any(sc[k] for sc in scen) else (None, None)
                  for t, k in zip(tables, ('penalties', 'events', 'paces'))]
    cs = RR.c_state(*state) if state is not None else None
    used, words = S * n_sims * n, S * n_sims
    hist, err = np.zeros((S, n, n), np.uint64), C.c_char_p()
    stage = np.full(PAD + used + PAD, STAGE_FILL, np.uint8)
    evs = np.full(PAD + words + PAD, EV_FILL, np.uint32)
    cars = np.full(PAD + used + PAD, CAR_FILL, np.uint16)
    delta, fate = np.zeros((S, n, 2 * n - 1), np.uint64), np.zeros((S, n, 4), np.uint64)
    events, carried = np.zeros((S, 3, L + 1), np.uint64), np.zeros((S, n, L + 1), np.uint64)
    opt = lambda a: KH._vp(a) if count else None
    rc = lib().emu_combined_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                                C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint32(S), counts, c_plans,
                                tables[0][0], tables[0][1], tables[1][0], tables[1][1], tables[2][0], tables[2][1],
                                C.c_uint64(n_sims), C.c_uint64(sim_offset), C.c_uint64(seed), KH._vp(hist),
                                KH._vp(stage[PAD:]), KH._vp(evs[PAD:]), KH._vp(cars[PAD:]), opt(delta), opt(fate),
                                opt(events), opt(carried), C.c_uint32(grid_x), C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (stage[:PAD] == STAGE_FILL).all() and (stage[PAD + used:] == STAGE_FILL).all()      # nothing outside the chunk
    assert (evs[:PAD] == EV_FILL).all() and (evs[PAD + words:] == EV_FILL).all()
    assert (cars[:PAD] == CAR_FILL).all() and (cars[PAD + used:] == CAR_FILL).all()
    car = cars[PAD:PAD + used].reshape(S, n_sims, n).copy()
    written = np.broadcast_to(PH.until_mask([sc['paces'] for sc in scen], n)[:, None, :], car.shape)
    assert (car[~written] == CAR_FILL).all() and (car[written] <= L).all()
    return dict(hist=hist.astype(np.int64), stage=stage[PAD:PAD + used].reshape(S, n_sims, n).copy(),
                evs=evs[PAD:PAD + words].reshape(S, n_sims).copy(), car=car, delta=delta.astype(np.int64),
                fate=fate.astype(np.int64), events=events.astype(np.int64), carried=carried.astype(np.int64))


def decode(stage, evs, car):
    """(orders [S][m][n], fates [S][m][n], event laps [S][m][3], laps carried [S][m][n]) of the three stagings."""
    n = stage.shape[2]
    assert (stage >> 7 == 0).all()
    pos = stage & 31
    assert (np.sort(pos, axis=2) == np.arange(n, dtype=np.uint8)).all()            # every row a permutation
    assert ((evs >> 30) == 0).all()
    seen = np.stack([(evs >> (10 * k)) & 1023 for k in range(3)], axis=2).astype(np.int64)
    return (np.argsort(pos, axis=2).astype(np.uint8), (stage >> 5) & 3, seen,
            np.where(car == CAR_FILL, 0, car).astype(np.int64))


def combined(case, scen, n_sims, seed, sim_offset=0, state=None, prob=None, null_counts=False):
    """-> dict(hist, orders, fates, seen, laps, delta, fate, events, carried): the emulated kernels' outputs with the
    host's derived centre bin and columns 0 filled in as the C ABI fills them."""
    r = combined_raw(case, scen, n_sims, seed, sim_offset, state, prob, null_counts=null_counts)
    orders, fates, seen, laps = decode(r['stage'], r['evs'], r['car'])
    n = orders.shape[2]
    delta, fate, carried = r['delta'], r['fate'], r['carried']
    assert (delta[:, :, n - 1] == 0).all() and (fate[:, :, 0] == 0).all() and (carried[:, :, 0] == 0).all()
    delta[:, :, n - 1] = n_sims - delta.sum(axis=2)
    fate[:, :, 0] = n_sims - fate.sum(axis=2)
    carried[:, :, 0] = n_sims - carried.sum(axis=2)
    return dict(hist=r['hist'], orders=orders, fates=fates, seen=seen, laps=laps, delta=delta, fate=fate,
                events=r['events'], carried=carried)


def check_against(got, case, want, m):
    """The outputs `got` (combined() here, or the C call's) against the restatement's (orders, fates, seen, carried) of
    combined_ref.ref_run: every order, and every count as the count of the restatement's per-simulation results."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    want_o, want_f, want_e, want_c = want
    for s in range(want_o.shape[0]):
        bad = [i for i in range(m) if not np.array_equal(got['orders'][s, i], want_o[s, i])]
        assert not bad, f'scenario {s}: {len(bad)} of {m} orders differ, first sim {bad[0]}'
    assert np.array_equal(got['hist'], NR.hist_counts(want_o, n))
    assert np.array_equal(got['delta'], SR.delta_counts(want_o, n))
    assert np.array_equal(got['fate'], NR.fate_counts(want_f, n))
    assert np.array_equal(got['events'], ER.event_counts(want_e, L))
    assert np.array_equal(got['carried'], PR.carried_counts(want_c, L))
    for k in ('fate', 'events', 'carried'):
        assert (got[k].sum(axis=2) == m).all(), k
