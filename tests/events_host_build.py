"""Host DEBUGGING build of csrc/events.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_scenario_kernel<false / true, kRuleEvents> and events_count on the CPU and decode the raw staging by the layout documented at the
top of events.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no CPU
path."""
import ctypes as C

import numpy as np

import events_ref as ER
import kernel_host_build as KH
import resume_ref as RR
import strategy_ref as SR

STAGE_FILL = 0xEE           # what the staging holds before the kernel runs (no position is 0xEE)
EV_FILL = 0xEEEEEEEE        # ... and the staged event counts (bits 30-31 of a staged word stay 0)
PAD = 4096                  # bytes (words) of fill kept around the chunk


def lib():
    L = KH.generic_lib()
    L.emu_events_run.restype = C.c_int
    return L


def events_raw(case, plans, overrides, n_sims, seed, sim_offset=0, state=None, prob=None, grid_x=3, count=True):
    """race_scenario_kernel with events (and events_count, as grid_x x S blocks of one thread) on the host -> (hist [S][n][n], stage
    [S][n_sims][n], ev_stage [S][n_sims], delta [S][n][2n-1] without its derived centre bin, events [S][3][L+1]), after
    checking that nothing is written before or past the chunk."""
    p, g = prob or KH.generic_problem(case)
    n, S, L = p.n, len(overrides), int(p.cfg.total_laps)
    plans = plans if plans is not None else [{}] * S
    counts, c_plans = SR.c_plans(plans)
    ecounts, c_evs = ER.c_events(overrides)
    cs = RR.c_state(*state) if state is not None else None
    used, words = S * n_sims * n, S * n_sims
    hist, err = np.zeros((S, n, n), np.uint64), C.c_char_p()
    stage = np.full(PAD + used + PAD, STAGE_FILL, np.uint8)
    evs = np.full(PAD + words + PAD, EV_FILL, np.uint32)
    delta, events = np.zeros((S, n, 2 * n - 1), np.uint64), np.zeros((S, 3, L + 1), np.uint64)
    rc = lib().emu_events_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                              C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint32(S), counts, c_plans,
                              ecounts, c_evs, C.c_uint64(n_sims), C.c_uint64(sim_offset), C.c_uint64(seed),
                              KH._vp(hist), KH._vp(stage[PAD:]), KH._vp(evs[PAD:]), KH._vp(delta) if count else None,
                              KH._vp(events) if count else None, C.c_uint32(grid_x), C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (stage[:PAD] == STAGE_FILL).all() and (stage[PAD + used:] == STAGE_FILL).all()      # nothing outside the chunk
    assert (evs[:PAD] == EV_FILL).all() and (evs[PAD + words:] == EV_FILL).all()
    return (hist.astype(np.int64), stage[PAD:PAD + used].reshape(S, n_sims, n).copy(),
            evs[PAD:PAD + words].reshape(S, n_sims).copy(), delta.astype(np.int64), events.astype(np.int64))


def decode(stage, evs):
    """(orders [S][m][n], event laps [S][m][3]) of the staged positions [S][m][n] and packed counts [S][m]."""
    n = stage.shape[2]
    assert (np.sort(stage, axis=2) == np.arange(n, dtype=np.uint8)).all()          # every row a permutation
    assert ((evs >> 30) == 0).all()
    seen = np.stack([(evs >> (10 * k)) & 1023 for k in range(3)], axis=2).astype(np.int64)
    return np.argsort(stage, axis=2).astype(np.uint8), seen


def events(case, plans, overrides, n_sims, seed, sim_offset=0, state=None, prob=None):
    """-> dict(hist, orders, seen, delta, events): the emulated kernels' outputs with the host's derived centre bin
    filled in as the C ABI fills it."""
    hist, stage, evs, delta, ev = events_raw(case, plans, overrides, n_sims, seed, sim_offset, state, prob)
    orders, seen = decode(stage, evs)
    n = stage.shape[2]
    assert (delta[:, :, n - 1] == 0).all()
    delta[:, :, n - 1] = n_sims - delta.sum(axis=2)
    return dict(hist=hist, orders=orders, seen=seen, delta=delta, events=ev)
