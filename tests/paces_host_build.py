"""Host DEBUGGING build of csrc/paces.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_scenario_kernel<false / true, kRulePaces> and paces_count on the CPU and decode the raw staging by the layout documented at the
top of paces.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no CPU
path."""
import ctypes as C

import numpy as np

import kernel_host_build as KH
import paces_ref as PR
import resume_ref as RR
import strategy_ref as SR

STAGE_FILL = 0xEE           # what the staging holds before the kernel runs (no position is 0xEE)
CAR_FILL = 0xEEEE           # ... and the staged laps carried (no race has 0xEEEE laps)
PAD = 4096                  # bytes (u16s) of fill kept around the chunk


def lib():
    L = KH.generic_lib()
    L.emu_paces_run.restype = C.c_int
    return L


def until_mask(offsets, n):
    """[S][n] bool: the drivers with an UNTIL_STOP offset in each scenario."""
    out = np.zeros((len(offsets), n), bool)
    for s, offs in enumerate(offsets):
        for d, kind, *_ in offs:
            if kind == PR.UNTIL_STOP:
                out[s, d] = True
    return out


def paces_raw(case, plans, offsets, n_sims, seed, sim_offset=0, state=None, prob=None, grid_x=3, count=True):
    """race_scenario_kernel with paces (and paces_count, as grid_x x S x (1 + n) blocks of one thread) on the host -> (hist [S][n][n],
    stage [S][n_sims][n], car_stage [S][n_sims][n], delta [S][n][2n-1] without its derived centre bin, carried
    [S][n][L+1] without its derived column 0), after checking that nothing is written before or past the chunk, nor at a
    driver without an UNTIL_STOP offset."""
    p, g = prob or KH.generic_problem(case)
    n, S, L = p.n, len(offsets), int(p.cfg.total_laps)
    plans = plans if plans is not None else [{}] * S
    counts, c_plans = SR.c_plans(plans)
    pcounts, c_offs = PR.c_paces(offsets)
    cs = RR.c_state(*state) if state is not None else None
    used = S * n_sims * n
    hist, err = np.zeros((S, n, n), np.uint64), C.c_char_p()
    stage = np.full(PAD + used + PAD, STAGE_FILL, np.uint8)
    cars = np.full(PAD + used + PAD, CAR_FILL, np.uint16)
    delta, carried = np.zeros((S, n, 2 * n - 1), np.uint64), np.zeros((S, n, L + 1), np.uint64)
    rc = lib().emu_paces_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                             C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint32(S), counts, c_plans,
                             pcounts, c_offs, C.c_uint64(n_sims), C.c_uint64(sim_offset), C.c_uint64(seed),
                             KH._vp(hist), KH._vp(stage[PAD:]), KH._vp(cars[PAD:]), KH._vp(delta) if count else None,
                             KH._vp(carried) if count else None, C.c_uint32(grid_x), C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (stage[:PAD] == STAGE_FILL).all() and (stage[PAD + used:] == STAGE_FILL).all()      # nothing outside the chunk
    assert (cars[:PAD] == CAR_FILL).all() and (cars[PAD + used:] == CAR_FILL).all()
    car = cars[PAD:PAD + used].reshape(S, n_sims, n).copy()
    written = np.broadcast_to(until_mask(offsets, n)[:, None, :], car.shape)
    assert (car[~written] == CAR_FILL).all() and (car[written] <= L).all()
    return (hist.astype(np.int64), stage[PAD:PAD + used].reshape(S, n_sims, n).copy(), car, delta.astype(np.int64),
            carried.astype(np.int64))


def decode(stage, car):
    """(orders [S][m][n], laps carried [S][m][n]: 0 where the driver has no UNTIL_STOP offset) of the staged positions
    and u16s."""
    n = stage.shape[2]
    assert (np.sort(stage, axis=2) == np.arange(n, dtype=np.uint8)).all()          # every row a permutation
    return np.argsort(stage, axis=2).astype(np.uint8), np.where(car == CAR_FILL, 0, car).astype(np.int64)


def paces(case, plans, offsets, n_sims, seed, sim_offset=0, state=None, prob=None):
    """-> dict(hist, orders, laps, delta, carried): the emulated kernels' outputs with the host's derived centre bin and
    column 0 filled in as the C ABI fills them."""
    hist, stage, car, delta, carried = paces_raw(case, plans, offsets, n_sims, seed, sim_offset, state, prob)
    orders, laps = decode(stage, car)
    n = stage.shape[2]
    assert (delta[:, :, n - 1] == 0).all() and (carried[:, :, 0] == 0).all()
    delta[:, :, n - 1] = n_sims - delta.sum(axis=2)
    carried[:, :, 0] = n_sims - carried.sum(axis=2)
    return dict(hist=hist, orders=orders, laps=laps, delta=delta, carried=carried)
