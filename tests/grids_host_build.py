"""Host DEBUGGING build of csrc/grids.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_scenario_kernel<false, kRuleGrid> and grid_count on the CPU and decode the raw staging by the layout documented at
the top of grids.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no CPU
path."""
import ctypes as C

import numpy as np

import grids_ref as GR
import kernel_host_build as KH
import strategy_ref as SR

STAGE_FILL = 0xEE           # what the staging holds before the kernel runs (no position is 0xEE)
CAR_FILL = 0xEEEE           # ... and the staged start slots (no slot is 0xEEEE)
PAD = 4096                  # bytes (u16s) of fill kept around the chunk


def lib():
    L = KH.generic_lib()
    L.emu_grid_run.restype = C.c_int
    return L


def grids_raw(case, plans, edits, n_sims, seed, sim_offset=0, prob=None, grid_x=3, count=True, stage_start=True):
    """race_scenario_kernel with grid edits (and grid_count, as grid_x x S x n blocks of one thread) on the host -> (hist
    [S][n][n], stage [S][n_sims][n], car_stage [S][n_sims][n] or None, start [S][n][n], gain [S][n][2n-1]), after checking
    that nothing is written before or past the chunk and that every staged cell is written."""
    p, g = prob or KH.generic_problem(case)
    n, S = p.n, len(edits)
    plans = plans if plans is not None else [{}] * S
    counts, c_plans = SR.c_plans(plans)
    ecounts, c_ed = GR.c_edits(edits)
    used = S * n_sims * n
    hist, err = np.zeros((S, n, n), np.uint64), C.c_char_p()
    stage = np.full(PAD + used + PAD, STAGE_FILL, np.uint8)
    cars = np.full(PAD + used + PAD, CAR_FILL, np.uint16)
    start, gain = np.zeros((S, n, n), np.uint64), np.zeros((S, n, 2 * n - 1), np.uint64)
    counted = count and stage_start
    rc = lib().emu_grid_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g), C.c_uint32(n), C.c_uint32(S), counts, c_plans,
                            ecounts, c_ed, C.c_uint64(n_sims), C.c_uint64(sim_offset), C.c_uint64(seed), KH._vp(hist),
                            KH._vp(stage[PAD:]), KH._vp(cars[PAD:]) if stage_start else None,
                            KH._vp(start) if counted else None, KH._vp(gain) if counted else None, C.c_uint32(grid_x),
                            C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (stage[:PAD] == STAGE_FILL).all() and (stage[PAD + used:] == STAGE_FILL).all()      # nothing outside the chunk
    assert (cars[:PAD] == CAR_FILL).all() and (cars[PAD + used:] == CAR_FILL).all()
    car = cars[PAD:PAD + used].reshape(S, n_sims, n).copy()
    if stage_start:
        assert (car < n).all()                                  # every cell written, with a slot of the grid
    else:
        assert (car == CAR_FILL).all()                          # a NULL staging is not written
    return (hist.astype(np.int64), stage[PAD:PAD + used].reshape(S, n_sims, n).copy(), car if stage_start else None,
            start.astype(np.int64), gain.astype(np.int64))


def decode(stage):
    """Finishing orders [S][m][n] of the staged positions."""
    n = stage.shape[2]
    assert (np.sort(stage, axis=2) == np.arange(n, dtype=np.uint8)).all()          # every row a permutation
    return np.argsort(stage, axis=2).astype(np.uint8)


def grids(case, plans, edits, n_sims, seed, sim_offset=0, prob=None):
    """-> dict(hist, orders, slots, delta, start, gain): the emulated kernels' outputs, and delta counted from the staged
    positions (strategy_count_deltas is written for its fixed block of 256 threads and runs on the device only)."""
    hist, stage, car, start, gain = grids_raw(case, plans, edits, n_sims, seed, sim_offset, prob)
    orders = decode(stage)
    return dict(hist=hist, orders=orders, slots=car.astype(np.int64), delta=SR.delta_counts(orders, stage.shape[2]),
                start=start, gain=gain)
