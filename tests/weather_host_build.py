"""Host DEBUGGING build of csrc/weather.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_scenario_kernel<false / true, kRuleWeather> and weather_count on the CPU and decode the raw staging by the layout
documented at the top of weather.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this
and has no CPU path."""
import ctypes as C

import numpy as np

import kernel_host_build as KH
import resume_ref as RR
import strategy_ref as SR
import weather_ref as WR

STAGE_FILL = 0xEE           # what the staging holds before the kernel runs (no position is 0xEE)
CAR_FILL = 0xEEEE           # ... and the staged laps on the wrong tyres (no race has 0xEEEE laps)
PAD = 4096                  # bytes (u16s) of fill kept around the chunk


def lib():
    L = KH.generic_lib()
    L.emu_weather_run.restype = C.c_int
    return L


def weather_raw(case, plans, changes, table, n_sims, seed, sim_offset=0, state=None, prob=None, grid_x=3, count=True,
                stage_wrong=True):
    """race_scenario_kernel with weather (and weather_count, as grid_x x S x n blocks of one thread) on the host -> (hist
    [S][n][n], stage [S][n_sims][n], car_stage [S][n_sims][n] or None, wrong [S][n][L+1] without its derived column 0),
    after checking that nothing is written before or past the chunk and that every staged cell is written."""
    p, g = prob or KH.generic_problem(case)
    n, S, L = p.n, len(changes), int(p.cfg.total_laps)
    plans = plans if plans is not None else [{}] * S
    counts, c_plans = SR.c_plans(plans)
    ccounts, c_ch = WR.c_changes(changes)
    model = WR.c_model(table)
    cs = RR.c_state(*state) if state is not None else None
    used = S * n_sims * n
    hist, err = np.zeros((S, n, n), np.uint64), C.c_char_p()
    stage = np.full(PAD + used + PAD, STAGE_FILL, np.uint8)
    cars = np.full(PAD + used + PAD, CAR_FILL, np.uint16)
    wrong = np.zeros((S, n, L + 1), np.uint64)
    rc = lib().emu_weather_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                               C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint32(S), counts, c_plans,
                               ccounts, c_ch, C.byref(model), C.c_uint64(n_sims), C.c_uint64(sim_offset),
                               C.c_uint64(seed), KH._vp(hist), KH._vp(stage[PAD:]),
                               KH._vp(cars[PAD:]) if stage_wrong else None,
                               KH._vp(wrong) if count and stage_wrong else None, C.c_uint32(grid_x), C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (stage[:PAD] == STAGE_FILL).all() and (stage[PAD + used:] == STAGE_FILL).all()      # nothing outside the chunk
    assert (cars[:PAD] == CAR_FILL).all() and (cars[PAD + used:] == CAR_FILL).all()
    car = cars[PAD:PAD + used].reshape(S, n_sims, n).copy()
    if stage_wrong:
        assert (car <= L).all()                                 # every cell written, none past the race's laps
    else:
        assert (car == CAR_FILL).all()                          # a NULL staging is not written
    return (hist.astype(np.int64), stage[PAD:PAD + used].reshape(S, n_sims, n).copy(), car if stage_wrong else None,
            wrong.astype(np.int64))


def decode(stage):
    """Finishing orders [S][m][n] of the staged positions."""
    n = stage.shape[2]
    assert (np.sort(stage, axis=2) == np.arange(n, dtype=np.uint8)).all()          # every row a permutation
    return np.argsort(stage, axis=2).astype(np.uint8)


def weather(case, plans, changes, table, n_sims, seed, sim_offset=0, state=None, prob=None):
    """-> dict(hist, orders, laps, delta, wrong_laps): the emulated kernels' outputs with the host's derived column 0 filled
    in as the C ABI fills it, and delta counted from the staged positions (strategy_count_deltas is written for its fixed
    block of 256 threads and runs on the device only)."""
    hist, stage, car, wrong = weather_raw(case, plans, changes, table, n_sims, seed, sim_offset, state, prob)
    orders = decode(stage)
    assert (wrong[:, :, 0] == 0).all()
    wrong[:, :, 0] = n_sims - wrong.sum(axis=2)
    return dict(hist=hist, orders=orders, laps=car.astype(np.int64), delta=SR.delta_counts(orders, stage.shape[2]),
                wrong_laps=wrong)
