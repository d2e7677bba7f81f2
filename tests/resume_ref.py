"""Race states for the tests of mcgp_run_from_state / RaceSimulator.run_from_state, taken from the CPU oracle's per-lap
trace (orc_run's orc_trace and grids): the state of simulation i after lap k, whose continuation as simulation i must
be the oracle's finishing order of i.  Also the numpy restatement of the retirement chains (race_common.hip.h)."""
import ctypes as C
import math

import numpy as np

import oracle_py as O
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import RaceState, _Problem
from monte_carlo_gp_amd import RaceConfig

SET_POP = O.load_cases()['set_pop']
PURPOSE_EVENT = 1 << 16
PURPOSE_RETIRE = 4 << 16


def threshold(p):
    """u < p for u = w / 2^32  <=>  w < ceil(p 2^32)  (params_build.h)."""
    if not p > 0:
        return 0
    return min(2 ** 32, math.ceil(p * 2.0 ** 32))


def field_case(n):
    """An n-car field with S60's parameters and 25 laps (the builder of test_gpu_matchups._field)."""
    rng = np.random.default_rng(n)
    drivers = [f'D{i:02d}' for i in range(n)]
    base = O.load_case('S60')
    case = dict(base)
    case['config'] = dict(base['config'], total_laps=25,
                          driver_teams={d: list(base['config']['dnf_rates'])[i % 10] for i, d in enumerate(drivers)})
    g = rng.random((n, n))
    g[:, n // 2] = 0.0
    case['grid_probs'] = {d: [float(x) for x in g[i]] for i, d in enumerate(drivers)}
    case['base_pace'] = {d: 90.0 + 0.2 * i for i, d in enumerate(drivers)}
    case['tire_deg'] = {d: 0.05 for d in drivers}
    case['driver_variance'] = {d: 0.2 for d in drivers}
    case['driver_dnf_rates'] = {d: 0.01 for d in drivers}
    return case


def lap_event(case, seed, sim, lap):
    """Laps DRS stays off after `lap`'s race event (red flag, safety car: 2; VSC: 1), 0 without one: the short-circuit
    chain of the event draws, counter {sim, lap, EVENT}."""
    cfg = case['config']
    e = O.philox([sim & 0xFFFFFFFF, sim >> 32, lap, PURPOSE_EVENT], [seed & 0xFFFFFFFF, seed >> 32])
    if e[0] < threshold(cfg['red_flag_probability']):
        return 2
    if e[1] < threshold(cfg['sc_probability']):
        return 2
    if e[2] < threshold(cfg['vsc_probability']):
        return 1
    return 0


def drs_disabled_until(case, seed, sim, k):
    """simulate_race's drs_disabled_until after lap k of simulation `sim` (events of laps 2 .. k replayed)."""
    dd = 0
    for lap in range(2, k + 1):
        inc = lap_event(case, seed, sim, lap)
        if inc:
            dd = lap + inc
    return dd


def first_event_lap(case, seed, sim):
    for lap in range(2, case['config']['total_laps'] + 1):
        if lap_event(case, seed, sim, lap):
            return lap
    return None


def traced_run(case, m, seed, sim_offset=0):
    """The oracle's run of m simulations with orders, grids and the per-lap trace of all of them."""
    return O.Problem(case).run(m, rng=O.RNG_PHILOX, seed=seed, sim_offset=sim_offset, want_orders=True, want_grids=True,
                               n_trace=m)


def state_arrays(ref, i, k):
    """The mcgp_race_state arrays (driver-index order) of traced simulation i after lap k."""
    tr = ref['trace']
    grid = ref['grids'][i]
    slot = np.zeros(len(grid), np.uint8)
    slot[grid] = np.arange(len(grid), dtype=np.uint8)
    retired = np.where(tr['dnf'][i, k - 1] != 0, tr['dnf_lap'][i, k - 1], 0).astype(np.int16)
    return dict(cumulative_time=np.ascontiguousarray(tr['cum'][i, k - 1], np.float64),
                last_lap_time=np.ascontiguousarray(tr['last'][i, k - 1], np.float64),
                grid_slot=slot, compound=np.ascontiguousarray(tr['comp'][i, k - 1], np.uint8),
                used_compounds=np.ascontiguousarray(tr['used'][i, k - 1], np.uint8),
                tire_age=np.ascontiguousarray(tr['age'][i, k - 1], np.int16), retired_lap=retired)


def race_state(arrays, lap, dd, drivers):
    """A RaceState (cars in grid order) from mcgp_race_state arrays."""
    by_slot = np.argsort(arrays['grid_slot'])
    obj = {'lap': int(lap), 'drs_disabled_until': int(dd), 'cars': [
        {'driver': drivers[d], 'cumulative_time': float(arrays['cumulative_time'][d]),
         'last_lap_time': float(arrays['last_lap_time'][d]),
         'tire_compound': N.COMPOUNDS[int(arrays['compound'][d])], 'tire_age': int(arrays['tire_age'][d]),
         'used_compounds': [c for j, c in enumerate(N.COMPOUNDS) if (int(arrays['used_compounds'][d]) >> j) & 1],
         'retired_lap': int(arrays['retired_lap'][d])} for d in by_slot]}
    return RaceState.from_json(obj)


def problem(case):
    return _Problem(RaceConfig(**case['config']), list(case['grid_probs']), case['base_pace'], case['tire_deg'],
                    case['driver_variance'], case['driver_dnf_rates'], case['track_condition'], SET_POP)


def c_state(arrays, lap, dd):
    p = lambda k, t: arrays[k].ctypes.data_as(C.POINTER(t))
    return N.McgpRaceState(lap=int(lap), drs_disabled_until=int(dd),
                           cumulative_time=p('cumulative_time', C.c_double), last_lap_time=p('last_lap_time', C.c_double),
                           grid_slot=p('grid_slot', C.c_uint8), compound=p('compound', C.c_uint8),
                           used_compounds=p('used_compounds', C.c_uint8), tire_age=p('tire_age', C.c_int16),
                           retired_lap=p('retired_lap', C.c_int16))


def run_c(prob, states, n_sims, sim_offsets, seed, orders=True, device=0):
    """mcgp_run_from_state: states = [(arrays, lap, drs_disabled_until)] -> (rc, hist [S][n][n], orders [S][N][n])."""
    S, n = len(states), prob.n
    cs = (N.McgpRaceState * S)(*[c_state(a, k, dd) for a, k, dd in states])
    offs = (C.c_uint64 * S)(*[int(x) for x in sim_offsets]) if sim_offsets is not None else None
    hist = np.zeros((S, n, n), np.uint64)
    o = np.zeros((S, n_sims, n), np.uint8) if orders else None
    rc = N.lib().mcgp_run_from_state(C.byref(prob.cfg), C.byref(prob.drv), n, S, cs, int(n_sims), offs, int(seed),
                                     device, hist.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     o.ctypes.data_as(C.POINTER(C.c_uint8)) if orders else None)
    return rc, hist.astype(np.int64), o


def counts(orders, n):
    """[driver][position] counts of finishing orders [m][n]."""
    h = np.zeros((n, n), np.int64)
    for p in range(n):
        np.add.at(h[:, p], orders[:, p], 1)
    return h


# ---- numpy restatement of the retirement chains of race_common.hip.h
def retirement_lap(w, t, L):
    """draw_retirement_lap: the lap (2 .. L) on which the chain S_2 = q, S_{j+1} = floor(S_j q / 2^32) first has
    w >= S, or 0."""
    if t == 0:
        return 0
    q = 2 ** 32 - t
    S = q
    for lap in range(2, L + 1):
        if not w < S:
            return lap
        S = (S * q) >> 32
    return 0


def retirement_lap_after(w, t, k, L):
    """draw_retirement_lap_after: the same chain shifted to start at lap k + 1 (k + 1 .. L), or 0."""
    r = retirement_lap(w, t, L - k + 1)
    return 0 if r == 0 else k - 1 + r
