"""RaceSimulator.run_*: what each method hands to the C ABI and how it puts the shards' results together, without a
device.  `_native.lib` is replaced by a recorder that keeps every call's arguments (scalars, and copies of the input
arrays) and writes a pattern derived from (entry point, sim_offset, count) into every output that is not NULL.  Each
method runs on one device and on three (7 simulations: ragged shards); the results must be the sum -- for finishing
orders the concatenation -- of the shards' patterns, and a shard's failure must surface with its own message."""
import ctypes as C
import threading

import numpy as np
import pytest

from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd import conditions as CD
from monte_carlo_gp_amd.simulation import (CarState, PitPlan, RaceConfig, RaceEvent, RaceSimulator, RaceState,
                                           TimePenalty)

DRIVERS = ['A', 'B', 'C']
n, L, SIMS, OFFSET, SEED = 3, 5, 7, 11, 5
ENTRY_ID = {name: i + 1 for i, name in enumerate(
    ('mcgp_run', 'mcgp_run_matchups', 'mcgp_run_trace', 'mcgp_run_from_state', 'mcgp_run_strategies',
     'mcgp_run_penalties', 'mcgp_run_events', 'mcgp_run_gaps', 'mcgp_run_stints', 'mcgp_run_moves',
     'mcgp_run_conditions'))}


def pattern(entry, k, offset, count, shape):
    """What the recorder writes into output `k` (in the order of the C arguments) of a call of `entry`."""
    size = int(np.prod(shape))
    v = np.arange(size, dtype=np.uint64) * np.uint64(k + 2) + np.uint64(ENTRY_ID[entry] * 100003 + offset * 17 + count)
    return v.reshape(shape)


def order_pattern(entry, offset, count, shape):
    v = (np.arange(int(np.prod(shape)), dtype=np.int64) * 3 + ENTRY_ID[entry] + 5 * offset + count) % 251
    return v.astype(np.uint8).reshape(shape)


def _vec(ptr, count, dtype=None):
    """A copy of `count` items behind a ctypes pointer or array (None for NULL)."""
    if ptr is None or count == 0:
        return None
    return np.array([ptr[i] for i in range(count)], dtype)


def _struct(s):
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        out[name] = list(v) if isinstance(v, C.Array) else v
    return out


class Recorder:
    """Stands in for the loaded library: the mcgp_run_* names of RaceSimulator's methods."""

    def __init__(self, fail_on_call=None):
        self.calls = []
        self.lock = threading.Lock()
        self.fail_on_call = fail_on_call          # this call (in order of arrival) returns -1 with a message
        self.err = threading.local()              # (mcgp_last_error is per thread in the library too)

    def mcgp_last_error(self):
        return getattr(self.err, 'msg', b'')

    def mcgp_device_count(self):
        return 1

    def _call(self, entry, cfg, drv, grid, state, offset, count, seed, device, inputs, outs, orders=None, states=1):
        cfg, drv = cfg._obj, drv._obj
        rec = dict(entry=entry, total_laps=cfg.total_laps, deviates=cfg.deviates, offset=int(offset), count=int(count),
                   seed=int(seed), device=int(device), grid=None if grid is None else _vec(grid, n * n).reshape(n, n),
                   base_pace=_vec(drv.base_pace, n), state=None, nulls=[k for k, (p, _) in enumerate(outs) if p is None],
                   **inputs)
        if state is not None:
            sts = [state._obj] if states == 1 and not isinstance(state, C.Array) else list(state)
            rec['state'] = [dict(lap=s.lap, drs_disabled_until=s.drs_disabled_until,
                                 **{k: _vec(getattr(s, k), n).tolist() for k, _ in N.McgpRaceState._fields_[2:]})
                            for s in sts]
        with self.lock:
            self.calls.append(rec)
            index = len(self.calls) - 1
        if index == self.fail_on_call:
            self.err.msg = f'shard at {offset} failed'.encode()
            return -1
        for k, (ptr, shape) in enumerate(outs):
            if ptr is not None:
                np.ctypeslib.as_array(ptr, shape)[...] += pattern(entry, k, rec['offset'], rec['count'], shape)
        if orders is not None and orders[0] is not None:
            np.ctypeslib.as_array(orders[0], orders[1])[...] = order_pattern(entry, rec['offset'], rec['count'], orders[1])
        return 0

    def mcgp_run(self, cfg, drv, grid, n_, count, offset, seed, device, hist, orders):
        return self._call('mcgp_run', cfg, drv, grid, None, offset, count, seed, device, {}, [(hist, (n, n))],
                          (orders, (count, n)))

    def mcgp_run_matchups(self, cfg, drv, grid, n_, count, offset, seed, device, hist, ahead, podium):
        return self._call('mcgp_run_matchups', cfg, drv, grid, None, offset, count, seed, device, {},
                          [(hist, (n, n)), (ahead, (n, n)), (podium, (n, n, n))])

    def mcgp_run_trace(self, cfg, drv, grid, n_, count, offset, seed, device, hist, lap_pos, led, stops, fastest, events):
        return self._call('mcgp_run_trace', cfg, drv, grid, None, offset, count, seed, device, {},
                          [(hist, (n, n)), (lap_pos, (L, n, n + 1)), (led, (n, L + 1)), (stops, (n, L + 1)),
                           (fastest, (n,)), (events, (3, L + 1))])

    def mcgp_run_from_state(self, cfg, drv, n_, S, states, count, offsets, seed, device, hist, orders):
        return self._call('mcgp_run_from_state', cfg, drv, None, states, offsets[0], count, seed, device,
                          dict(sim_offsets=_vec(offsets, S).tolist()), [(hist, (S, n, n))], (orders, (S, count, n)),
                          states=S)

    def _scenarios(self, entry, cfg, drv, grid, state, S, plan_count, plans, extra, count, offset, seed, device, outs, orders):
        counts = _vec(plan_count, S).tolist()
        inputs = dict(S=S, plan_count=counts, plans=[_struct(plans[i]) for i in range(sum(counts))], **extra)
        return self._call(entry, cfg, drv, grid, state, offset, count, seed, device, inputs, outs, (orders, (S, count, n)))

    def mcgp_run_strategies(self, cfg, drv, grid, state, n_, S, plan_count, plans, count, offset, seed, device, hist,
                            delta, orders):
        return self._scenarios('mcgp_run_strategies', cfg, drv, grid, state, S, plan_count, plans, {}, count, offset, seed,
                               device, [(hist, (S, n, n)), (delta, (S, n, 2 * n - 1))], orders)

    def mcgp_run_penalties(self, cfg, drv, grid, state, n_, S, plan_count, plans, pen_count, pens, count, offset, seed,
                           device, hist, delta, fate, orders):
        pc = _vec(pen_count, S).tolist()
        extra = dict(item_count=pc, items=[_struct(pens[i]) for i in range(sum(pc))])
        return self._scenarios('mcgp_run_penalties', cfg, drv, grid, state, S, plan_count, plans, extra, count, offset,
                               seed, device, [(hist, (S, n, n)), (delta, (S, n, 2 * n - 1)), (fate, (S, n, 4))], orders)

    def mcgp_run_events(self, cfg, drv, grid, state, n_, S, plan_count, plans, ev_count, evs, count, offset, seed, device,
                        hist, delta, events, orders):
        ec = _vec(ev_count, S).tolist()
        extra = dict(item_count=ec, items=[_struct(evs[i]) for i in range(sum(ec))])
        return self._scenarios('mcgp_run_events', cfg, drv, grid, state, S, plan_count, plans, extra, count, offset, seed,
                               device, [(hist, (S, n, n)), (delta, (S, n, 2 * n - 1)), (events, (S, 3, L + 1))], orders)

    def mcgp_run_gaps(self, cfg, drv, grid, state, n_, E, edges, P, pairs, count, offset, seed, device, hist, lap_gap,
                      lead, pair):
        inputs = dict(edges=_vec(edges, E).tolist(), pairs=None if pairs is None else _vec(pairs, 2 * P).tolist())
        return self._call('mcgp_run_gaps', cfg, drv, grid, state, offset, count, seed, device, inputs,
                          [(hist, (n, n)), (lap_gap, (L, n, E + 2)), (lead, (L, E + 2)), (pair, (L, P, 2 * E + 3))])

    def mcgp_run_stints(self, cfg, drv, grid, state, n_, count, offset, seed, device, hist, stop_lap, stops_pos, seq):
        return self._call('mcgp_run_stints', cfg, drv, grid, state, offset, count, seed, device, {},
                          [(hist, (n, n)), (stop_lap, (n, N.STINT_STOPS, L + 1)), (stops_pos, (n, N.STINT_STOPS + 1, n)),
                           (seq, (n, N.STINT_SEQ_CODES))])

    def mcgp_run_moves(self, cfg, drv, grid, state, n_, count, offset, seed, device, hist, grid_fin, start_gain, passes,
                       race_passes, lap_passes, pair_passes):
        return self._call('mcgp_run_moves', cfg, drv, grid, state, offset, count, seed, device, {},
                          [(hist, (n, n)), (grid_fin, (n, n, n)), (start_gain, (n, 2 * n)),
                           (passes, (n, len(N.MOVE_KINDS), N.MOVE_DRIVER_CAP + 1)), (race_passes, (N.MOVE_RACE_CAP + 1,)),
                           (lap_passes, (L + 1, 2)), (pair_passes, (n, n))])

    def mcgp_run_conditions(self, cfg, drv, grid, state, n_, K, table, count, offset, seed, device, hist, cnt, cond_hist):
        inputs = dict(conditions=[(table[i].n_atoms, [_struct(table[i].atom[j]) for j in range(table[i].n_atoms)])
                                  for i in range(K)])
        return self._call('mcgp_run_conditions', cfg, drv, grid, state, offset, count, seed, device, inputs,
                          [(hist, (n, n)), (cnt, (K,)), (cond_hist, (K, n, n))])


# ------------------------------------------------------------------------------------------------ the calls' inputs
GRID = {'A': [0.6, 0.3, 0.1], 'B': [0.3, 0.4, 0.3], 'C': [0.1, 0.3, 0.6]}
GRID_MATRIX = np.array([GRID[d] for d in DRIVERS])
PACE = {'A': 90.0, 'B': 90.5, 'C': 91.0}
RACE = dict(base_pace=PACE, tire_deg={d: 0.05 for d in DRIVERS}, driver_variance={d: 0.2 for d in DRIVERS})


def make_state(lap=2, swap=False):
    order = ['B', 'A', 'C'] if swap else ['A', 'B', 'C']
    cars = [CarState(driver=d, team='', position=i + 1, lap=lap, tire_compound='SOFT' if d == 'A' else 'MEDIUM',
                     tire_age=3 + i, fuel_load=100.0, time_behind_leader=0.0, pit_stops=0,
                     cumulative_time=180.0 + i, last_lap_time=90.0 + i, used_compounds={'HARD'} if d == 'C' else set())
            for i, d in enumerate(order)]
    return RaceState(lap=lap, drs_disabled_until=3, cars=cars)


def expected_state(state):
    a = state.arrays(DRIVERS, L)
    return dict(lap=state.lap, drs_disabled_until=state.drs_disabled_until, **{k: v.tolist() for k, v in a.items()})


def simulator(device):
    cfg = RaceConfig(total_laps=L, pit_loss=20.0, overtake_delta=0.3, sc_probability=0.02, vsc_probability=0.02,
                     red_flag_probability=0.0, dnf_rates={}, drs_zones=1, drs_delta=0.3,
                     tire_compounds={'SOFT': {}, 'MEDIUM': {}, 'HARD': {}}, driver_teams={})
    return RaceSimulator(cfg, device=device)


STATE, STATE2 = make_state(), make_state(3, swap=True)
PLANS = {'base': [], 'one': [PitPlan('A', [(3, 'HARD')], start='SOFT', start_age=1), PitPlan('C', [(2, 'SOFT'), (4, 'HARD')])]}
STATE_PLANS = {'p': [PitPlan('B', [(4, 'HARD')])]}
PENS = {'pen': [TimePenalty('B', 5.0), TimePenalty('A', 10.0, 'flag'), TimePenalty('A', 3.5, 'lap', 4)], 'clean': []}
EVENTS = {'sc': [RaceEvent('sc', 3, 4), RaceEvent('none', 2)], 'free': []}
CONDS = {'w': 'A.wins', 'wp': 'A.wins & B.podium'}


def plan_dict(driver, start, age, stops):
    laps, comps = [s[0] for s in stops], [N.COMPOUND_ID[s[1]] for s in stops]
    pad = N.MAX_PLAN_STOPS - len(stops)
    return dict(driver=driver, start_compound=start, start_age=age, n_stops=len(stops), stop_lap=laps + [0] * pad,
                stop_compound=comps + [0] * pad)


PLAN_ONE = [plan_dict(0, N.COMPOUND_ID['SOFT'], 1, [(3, 'HARD')]), plan_dict(2, -1, 0, [(2, 'SOFT'), (4, 'HARD')])]

# name -> (entry point, call, from a state?, names of the result's count arrays in the order of the C outputs, the
#          finishing orders' simulation axis or None, the call's own recorded inputs)
CASES = {
    'run_monte_carlo': ('mcgp_run', lambda s: s.run_monte_carlo(SIMS, GRID, **RACE, seed=SEED, sim_offset=OFFSET,
                                                                return_orders=True), None, ['hist'], 0, {}),
    'run_matchups': ('mcgp_run_matchups', lambda s: s.run_matchups(SIMS, GRID, **RACE, seed=SEED, sim_offset=OFFSET),
                     None, ['hist', 'ahead', 'podium'], None, {}),
    'run_trace': ('mcgp_run_trace', lambda s: s.run_trace(SIMS, GRID, **RACE, seed=SEED, sim_offset=OFFSET), None,
                  ['hist', 'lap_pos', 'laps_led', 'stops', 'fastest', 'events'], None, {}),
    'run_from_state': ('mcgp_run_from_state',
                       lambda s: s.run_from_state(SIMS, [STATE, STATE2], **RACE, seed=SEED, sim_offset=[OFFSET, 20],
                                                  drivers=DRIVERS, return_orders=True), [STATE, STATE2], ['hist'], 1, {}),
    'run_strategies': ('mcgp_run_strategies',
                       lambda s: s.run_strategies(SIMS, PLANS, **RACE, grid_probs=GRID, seed=SEED, sim_offset=OFFSET,
                                                  return_orders=True), None, ['hist', 'delta'], 1,
                       dict(S=2, plan_count=[0, 2], plans=PLAN_ONE)),
    'run_penalties': ('mcgp_run_penalties',
                      lambda s: s.run_penalties(SIMS, PENS, STATE_PLANS, **RACE, state=STATE, seed=SEED, sim_offset=OFFSET,
                                                drivers=DRIVERS, return_orders=True, allow_single_compound=True), [STATE],
                      ['hist', 'delta', 'fate'], 1,
                      dict(S=3, plan_count=[0, 0, 1], plans=[plan_dict(1, -1, 0, [(4, 'HARD')])], item_count=[3, 0, 0],
                           items=[dict(driver=1, kind=N.PEN_SERVE_AT_STOP, lap=3, seconds=5.0),
                                  dict(driver=0, kind=N.PEN_AT_FLAG, lap=0, seconds=10.0),
                                  dict(driver=0, kind=N.PEN_ON_LAP, lap=4, seconds=3.5)])),
    'run_events': ('mcgp_run_events',
                   lambda s: s.run_events(SIMS, EVENTS, PLANS, **RACE, grid_probs=GRID, seed=SEED, sim_offset=OFFSET), None,
                   ['hist', 'delta', 'events'], None,
                   dict(S=4, plan_count=[0, 0, 0, 2], plans=PLAN_ONE, item_count=[2, 0, 0, 0],
                        items=[dict(first_lap=3, last_lap=4, kind=N.EVT_SAFETY_CAR),
                               dict(first_lap=2, last_lap=2, kind=N.EVT_NONE)])),
    'run_gaps': ('mcgp_run_gaps',
                 lambda s: s.run_gaps(SIMS, GRID, **RACE, edges=[0.5, 2.0], pairs=[('C', 'A')], seed=SEED, sim_offset=OFFSET),
                 None, ['hist', 'lap_gap', 'lead', 'pair'], None, dict(edges=[0.5, 2.0], pairs=[2, 0])),
    'run_stints': ('mcgp_run_stints',
                   lambda s: s.run_stints(SIMS, **RACE, state=STATE, seed=SEED, sim_offset=OFFSET, drivers=DRIVERS), [STATE],
                   ['hist', 'stop_lap', 'stops_pos', 'seq'], None, {}),
    'run_moves': ('mcgp_run_moves', lambda s: s.run_moves(SIMS, GRID, **RACE, seed=SEED, sim_offset=OFFSET), None,
                  ['hist', 'grid_fin', 'start_gain', 'passes', 'race_passes', 'lap_passes', 'pair_passes'], None, {}),
    'run_conditions': ('mcgp_run_conditions',
                       lambda s: s.run_conditions(SIMS, CONDS, GRID, **RACE, seed=SEED, sim_offset=OFFSET), None,
                       ['hist', 'count', 'cond_hist'], None,
                       dict(conditions=[(len(c.atoms), [_struct(a) for a in c.c_struct().atom[:len(c.atoms)]])
                                        for c in CD.parse_all(CONDS, DRIVERS).values()])),
}


def counts_of(name, res):
    """The result's count arrays by name, and its finishing orders (or None)."""
    if name == 'run_monte_carlo':
        return {}, res[1]
    if name == 'run_from_state':
        return {}, res[1]
    if name == 'run_conditions':
        return dict(hist=res.hist, count=np.array([res.counts[k] for k in res.names]), cond_hist=res.cond_hist), None
    return {k: getattr(res, k) for k in CASES[name][3]}, getattr(res, 'orders', None)


@pytest.mark.parametrize('device', [0, [0, 0, 0]], ids=['one', 'three'])
@pytest.mark.parametrize('name', list(CASES))
def test_call(monkeypatch, name, device):
    entry, call, states, outputs, order_axis, inputs = CASES[name]
    rec = Recorder()
    monkeypatch.setattr(N, 'lib', lambda: rec)
    sim = simulator(device)
    res = call(sim)
    calls = sorted(rec.calls, key=lambda c: c['offset'])
    assert len(calls) == (1 if device == 0 else 3) and all(c['entry'] == entry for c in calls)
    # the shards tile [OFFSET, OFFSET + SIMS)
    assert calls[0]['offset'] == OFFSET and sum(c['count'] for c in calls) == SIMS
    assert all(a['offset'] + a['count'] == b['offset'] for a, b in zip(calls, calls[1:]))
    assert all(c['count'] > 0 for c in calls) and len({c['count'] for c in calls}) == (1 if device == 0 else 2)
    for c in calls:
        # the inputs are what the arguments say
        assert (c['total_laps'], c['deviates'], c['seed'], c['device']) == (L, 0, SEED, 0)
        assert c['base_pace'].tolist() == [PACE[d] for d in DRIVERS]
        if states is None:
            assert c['state'] is None and np.array_equal(c['grid'], GRID_MATRIX)
        else:
            assert c['grid'] is None and c['state'] == [expected_state(s) for s in states]
        if name == 'run_from_state':
            assert c['sim_offsets'] == [c['offset'], c['offset'] - OFFSET + 20]
        for key, want in inputs.items():
            assert c[key] == want, key
        assert c['nulls'] == []
    # the counts are the sum of the shards' patterns, as int64
    got, orders = counts_of(name, res)
    lead = {'run_from_state': (2,)}.get(name, ())
    S = inputs.get('S')
    for k, key in enumerate(outputs):
        if key not in got:
            continue
        shape = got[key].shape
        want = sum(pattern(entry, k, c['offset'], c['count'], shape) for c in calls)
        assert got[key].dtype == np.int64 and np.array_equal(got[key], want.astype(np.int64)), key
    hist_shape = sim.last_histogram.shape
    assert hist_shape == (lead + (n, n) if S is None else (S, n, n))
    assert np.array_equal(sim.last_histogram, sum(pattern(entry, 0, c['offset'], c['count'], hist_shape) for c in calls))
    assert sim.last_histogram.dtype == np.int64 and sim.last_drivers == DRIVERS
    # the finishing orders are the shards' one after the other along the simulation axis
    if order_axis is not None:
        front = (lead or (() if S is None else (S,)))
        want = np.concatenate([order_pattern(entry, c['offset'], c['count'], front + (c['count'], n)) for c in calls],
                              axis=order_axis)
        assert orders.dtype == np.uint8 and np.array_equal(orders, want)
    else:
        assert orders is None


@pytest.mark.parametrize('name', list(CASES))
def test_failed_shard_raises_with_its_message(monkeypatch, name):
    rec = Recorder(fail_on_call=1)
    monkeypatch.setattr(N, 'lib', lambda: rec)
    sim = simulator([0, 0, 0])
    with pytest.raises(N.McgpError) as e:
        CASES[name][1](sim)
    failed = rec.calls[1]
    assert e.value.code == -1 and f"shard at {failed['offset']} failed" in str(e.value)
