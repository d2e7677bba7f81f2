"""Monte Carlo race simulation on MI355X -- host side of the drop-in boundary.

Mirrors the reference's interface for the hot path (reference src/simulation.py):

    RaceConfig                                   :37-52   same fields, same defaults
    RaceSimulator(config)                        :55-57
    RaceSimulator.run_monte_carlo(...)           :59-100  same arguments, same result shape
    RaceSimulator.simulate_race(grid, ...)       :147-242 one race, list of (driver, position)
    RaceSimulator.run_matchups(...)              (not in the reference) head-to-head and podium counts of one race
    RaceSimulator.run_from_state(...)            (not in the reference) the rest of a race from a mid-race RaceState
    RaceSimulator.run_strategies(...)            (not in the reference) one race under planned pit stops (PitPlan)
    RaceSimulator.run_penalties(...)             (not in the reference) ... and under time penalties (TimePenalty)

The per-lap loop itself runs in hand-written HIP (csrc/race_kernel_reg.hip.h) behind
the C ABI of include/mcgp.h; this module only resolves the reference's dict
defaults into dense arrays, calls the library through ctypes and reshapes the
integer histogram into the reference's `dict[driver][position] -> probability`.
There is no CPU path: without the HIP library or a GPU the calls raise.

Randomness: the reference seeds two global Mersenne-Twister streams
(:76-78); here every draw is a pure function of (seed, simulation id, lap,
purpose, index) under Philox4x32-10, so results are reproducible for a given
seed on any number of GPUs.  `seed=None` draws a 64-bit seed from Python's
global `random`, which keeps a globally seeded backtest reproducible the way
reference src/validation.py:172-174 relies on.
"""
from __future__ import annotations

import ctypes as C
import math
import random
from dataclasses import dataclass, field

import numpy as np

from . import _native as N


@dataclass
class CarState:
    """The reference's per-car record (:9-34), kept for callers that import it: same fields, same defaults, same
    __post_init__.  Nothing here computes on it -- on the device a car is a binary64 `cumulative_time` and one packed
    word (grid slot, tyre age or retirement lap, driver, compound, dirty-air / DRS / retired flags, dry compounds used:
    csrc/race_kernel_reg.hip.h) in registers, and its `last_lap_time` a row of LDS; `position`, `pit_stops`,
    `laps_completed`, `team` and `fuel_load` are inert or derivable in the reference's loop."""
    driver: str
    team: str
    position: int
    lap: int
    tire_compound: str
    tire_age: int
    fuel_load: float
    time_behind_leader: float
    pit_stops: int
    cumulative_time: float = 0.0
    drs_enabled: bool = False
    dnf: bool = False
    used_compounds: set = field(default_factory=set)
    laps_completed: int = 0
    last_lap_time: float = 0.0

    def __post_init__(self):
        self.used_compounds.add(self.tire_compound)          # the starting compound counts as used (:31-34)


@dataclass
class RaceState:
    """A race after `lap` laps (1 .. total_laps), as the race model leaves it at the end of that lap: the input of
    RaceSimulator.run_from_state.  `cars` are CarState records in GRID order, as the reference's own list is (it never
    reorders it): the list index is the car's start-grid slot.  Per car it reads `driver`, `cumulative_time`,
    `last_lap_time`, `tire_compound` and `used_compounds` (the reference's compound names), `tire_age`, and `dnf` with
    `lap` as the lap of retirement.  `drs_disabled_until` is the reference simulate_race's variable: lap + 2 after a red
    flag or safety car, lap + 1 after a VSC, 0 if no event has happened."""
    lap: int
    drs_disabled_until: int = 0
    cars: list = field(default_factory=list)

    @staticmethod
    def from_json(obj: dict) -> 'RaceState':
        """{"lap", "drs_disabled_until" (optional), "cars": [{"driver", "cumulative_time", "last_lap_time",
        "tire_compound", "tire_age", "used_compounds", "retired_lap" (0 = running)}, ...] in grid order}."""
        lap = int(obj['lap'])
        cars = []
        for slot, c in enumerate(obj['cars']):
            retired = int(c.get('retired_lap', 0))
            cars.append(CarState(driver=str(c['driver']), team='', position=slot + 1, lap=retired if retired else lap,
                                 tire_compound=str(c['tire_compound']), tire_age=int(c['tire_age']),
                                 fuel_load=max(0.0, 110.0 - 1.5 * lap), time_behind_leader=0.0, pit_stops=0,
                                 cumulative_time=float(c['cumulative_time']), dnf=bool(retired),
                                 used_compounds={str(u) for u in c.get('used_compounds', [])},
                                 laps_completed=retired if retired else lap, last_lap_time=float(c['last_lap_time'])))
        return RaceState(lap=lap, drs_disabled_until=int(obj.get('drs_disabled_until', 0)), cars=cars)

    def to_json(self) -> dict:
        order = {c: i for i, c in enumerate(N.COMPOUNDS)}
        return {'lap': int(self.lap), 'drs_disabled_until': int(self.drs_disabled_until),
                'cars': [{'driver': c.driver, 'cumulative_time': float(c.cumulative_time),
                          'last_lap_time': float(c.last_lap_time), 'tire_compound': c.tire_compound,
                          'tire_age': int(c.tire_age),
                          'used_compounds': sorted(c.used_compounds, key=lambda u: order.get(u, len(order))),
                          'retired_lap': int(c.lap) if c.dnf else 0} for c in self.cars]}

    def arrays(self, drivers, total_laps=None) -> dict:
        """The mcgp_race_state arrays in the order of `drivers` (every car's driver exactly once): cumulative_time,
        last_lap_time (float64), grid_slot (= list index), compound (id), used_compounds (bit per compound id; the
        current compound included), tire_age, retired_lap (int16).  ValueError naming the driver on a bad field."""
        drivers = [str(d) for d in drivers]
        lap = int(self.lap)
        if lap < 1 or (total_laps is not None and lap > int(total_laps)):
            raise ValueError(f'lap must be in [1, total_laps], got {lap}')
        dd = int(self.drs_disabled_until)
        if dd < 0 or (total_laps is not None and dd > int(total_laps) + 2):
            raise ValueError(f'drs_disabled_until must be in [0, total_laps + 2], got {dd}')
        index = {d: i for i, d in enumerate(drivers)}
        names = [str(c.driver) for c in self.cars]
        if sorted(names) != sorted(drivers) or len(set(names)) != len(names):
            raise ValueError(f'the state\'s cars {names} are not the drivers {drivers}, each once')
        n = len(drivers)
        a = dict(cumulative_time=np.zeros(n, np.float64), last_lap_time=np.zeros(n, np.float64),
                 grid_slot=np.zeros(n, np.uint8), compound=np.zeros(n, np.uint8),
                 used_compounds=np.zeros(n, np.uint8), tire_age=np.zeros(n, np.int16),
                 retired_lap=np.zeros(n, np.int16))
        max_age = 1023 - (int(total_laps) - lap) if total_laps is not None else 1023
        for slot, c in enumerate(self.cars):
            d, i = str(c.driver), index[str(c.driver)]
            if c.tire_compound not in N.COMPOUND_ID:
                raise ValueError(f'{d}: tire_compound must be one of {list(N.COMPOUNDS)}, got {c.tire_compound!r}')
            bad = [u for u in c.used_compounds if u not in N.COMPOUND_ID]
            if bad:
                raise ValueError(f'{d}: used_compounds has unknown compounds {bad}')
            for key in ('cumulative_time', 'last_lap_time'):
                if not math.isfinite(float(getattr(c, key))):
                    raise ValueError(f'{d}: {key} is not finite')
            if not 0 <= int(c.tire_age) <= max_age:
                raise ValueError(f'{d}: tire_age must be in [0, {max_age}], got {c.tire_age}')
            retired = int(c.lap) if c.dnf else 0
            if c.dnf and not 1 <= retired <= lap:
                raise ValueError(f'{d}: a retired car\'s lap must be in [1, {lap}], got {c.lap}')
            a['cumulative_time'][i] = float(c.cumulative_time)
            a['last_lap_time'][i] = float(c.last_lap_time)
            a['grid_slot'][i] = slot
            a['compound'][i] = N.COMPOUND_ID[c.tire_compound]
            a['used_compounds'][i] = sum(1 << N.COMPOUND_ID[u] for u in set(c.used_compounds) | {c.tire_compound})
            a['tire_age'][i] = int(c.tire_age)
            a['retired_lap'][i] = retired
        return a

    def c_struct(self, arrays):
        """mcgp_race_state over `arrays` (from arrays(); the caller keeps them alive)."""
        p = lambda k, t: arrays[k].ctypes.data_as(C.POINTER(t))
        return N.McgpRaceState(lap=int(self.lap), drs_disabled_until=int(self.drs_disabled_until),
                               cumulative_time=p('cumulative_time', C.c_double), last_lap_time=p('last_lap_time', C.c_double),
                               grid_slot=p('grid_slot', C.c_uint8), compound=p('compound', C.c_uint8),
                               used_compounds=p('used_compounds', C.c_uint8), tire_age=p('tire_age', C.c_int16),
                               retired_lap=p('retired_lap', C.c_int16))


@dataclass
class RaceConfig:
    """Same fields and defaults as the reference's RaceConfig (:37-52)."""
    total_laps: int
    pit_loss: float
    overtake_delta: float
    sc_probability: float
    vsc_probability: float
    red_flag_probability: float
    dnf_rates: dict
    drs_zones: int
    drs_delta: float
    tire_compounds: dict
    driver_teams: dict
    dirty_air_threshold: float = 2.0
    dirty_air_penalty: float = 0.5


# `available.pop()` at reference :486,488 picks from a two-string set; CPython's answer
# depends on PYTHONHASHSEED.  These are the outcomes under PYTHONHASHSEED=0 (the setting the
# golden fixtures were made with, tests/golden/cases.json "set_pop").
DEFAULT_SET_POP = {'SOFT_HARD': 'HARD', 'MEDIUM_HARD': 'MEDIUM'}


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _optr(a):
    """An output buffer as the C ABI takes it: uint64 counts, uint8 finishing orders or binary32 values; None (not wanted)
    is NULL."""
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_float if a.dtype == np.float32 else C.c_uint64))


def _gap_edge_array(edges):
    """The bin edges of run_gaps / run_pit_windows as the C ABI takes them (None: DEFAULT_GAP_EDGES), checked."""
    edge_arr = np.ascontiguousarray(DEFAULT_GAP_EDGES if edges is None else list(edges), np.float64)
    if edge_arr.ndim != 1 or not 1 <= len(edge_arr) <= N.MAX_GAP_EDGES:
        raise ValueError(f'edges: 1 to {N.MAX_GAP_EDGES} values, got {edge_arr.shape}')
    if not (np.isfinite(edge_arr).all() and edge_arr[0] > 0 and (np.diff(edge_arr) > 0).all()):
        raise ValueError('edges must be finite, positive and strictly increasing')
    return edge_arr


def _count_arrays(result):
    """The count arrays of a result object, by field name."""
    return {k: v for k, v in vars(result).items() if isinstance(v, np.ndarray)}


class _Source:
    """Where a call's races start, as RaceSimulator._source resolved it: from the grid (grid_probs) or from a mid-race
    RaceState (state), for `drivers` in index order.  The grid matrix and the state's arrays are built on first use, so
    that a call with nothing to run builds (and checks) neither."""

    def __init__(self, grid_probs, state, drivers, total_laps):
        self.grid_probs, self.state, self.drivers, self.total_laps = grid_probs, state, drivers, int(total_laps)
        self._arrays = self._keep = self._c_args = None

    def first_lap(self, from_grid=2):
        """The first lap the call runs: `from_grid` (2: the first lap with a pit step), or the one after the state's."""
        return from_grid if self.state is None else int(self.state.lap) + 1

    @property
    def arrays(self):
        """The state's arrays in driver order (RaceState.arrays; None from the grid)."""
        if self.state is not None and self._arrays is None:
            self._arrays = self.state.arrays(self.drivers, self.total_laps)
        return self._arrays

    def c_args(self):
        """The entry points' (grid_probs, state) arguments: the matrix and NULL, or NULL and the mcgp_race_state."""
        if self._c_args is None:
            if self.state is None:
                self._keep = RaceSimulator._grid_matrix({str(k): v for k, v in self.grid_probs.items()}, self.drivers)
                self._c_args = (_dptr(self._keep), None)
            else:
                self._keep = self.state.c_struct(self.arrays)
                self._c_args = (None, C.byref(self._keep))
        return self._c_args


class _Problem:
    """run_monte_carlo's arguments resolved to the dense tables of include/mcgp.h."""

    def __init__(self, config: RaceConfig, drivers, base_pace, tire_deg, driver_variance,
                 driver_dnf_rates, track_condition, set_pop, deviates=32):
        if track_condition not in N.TRACK_ID:
            raise ValueError(f"track_condition must be 'dry', 'damp' or 'wet', got {track_condition!r}")
        self.drivers = [str(d) for d in drivers]
        n = self.n = len(self.drivers)
        c = self.cfg = N.McgpConfig()
        c.total_laps = int(config.total_laps)
        c.track_condition = N.TRACK_ID[track_condition]
        c.pit_loss = float(config.pit_loss)
        c.overtake_delta = float(config.overtake_delta)
        c.sc_probability = float(config.sc_probability)
        c.vsc_probability = float(config.vsc_probability)
        c.red_flag_probability = float(config.red_flag_probability)
        c.drs_delta = float(config.drs_delta)
        c.dirty_air_threshold = float(config.dirty_air_threshold)
        c.dirty_air_penalty = float(config.dirty_air_penalty)
        for name, i in N.COMPOUND_ID.items():
            info = config.tire_compounds.get(name, {})        # reference :317,454
            c.comp_pace_delta[i] = float(info.get('pace_delta', 0))
            c.comp_deg_rate[i] = float(info.get('deg_rate', 0.05))
            c.comp_optimal_laps[i] = int(info.get('optimal_laps', 30))
        c.pop_soft_hard = N.COMPOUND_ID[set_pop['SOFT_HARD']]
        c.pop_medium_hard = N.COMPOUND_ID[set_pop['MEDIUM_HARD']]
        if deviates not in (32, 53):
            raise ValueError(f'deviates must be 32 or 53, got {deviates!r}')
        c.deviates = 1 if deviates == 53 else 0

        driver_dnf_rates = driver_dnf_rates or {}
        team_rate = [config.dnf_rates.get(config.driver_teams.get(d, 'Unknown'), 0.002)   # :263,286
                     for d in self.drivers]
        f64 = np.float64
        self.arrays = dict(
            base_pace=np.array([base_pace.get(d, 90.0) for d in self.drivers], f64),           # :202
            tire_deg=np.array([tire_deg.get(d, 0.05) for d in self.drivers], f64),             # :203
            tire_deg_pit=np.array([tire_deg.get(d, 0.0) for d in self.drivers], f64),          # :458
            variance=np.array([driver_variance.get(d, 0.15) for d in self.drivers], f64),      # :204
            team_dnf=np.array(team_rate, f64),
            lap_dnf=np.array([driver_dnf_rates.get(d, team_rate[i])                           # :190-193
                              for i, d in enumerate(self.drivers)], f64),
        )
        self.drv = N.McgpDrivers(**{k: _dptr(v) for k, v in self.arrays.items()})


class RaceSimulator:
    """Drop-in for the reference's RaceSimulator (:55-560) with the race loop on the GPU."""

    def __init__(self, config: RaceConfig, device=0, set_pop: dict | None = None, deviates: int = 32):
        """`deviates`: 32 (default) -- uniforms w / 2^32 and normals from a binary32 cubic table, the fast path -- or 53:
        the reference's width, 53-bit uniforms and binary64 normals (reference :137,194,302,330,524), every draw keeping
        the 32-bit mode's word as its leading bits; a priced option (include/mcgp.h: mcgp_config.deviates), every field
        size.

        `device`: a HIP device index (default 0), a list of indices, or 'all' (every visible device).  With more
        than one device a run_monte_carlo call is split by simulation id into contiguous shards, one host thread per
        device over the same C entry point, and the integer histograms are added on the host -- the whole node from the
        plain single-process call the reference's caller makes (reference src/predictor.py:264,283-291), with results
        identical to a one-device run (every draw is a function of the global simulation id).  An index may be
        listed more than once (shards then queue on that device).  The torchrun + RCCL path (distributed.py) is
        separate and unchanged."""
        self.config = config
        self.deviates = int(deviates)
        if isinstance(device, str):
            if device != 'all':
                raise ValueError(f"device must be an index, a list of indices or 'all', got {device!r}")
            count = N.lib().mcgp_device_count()
            if count < 1:
                raise N.McgpError(-2, 'no HIP device visible (this library has no CPU path)')
            self.devices = list(range(count))
        elif isinstance(device, (list, tuple)):
            if not device:
                raise ValueError('device list is empty')
            self.devices = [int(d) for d in device]
        else:
            self.devices = [int(device)]
        self.device = self.devices[0]        # single-device entry points (simulate_race, the front end) use the first
        self.set_pop = dict(set_pop or DEFAULT_SET_POP)
        self.last_histogram = None      # np.int64 [n, n], counts[driver][position-1] of the last run
        self.last_drivers = None
        self._race_inputs = None

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _grid_matrix(grid_probs, drivers):
        n = len(drivers)
        g = np.zeros((n, n), np.float64)
        for i, d in enumerate(drivers):
            row = grid_probs[d]
            m = min(len(row), n)             # `pos < len(grid_probs.get(d, []))` else 0, reference :120
            g[i, :m] = np.asarray(row[:m], np.float64)
        return np.ascontiguousarray(g)

    @staticmethod
    def _resolve_seed(seed):
        if seed is None:
            return random.getrandbits(64)
        seed = int(seed)
        if seed < 0:
            seed = -seed                     # random.seed() uses abs(seed)
        return seed & 0xFFFFFFFFFFFFFFFF

    def _run_sharded(self, run_shard, n_simulations):
        """run_shard(device, offset, count) -> (result, rc, message) over self.devices: contiguous shards of the
        simulation ids, one host thread per device.  Raises on the first failed shard; returns the shards' results."""
        if len(self.devices) == 1:
            parts = [run_shard(self.devices[0], 0, int(n_simulations))]
        else:
            from concurrent.futures import ThreadPoolExecutor
            from .distributed import shard_range
            world = len(self.devices)
            shards = [shard_range(int(n_simulations), k, world) for k in range(world)]
            with ThreadPoolExecutor(world) as ex:          # ctypes releases the GIL for the duration of the call
                parts = list(ex.map(lambda a: run_shard(a[0], *a[1]), zip(self.devices, shards)))
        for _, rc, msg in parts:
            if rc != 0:
                raise N.McgpError(rc, msg)
        return parts

    def _problem(self, drivers, base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition):
        n = len(drivers)
        if n < 1 or n > N.MAX_CARS:
            raise ValueError(f'number of drivers must be in [1, {N.MAX_CARS}], got {n}')
        return _Problem(self.config, drivers, base_pace, tire_deg, driver_variance, driver_dnf_rates,
                        track_condition, self.set_pop, self.deviates)

    def _source(self, grid_probs, state, drivers):
        """The start of a call's races and its drivers (default: grid_probs' keys, or the state's grid order)."""
        if (grid_probs is None) == (state is None):
            raise ValueError('give exactly one of grid_probs (a run from the grid) and state (a run from a race state)')
        if drivers is None:
            drivers = list(grid_probs.keys()) if grid_probs is not None else [c.driver for c in state.cars]
        drivers = [str(d) for d in drivers]
        if grid_probs is not None and sorted(drivers) != sorted(str(k) for k in grid_probs.keys()):
            raise ValueError('drivers must be the keys of grid_probs')
        return _Source(grid_probs, state, drivers, self.config.total_laps)

    def _run_counted(self, n_simulations, drivers, alloc, call, orders_axis=None):
        """The sharded run behind every run_* method.  alloc(count) -> {name: buffer} makes one shard's outputs:
        np.uint64 counts, under 'orders' the np.uint8 finishing orders of `count` simulations, None for an output that
        is not wanted.  call(lib, device, offset, count, buffers) makes the C call for simulations offset .. offset +
        count - 1 of the run and returns its code.  Returns, by name, the shards' counts added up (np.int64), their
        orders one after the other along `orders_axis`, and None where alloc gave None -- for n_simulations <= 0 what
        alloc(0) gives, without a call.  Sets last_histogram (the 'hist' counts) and last_drivers."""
        if n_simulations <= 0:
            parts = [alloc(0)]
        else:
            lib = N.lib()

            def shard(device, offset, count):
                bufs = alloc(int(count))
                rc = call(lib, device, int(offset), int(count), bufs)
                # (mcgp_last_error is thread-local: read it on the thread that made the call)
                return bufs, rc, (lib.mcgp_last_error().decode('utf-8', 'replace') if rc != 0 else '')

            parts = [bufs for bufs, _, _ in self._run_sharded(shard, n_simulations)]
        total = {}
        for k, first in parts[0].items():
            if first is None:
                total[k] = None
            elif k in ('orders', 'offsets'):                 # written per simulation, not counted
                total[k] = np.concatenate([p[k] for p in parts], axis=orders_axis)
            else:
                total[k] = np.sum([p[k] for p in parts], axis=0, dtype=np.uint64).astype(np.int64)
        self.last_histogram, self.last_drivers = total['hist'], drivers
        return total

    @staticmethod
    def _entry_call(entry, prob, head, sim_offset, seed64, outs):
        """_run_counted's `call` for an entry point of the usual shape: lib.<entry>(cfg, drivers, *head, n_sims,
        sim_offset, seed, device, *outputs), the outputs being the buffers named by `outs` (None: NULL)."""
        def call(lib, device, offset, count, bufs):
            return getattr(lib, entry)(C.byref(prob.cfg), C.byref(prob.drv), *head, count, int(sim_offset) + offset,
                                       seed64, device, *[_optr(bufs.get(k)) for k in outs])
        return call

    def _run_entry(self, entry, n_simulations, drivers, race, seed, sim_offset, head, alloc, outs):
        """One race counted by lib.<entry>: _run_counted over _entry_call.  race: _problem's arguments after the drivers;
        head(n): the entry point's arguments between the driver tables and n_sims.  Without drivers or simulations
        nothing is resolved, built or called: the counts are alloc(0)'s."""
        if not drivers or n_simulations <= 0:
            return self._run_counted(0, drivers, alloc, None)
        prob = self._problem(drivers, *race)
        call = self._entry_call(entry, prob, head(prob.n), sim_offset, self._resolve_seed(seed), outs)
        return self._run_counted(n_simulations, drivers, alloc, call)

    def _pack_plans(self, names, plans_of, src, check_compounds, kinds=()):
        """The scenarios' pit plans as mcgp_pit_plan structs with their count per scenario, and likewise the items of
        each of the call's own `kinds`, (items_of {name: [item]}, pack_items), through pack_items(name, items, index)
        -> [struct]: scenario by scenario, plans first, then the kinds in their order.  check_compounds: the
        two-compound rule holds for every plan (a bool, or scenario name -> bool).  -> counts, structs, [(counts,
        structs) of each kind]."""
        index = {d: i for i, d in enumerate(src.drivers)}
        counts, c_plans, packed_kinds = [], [], [([], []) for _ in kinds]
        for name in names:
            plans = plans_of.get(name, [])
            for plan in plans:
                if str(plan.driver) not in index:
                    raise ValueError(f'scenario {name!r}: {plan.driver!r} is not one of the drivers')
                if check_compounds(name) if callable(check_compounds) else check_compounds:
                    used = None
                    if src.arrays is not None:
                        used = {c for j, c in enumerate(N.COMPOUNDS)
                                if (int(src.arrays['used_compounds'][index[str(plan.driver)]]) >> j) & 1}
                    check_two_compounds(plan, used, name)
                c_plans.append(plan.c_struct(index, from_state=src.state is not None))
            counts.append(len(plans))
            for (items_of, pack_items), (item_counts, c_items) in zip(kinds, packed_kinds):
                packed = pack_items(name, items_of.get(name, []), index)
                c_items += packed
                item_counts.append(len(packed))
        return counts, c_plans, packed_kinds

    def _run_scenarios(self, entry, result, label, n_simulations, kinds, strategies, race, grid_probs, state, seed,
                       sim_offset, drivers, return_orders, allow_single_compound, call_wide=(), all_dry=None,
                       grid_only=False, written=None, result_args=None):
        """run_strategies, run_penalties, run_events, run_paces, run_combined, run_weather and run_grids: the race under named scenarios of pit
        plans (`strategies`) and of the call's own `kinds` of items, a list (empty for run_strategies) of (items {name:
        [item]}, item_type: their struct, pack_items: see _pack_plans, extra = (name, shape(S, n, L)): the kind's own
        count array, or a list of such pairs).  The scenario names are the union of the dicts in the order given, the kinds' first; the kinds'
        (count, items) pairs follow the plans among the arguments and their count arrays follow hist and delta among
        the outputs, both in the kinds' order.  result: the result class; label: the dicts' names for the message.
        call_wide: the call's arguments that hold for every scenario, after the kinds' (run_weather: its model).
        all_dry: scenario name -> is the track dry on every lap (None: track_condition says so for all of them); the
        two-compound rule is checked for the plans of those scenarios.  grid_only: the entry point has no state argument
        (run_grids, which has refused a state by then).  written: {name: dtype} of the call's own outputs that are
        written per simulation, [S][count][n], between the count arrays and the orders (run_priors: its offsets; None as a
        dtype: NULL).  result_args: further keyword arguments of the result."""
        src = self._source(grid_probs, state, drivers)
        strategies = strategies or {}
        names = []
        for given in [items for items, _, _, _ in kinds] + [strategies]:
            names += [str(k) for k in given.keys() if str(k) not in names]
        if not 1 <= len(names) <= N.MAX_SCENARIOS:
            raise ValueError(f'{label}: 1 to {N.MAX_SCENARIOS} scenarios, got {len(names)}')
        drivers = src.drivers
        prob = self._problem(drivers, *race)
        n, L, S = prob.n, int(self.config.total_laps), len(names)
        src.arrays                                   # (a bad state is reported before a bad plan)
        by_name = lambda given: {str(k): list(v) for k, v in given.items()}
        counts, c_plans, packed_kinds = self._pack_plans(
            names, by_name(strategies), src,
            not allow_single_compound and (all_dry if all_dry is not None else race[-1] == 'dry'),
            [(by_name(items), pack) for items, _, pack, _ in kinds])
        head = (src.c_args()[:1] if grid_only else src.c_args()) + (n, S, (C.c_uint32 * S)(*counts), (N.McgpPitPlan * max(len(c_plans), 1))(*c_plans))
        for (_, item_type, _, _), (item_counts, c_items) in zip(kinds, packed_kinds):
            head += ((C.c_uint32 * S)(*item_counts), (item_type * max(len(c_items), 1))(*c_items))
        head += tuple(call_wide)
        n_simulations = max(int(n_simulations), 0)
        seed64 = self._resolve_seed(seed)
        if not hasattr(N.lib(), entry):
            raise N.McgpError(-1, f'the loaded library does not export {entry}')
        extras = [pair for _, _, _, extra in kinds for pair in (extra if isinstance(extra, list) else [extra])]
        shapes = dict(hist=(S, n, n), delta=(S, n, 2 * n - 1), **{name: shape(S, n, L) for name, shape in extras})

        def alloc(count):
            return dict({k: np.zeros(shape, np.uint64) for k, shape in shapes.items()},
                        **{k: np.zeros((S, count, n), dt) if dt is not None else None for k, dt in (written or {}).items()},
                        orders=np.zeros((S, count, n), np.uint8) if return_orders else None)

        outs = list(shapes) + list(written or {}) + ['orders']
        total = self._run_counted(n_simulations, drivers, alloc,
                                  self._entry_call(entry, prob, head, sim_offset, seed64, outs), 1)
        return result(names=names, drivers=drivers, n_simulations=n_simulations, **total, **(result_args or {}))

    # ---- the scenario calls' own kinds of items: (items, struct, pack_items, (count array, its shape)) for _run_scenarios
    def _penalty_kind(self, penalties, state):
        def pack(name, pens, index):
            packed, seen = [], set()
            for pen in pens:
                if str(pen.driver) not in index:
                    raise ValueError(f'scenario {name!r}: {pen.driver!r} is not one of the drivers')
                c = pen.c_struct(index, 2 if state is None else int(state.lap) + 1)
                key = (c.driver, c.kind, c.lap if c.kind == N.PEN_ON_LAP else 0)
                if key in seen:
                    raise ValueError(f'scenario {name!r}: {pen.driver} has two penalties of kind {pen.kind!r}'
                                     + (f' on lap {c.lap}' if c.kind == N.PEN_ON_LAP else '') + '; sum them into one')
                seen.add(key)
                packed.append(c)
            if len(pens) > N.MAX_SCENARIO_PENALTIES:
                raise ValueError(f'scenario {name!r}: at most {N.MAX_SCENARIO_PENALTIES} penalties, got {len(pens)}')
            return packed

        return penalties, N.McgpTimePenalty, pack, ('fate', lambda S, n, L: (S, n, 4))

    def _event_kind(self, events, state):
        def pack(name, evs, index):
            if len(evs) > N.MAX_SCENARIO_EVENTS:
                raise ValueError(f'scenario {name!r}: at most {N.MAX_SCENARIO_EVENTS} overrides, got {len(evs)}')
            packed, covered = [], {}
            for ev in evs:
                try:
                    c = ev.c_struct(2 if state is None else int(state.lap) + 1, int(self.config.total_laps))
                except ValueError as e:
                    raise ValueError(f'scenario {name!r}: {e}') from None
                for lap in range(c.first_lap, c.last_lap + 1):
                    if lap in covered:
                        raise ValueError(f'scenario {name!r}: lap {lap} has two overrides ({covered[lap]} and {ev})')
                    covered[lap] = ev
                packed.append(c)
            return packed

        return events, N.McgpLapEvent, pack, ('events', lambda S, n, L: (S, 3, L + 1))

    def _pace_kind(self, paces, grid_probs, state):
        first = _Source(grid_probs, state, None, self.config.total_laps).first_lap(from_grid=1)

        def pack(name, offs, index):
            if len(offs) > N.MAX_SCENARIO_PACES:
                raise ValueError(f'scenario {name!r}: at most {N.MAX_SCENARIO_PACES} offsets, got {len(offs)}')
            packed, covered, until = [], {}, {}
            for off in offs:
                if str(off.driver) not in index:
                    raise ValueError(f'scenario {name!r}: {off.driver!r} is not one of the drivers')
                try:
                    c = off.c_struct(index, first, int(self.config.total_laps))
                except ValueError as e:
                    raise ValueError(f'scenario {name!r}: {e}') from None
                if c.kind == N.PACE_UNTIL_STOP:
                    if c.driver in until:
                        raise ValueError(f'scenario {name!r}: {off.driver} has two until-stop offsets '
                                         f'({until[c.driver]} and {off})')
                    until[c.driver] = off
                else:
                    for lap in range(c.first_lap, c.last_lap + 1):
                        if (c.driver, lap) in covered:
                            raise ValueError(f'scenario {name!r}: {off.driver} has two offsets on lap {lap} '
                                             f'({covered[c.driver, lap]} and {off})')
                        covered[c.driver, lap] = off
                packed.append(c)
            return packed

        return paces, N.McgpPaceOffset, pack, ('carried', lambda S, n, L: (S, n, L + 1))

    @staticmethod
    def _until_from(paces):
        return {(str(name), str(off.driver)): int(off.until_stop_from) for name, offs in paces.items()
                for off in offs if off.until_stop_from is not None}

    # ------------------------------------------------------------------ reference surface
    def run_monte_carlo(
        self,
        n_simulations: int,
        grid_probs: dict,
        base_pace: dict,
        tire_deg: dict,
        driver_variance: dict,
        driver_dnf_rates: dict | None = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        return_orders: bool = False,
    ):
        """Run n simulations and return position probability distributions (reference :59-100).

        Returns {driver: {position (1-based): probability}} holding only non-zero cells,
        like the reference.  Extra keyword arguments (not in the reference):
        sim_offset -- first global simulation id (for sharding a run over ranks);
        return_orders -- also return the [n_sims, n] finishing orders (driver index per position).
        """
        drivers = [str(d) for d in grid_probs.keys()]
        if not drivers or n_simulations <= 0:
            self.last_histogram, self.last_drivers = np.zeros((len(drivers),) * 2, np.int64), drivers
            return ({}, np.zeros((0, len(drivers)), np.uint8)) if return_orders else {}
        prob = self._problem(drivers, base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition)
        n = prob.n
        g = self._grid_matrix({str(k): v for k, v in grid_probs.items()}, drivers)
        orders = np.zeros((n_simulations, n), np.uint8) if return_orders else None
        seed64 = self._resolve_seed(seed)

        def call(lib, device, offset, count, bufs):
            o = orders[offset:offset + count] if return_orders else None       # contiguous rows of the caller's buffer
            return lib.mcgp_run(C.byref(prob.cfg), C.byref(prob.drv), _dptr(g), n, count, int(sim_offset) + offset, seed64,
                                device, _optr(bufs['hist']), _optr(o))

        self._run_counted(n_simulations, drivers, lambda count: dict(hist=np.zeros((n, n), np.uint64)), call)
        result = histogram_to_probs(self.last_histogram, drivers, n_simulations)
        return (result, orders) if return_orders else result

    def run_matchups(
        self,
        n_simulations: int,
        grid_probs: dict,
        base_pace: dict,
        tire_deg: dict,
        driver_variance: dict,
        driver_dnf_rates: dict | None = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        podiums: bool = True,
    ) -> 'MatchupResult':
        """run_monte_carlo's race, counted for pairs and podiums on the device (include/mcgp.h: mcgp_run_matchups).

        Same arguments, simulations and sharding over self.devices as run_monte_carlo; returns a MatchupResult whose
        position histogram equals run_monte_carlo's, plus head-to-head counts and (podiums=True, at least 3 drivers) the
        counts of every ordered podium.  No finishing order leaves the device.  Sets last_histogram / last_drivers."""
        drivers = [str(d) for d in grid_probs.keys()]
        n = len(drivers)
        n_simulations = int(n_simulations)
        want_podium = bool(podiums) and n >= 3
        src = _Source(grid_probs, None, drivers, self.config.total_laps)
        total = self._run_entry(
            'mcgp_run_matchups', n_simulations, drivers,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), seed, sim_offset,
            lambda n: (src.c_args()[0], n),
            lambda count: dict(hist=np.zeros((n, n), np.uint64), ahead=np.zeros((n, n), np.uint64),
                               podium=np.zeros((n, n, n), np.uint64) if want_podium else None),
            ['hist', 'ahead', 'podium'])
        return MatchupResult(drivers=drivers, n_simulations=max(n_simulations, 0), **total)

    def run_trace(
        self,
        n_simulations: int,
        grid_probs: dict,
        base_pace: dict,
        tire_deg: dict,
        driver_variance: dict,
        driver_dnf_rates: dict | None = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
    ) -> 'TraceResult':
        """run_monte_carlo's race, counted lap by lap on the device (include/mcgp.h: mcgp_run_trace): running positions
        after every lap, laps led, pit stops, fastest lap and race events.  Same arguments, simulations and sharding over
        self.devices as run_monte_carlo; the TraceResult's position histogram equals run_monte_carlo's.  32-bit deviates
        only.  Sets last_histogram / last_drivers."""
        drivers = [str(d) for d in grid_probs.keys()]
        n, L = len(drivers), int(self.config.total_laps)
        n_simulations = int(n_simulations)
        src = _Source(grid_probs, None, drivers, L)
        total = self._run_entry(
            'mcgp_run_trace', n_simulations, drivers,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), seed, sim_offset,
            lambda n: (src.c_args()[0], n),
            lambda count: _count_arrays(TraceResult.empty(drivers, L, count, dtype=np.uint64)),
            ['hist', 'lap_pos', 'laps_led', 'stops', 'fastest', 'events'])
        return TraceResult(drivers=drivers, n_simulations=max(n_simulations, 0), total_laps=L, **total)

    def run_from_state(
        self,
        n_simulations: int,
        state,
        base_pace: dict,
        tire_deg: dict,
        driver_variance: dict,
        driver_dnf_rates: dict | None = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset=0,
        drivers=None,
        return_orders: bool = False,
    ):
        """In-race odds: the rest of the race from a RaceState, or from each of a list of them (scenarios of the same
        drivers), on the device (include/mcgp.h: mcgp_run_from_state).  Returns run_monte_carlo's {driver: {position:
        probability}} for one state, a list of them for a list.

        Simulation i of every state has id sim_offset + i (sim_offset: an int, or one per state) and makes on the laps
        after the state exactly the draws run_monte_carlo's simulation i makes there: scenarios given the same ids see
        the same random futures (common random numbers).  `drivers` fixes the driver-index order (default: the first
        state's grid order); with a run_monte_carlo call's grid_probs key order, a state that run's simulation i reached
        continues, as simulation i, into that run's finishing order.  A running car whose once-per-race retirement
        draw names a lap the state has already passed gets a fresh draw over the remaining laps.  32-bit deviates only.
        return_orders: also the finishing orders ([N, n], or [S, N, n] for a list).  last_histogram: [n, n], or
        [S, n, n] for a list.  Same seed rules and device sharding as run_monte_carlo."""
        single = isinstance(state, RaceState)
        states = [state] if single else list(state)
        if not states:
            raise ValueError('no race state given')
        drivers = [str(d) for d in (drivers if drivers is not None else [c.driver for c in states[0].cars])]
        S, n_simulations = len(states), int(n_simulations)
        offsets = [int(sim_offset)] * S if isinstance(sim_offset, (int, np.integer)) else [int(x) for x in sim_offset]
        if len(offsets) != S:
            raise ValueError(f'sim_offset: one per state ({S}), got {len(offsets)}')
        prob = self._problem(drivers, base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition)
        n = prob.n
        arrays = [st.arrays(drivers, self.config.total_laps) for st in states]
        c_states = (N.McgpRaceState * S)(*[st.c_struct(a) for st, a in zip(states, arrays)])
        shape = (n, n) if single else (S, n, n)
        if n_simulations <= 0:
            self.last_histogram, self.last_drivers = np.zeros(shape, np.int64), drivers
            empty = [{} for _ in states]
            res = empty[0] if single else empty
            if return_orders:
                return res, np.zeros((0, n) if single else (S, 0, n), np.uint8)
            return res
        seed64 = self._resolve_seed(seed)

        def alloc(count):
            return dict(hist=np.zeros((S, n, n), np.uint64),
                        orders=np.zeros((S, count, n), np.uint8) if return_orders else None)

        def call(lib, device, offset, count, bufs):
            so = (C.c_uint64 * S)(*[x + offset for x in offsets])
            return lib.mcgp_run_from_state(C.byref(prob.cfg), C.byref(prob.drv), n, S, c_states, count, so, seed64, device,
                                           _optr(bufs['hist']), _optr(bufs['orders']))

        total = self._run_counted(n_simulations, drivers, alloc, call, 1)
        hist, orders = total['hist'], total['orders']
        if single:
            self.last_histogram = hist[0]
        probs = [histogram_to_probs(hist[s], drivers, n_simulations) for s in range(S)]
        res = probs[0] if single else probs
        if return_orders:
            return res, (orders[0] if single else orders)
        return res

    def run_strategies(
        self,
        n_simulations: int,
        strategies: dict,
        base_pace: dict,
        tire_deg: dict,
        driver_variance: dict,
        driver_dnf_rates: dict | None = None,
        grid_probs: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
        return_orders: bool = False,
        allow_single_compound: bool = False,
    ) -> 'StrategyResult':
        """Pit-strategy comparison (include/mcgp.h: mcgp_run_strategies): the race under each scenario of `strategies`,
        {name: [PitPlan, ...]} with at most one plan per driver (at most 64 scenarios; the first is the one `compare`
        measures against).  Drivers without a plan keep the model's pit rule; a planned driver stops only on its plan's
        laps.  From the grid (grid_probs) or from a mid-race RaceState (state; plans then have no start fields and stop
        after the state's lap).  Simulation i of every scenario has id sim_offset + i and makes run_monte_carlo's (or
        run_from_state's) draws: an empty scenario gives exactly that call's histogram, and the scenarios share the
        grid, the retirements and the race events.  On a dry track a plan that cannot use two dry compounds raises
        ValueError unless allow_single_compound.  32-bit deviates only; same seed rules and device sharding as
        run_monte_carlo.  last_histogram: [S, n, n]."""
        return self._run_scenarios(
            'mcgp_run_strategies', StrategyResult, 'strategies', n_simulations, [], strategies,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), grid_probs, state, seed, sim_offset,
            drivers, return_orders, allow_single_compound)

    def run_penalties(
        self,
        n_simulations: int,
        penalties: dict,
        strategies: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        grid_probs: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
        return_orders: bool = False,
        allow_single_compound: bool = False,
    ) -> 'PenaltyResult':
        """Time penalties (include/mcgp.h: mcgp_run_penalties): the race under each scenario of `penalties`, {name:
        [TimePenalty, ...]}, and `strategies`, {name: [PitPlan, ...]} or None; a scenario holds the penalties and the
        plans given under its name, and the scenario names are the union of the two dicts in the order given (penalties
        first; at most 64; the first is the one `compare` measures against).  Per scenario and driver at most one
        penalty of kind 'serve', one of kind 'flag' and one of kind 'lap' per lap: two of one kind raise ValueError (sum
        them).  Everything else -- the remaining arguments, the plans' checks, the simulation ids and draws, the seed
        rules and the device sharding -- is run_strategies': a scenario without penalties gives exactly its counts.
        last_histogram: [S, n, n]."""
        return self._run_scenarios(
            'mcgp_run_penalties', PenaltyResult, 'penalties / strategies', n_simulations,
            [self._penalty_kind(penalties, state)], strategies,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), grid_probs, state, seed, sim_offset,
            drivers, return_orders, allow_single_compound)

    def run_events(
        self,
        n_simulations: int,
        events: dict,
        strategies: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        grid_probs: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
        return_orders: bool = False,
        allow_single_compound: bool = False,
    ) -> 'EventResult':
        """Event scenarios (include/mcgp.h: mcgp_run_events): the race under each scenario of `events`, {name:
        [RaceEvent, ...]}, and `strategies`, {name: [PitPlan, ...]} or None; a scenario holds the overrides and the plans
        given under its name, and the scenario names are the union of the two dicts in the order given (events first; at
        most 64; the first is the one `compare` measures against).  On the laps a RaceEvent covers, the race has that
        event ('sc', 'vsc', 'red') or none ('none') instead of what the lap draws; other laps are drawn as always.  An
        event is one lap's bunching of the field: a safety-car period of several laps is a range, and pitting under it
        is what the plans say.  Overlapping overrides in one scenario, an unknown kind and a lap outside the laps still
        to run raise ValueError.  Everything else -- the remaining arguments, the plans' checks, the simulation ids and
        draws, the seed rules and the device sharding -- is run_strategies': a scenario without overrides gives exactly
        its counts.  last_histogram: [S, n, n]."""
        return self._run_scenarios(
            'mcgp_run_events', EventResult, 'events / strategies', n_simulations, [self._event_kind(events, state)],
            strategies, (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), grid_probs, state, seed,
            sim_offset, drivers, return_orders, allow_single_compound)

    def run_paces(
        self,
        n_simulations: int,
        paces: dict,
        strategies: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        grid_probs: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
        return_orders: bool = False,
        allow_single_compound: bool = False,
    ) -> 'PaceResult':
        """Pace scenarios (include/mcgp.h: mcgp_run_paces): the race under each scenario of `paces`, {name:
        [PaceOffset, ...]}, and `strategies`, {name: [PitPlan, ...]} or None; a scenario holds the offsets and the plans
        given under its name, and the scenario names are the union of the two dicts in the order given (paces first; at
        most 64; the first is the one `compare` measures against).  A PaceOffset adds seconds to a driver's base pace on
        a range of laps, or from a lap until the car's next pit stop, wherever the model reads the base pace: the lap
        time, and the pace of the overtake model (a slowed car is easier to pass).  From the grid an offset may name lap
        1; from a state, the laps after the state's.  Two lap ranges of one driver that share a lap, a second
        until-stop offset of one driver, and a lap outside the laps still to run raise ValueError.  Everything else --
        the remaining arguments, the plans' checks, the simulation ids and draws, the seed rules and the device
        sharding -- is run_strategies': a scenario without offsets gives exactly its counts.  last_histogram:
        [S, n, n]."""
        res = self._run_scenarios(
            'mcgp_run_paces', PaceResult, 'paces / strategies', n_simulations, [self._pace_kind(paces, grid_probs, state)],
            strategies, (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), grid_probs, state, seed,
            sim_offset, drivers, return_orders, allow_single_compound)
        res.until_from = self._until_from(paces)
        return res

    def run_combined(
        self,
        n_simulations: int,
        scenarios: dict,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        grid_probs: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
        return_orders: bool = False,
        allow_single_compound: bool = False,
    ) -> 'CombinedResult':
        """Combined what-if scenarios (include/mcgp.h: mcgp_run_combined, which states how the rule sets meet on one
        lap): the race under each scenario of `scenarios`, {name: {'plans': [PitPlan, ...], 'penalties': [TimePenalty,
        ...], 'events': [RaceEvent, ...], 'paces': [PaceOffset, ...]}}, any of the four keys left out or empty (at most 64
        scenarios, in the order given; the first is the one `compare` measures against).  Each kind keeps the checks
        and limits of its own call (run_strategies, run_penalties, run_events, run_paces), and a scenario with one kind
        of item gives exactly that call's counts.  Everything else -- the remaining arguments, the simulation ids and
        draws, the seed rules and the device sharding -- is run_strategies'.  last_histogram: [S, n, n]."""
        known = ('plans', 'penalties', 'events', 'paces')
        for name, sc in scenarios.items():
            if not isinstance(sc, dict) or set(sc) - set(known):
                raise ValueError(f'scenario {str(name)!r}: a dict with any of the keys {list(known)}, got '
                                 + (f'{sorted(set(sc) - set(known))}' if isinstance(sc, dict) else type(sc).__name__))
        of = lambda key: {str(name): list(sc.get(key) or []) for name, sc in scenarios.items()}
        paces = of('paces')
        res = self._run_scenarios(
            'mcgp_run_combined', CombinedResult, 'scenarios', n_simulations,
            [self._penalty_kind(of('penalties'), state), self._event_kind(of('events'), state),
             self._pace_kind(paces, grid_probs, state)], of('plans'),
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), grid_probs, state, seed, sim_offset,
            drivers, return_orders, allow_single_compound)
        res.until_from = self._until_from(paces)
        return res

    def _change_kind(self, changes, state):
        first = 2 if state is None else int(state.lap) + 1

        def pack(name, chs, index):
            if len(chs) > N.MAX_SCENARIO_TRACK_CHANGES:
                raise ValueError(f'scenario {name!r}: at most {N.MAX_SCENARIO_TRACK_CHANGES} changes, got {len(chs)}')
            packed, covered = [], {}
            for ch in chs:
                try:
                    c = ch.c_struct(first, int(self.config.total_laps))
                except ValueError as e:
                    raise ValueError(f'scenario {name!r}: {e}') from None
                for lap in range(c.first_lap, c.last_lap + 1):
                    if lap in covered:
                        raise ValueError(f'scenario {name!r}: lap {lap} has two changes ({covered[lap]} and {ch})')
                    covered[lap] = ch
                packed.append(c)
            return packed

        return changes, N.McgpTrackChange, pack, ('wrong_laps', lambda S, n, L: (S, n, L + 1))

    def run_weather(
        self,
        n_simulations: int,
        changes: dict,
        strategies: dict | None = None,
        model: 'WeatherModel | None' = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        grid_probs: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
        return_orders: bool = False,
        allow_single_compound: bool = False,
    ) -> 'WeatherResult':
        """Weather scenarios (include/mcgp.h: mcgp_run_weather): the race under each scenario of `changes`, {name:
        [TrackChange, ...]}, and `strategies`, {name: [PitPlan, ...]} or None; a scenario holds the changes and the plans
        given under its name, and the scenario names are the union of the two dicts in the order given (changes first; at
        most 64; the first is the one `compare` measures against).  On the laps a TrackChange covers the track has that
        condition instead of `track_condition`: a red flag's tyre change and the model's pit rule pick their compound
        for it, a car under the rule also stops as soon as it is on the wrong class of tyres (dry tyres on a damp or wet
        track, INTERMEDIATE or WET on a dry one; not in the last five laps), and every car's base pace carries
        `model`'s seconds for its compound under the lap's condition (WeatherModel(): the project's default table).
        A planned driver stops only where its plan says: "stays out" is a plan without a stop on that lap.  From the
        grid a change may name laps 2..L (lap 1 has `track_condition`); from a state, the laps after the state's.
        Overlapping changes in one scenario, an unknown condition and a lap outside those raise ValueError.  The
        two-compound check on plans applies only to a scenario whose track is dry on every lap.  Everything else -- the
        remaining arguments, the plans' other checks, the simulation ids and draws, the seed rules and the device
        sharding -- is run_strategies': a scenario without changes in which nobody is on the wrong tyres gives, under a
        model that is zero there, exactly its counts.  last_histogram: [S, n, n]."""
        model = model if model is not None else WeatherModel()
        L = int(self.config.total_laps)
        first_run = 1 if state is None else int(state.lap) + 1
        changes = {str(k): list(v) for k, v in changes.items()}

        def all_dry(name):
            cond = [str(track_condition)] * (L + 1)
            for ch in changes.get(name, []):
                for lap in range(max(int(ch.first_lap), 0), min(int(ch.last_lap), L) + 1):
                    cond[lap] = str(ch.condition)
            return all(c == 'dry' for c in cond[first_run:])

        return self._run_scenarios(
            'mcgp_run_weather', WeatherResult, 'changes / strategies', n_simulations, [self._change_kind(changes, state)],
            strategies, (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), grid_probs, state, seed,
            sim_offset, drivers, return_orders, allow_single_compound, call_wide=(C.byref(model.c_struct()),),
            all_dry=all_dry)

    def _grid_kind(self, edits):
        def pack(name, eds, index):
            n = len(index)
            if len(eds) > n:
                raise ValueError(f'scenario {name!r}: at most one edit per driver, got {len(eds)} for {n} drivers')
            packed, seen, slots = [], {}, {}
            for ed in eds:
                if str(ed.driver) not in index:
                    raise ValueError(f'scenario {name!r}: {ed.driver!r} is not one of the drivers')
                try:
                    c = ed.c_struct(index)
                except ValueError as e:
                    raise ValueError(f'scenario {name!r}: {e}') from None
                if c.driver in seen:
                    raise ValueError(f'scenario {name!r}: {ed.driver} has two edits ({seen[c.driver]} and {ed})')
                seen[c.driver] = ed
                if c.kind == N.GRID_PIN:
                    if c.value in slots:
                        raise ValueError(f'scenario {name!r}: slot {c.value} is pinned twice ({slots[c.value]} and {ed})')
                    slots[c.value] = ed
                packed.append(c)
            n_pit = sum(1 for c in packed if c.kind == N.GRID_PIT_LANE)
            for slot, ed in slots.items():
                if slot > n - n_pit:
                    raise ValueError(f"scenario {name!r}: {ed}: slot {slot} is one of the last {n_pit}, which the scenario's "
                                     f'pit-lane starters take')
            return packed

        return edits, N.McgpGridEdit, pack, [('start', lambda S, n, L: (S, n, n)),
                                             ('gain', lambda S, n, L: (S, n, 2 * n - 1))]

    def run_grids(
        self,
        n_simulations: int,
        edits: dict,
        strategies: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        grid_probs: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
        return_orders: bool = False,
        allow_single_compound: bool = False,
    ) -> 'GridResult':
        """Grid scenarios (include/mcgp.h: mcgp_run_grids): the race under each scenario of `edits`, {name: [GridEdit,
        ...]}, and `strategies`, {name: [PitPlan, ...]} or None; a scenario holds the edits and the plans given under its
        name, and the scenario names are the union of the two dicts in the order given (edits first; at most 64; the
        first is the one `compare` measures against).  Every simulation draws its grid as run_monte_carlo's does; then
        the scenario's pit-lane starters take the last slots (in their drawn order), its pinned drivers their slots, and
        the others line up by (drawn slot + places dropped, drawn slot) on the slots left, as the reference's
        apply_grid_penalties does for one grid.  The cars start from the new slots: start tyres, lap 1 and every tie
        of times follow them, and a pit-lane starter's lap 1 is longer by its seconds.  At most one edit per driver and
        scenario; two pins on one slot, a pin on a slot the pit-lane starters take and an unknown driver raise
        ValueError.  A mid-race state has no grid: `state` raises ValueError.  Everything else -- the remaining
        arguments, the plans' checks, the simulation ids and draws, the seed rules and the device sharding -- is
        run_strategies': a scenario without edits gives exactly its counts.  last_histogram: [S, n, n]."""
        if state is not None:
            raise ValueError('run_grids runs from the grid: a mid-race state has no grid to edit (state must be None)')
        edits = {str(k): list(v) for k, v in edits.items()}
        return self._run_scenarios(
            'mcgp_run_grids', GridResult, 'edits / strategies', n_simulations, [self._grid_kind(edits)], strategies,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), grid_probs, None, seed, sim_offset,
            drivers, return_orders, allow_single_compound, grid_only=True)

    def run_priors(
        self,
        n_simulations: int,
        priors: dict,
        edges=(),
        strategies: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        grid_probs: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
        return_orders: bool = False,
        return_offsets: bool = False,
        allow_single_compound: bool = False,
    ) -> 'PriorResult':
        """Pace uncertainty (include/mcgp.h: mcgp_run_priors): the race under each scenario of `priors`, {name:
        [PacePrior, ...]}, and `strategies`, {name: [PitPlan, ...]} or None; a scenario holds the priors and the plans
        given under its name, and the scenario names are the union of the two dicts in the order given (priors first; at
        most 64; the first is the one `compare` measures against, so give it no priors to compare against the race as
        forecast).  Every simulation first draws an error of each driver's base pace -- PacePrior.driver's own
        component, PacePrior.group's component shared by its members, both normal with the given sigma in seconds a lap
        -- and races under it, wherever the model reads the base pace.  The deviates depend on the seed, the simulation
        and the driver alone, so scenarios that differ in their sigmas are compared under common random numbers.
        `edges` (at most 15 increasing seconds) bin each driver's own drawn error: the result's `draws` holds its
        finishing distribution by that bin, a pace-sensitivity curve from the same simulations.  A second own prior of
        one driver, a driver in two groups and an unknown driver raise ValueError.  return_offsets: also the drawn errors
        [S, N, n] (binary32).  Everything else -- the remaining arguments, the plans' checks, the simulation ids and the
        race's own draws, the seed rules and the device sharding -- is run_strategies': a scenario without priors gives
        exactly its counts.  last_histogram: [S, n, n]."""
        edge_arr = np.ascontiguousarray(list(edges), np.float64)
        if edge_arr.ndim != 1 or len(edge_arr) > N.MAX_PRIOR_EDGES:
            raise ValueError(f'edges: at most {N.MAX_PRIOR_EDGES} values, got {edge_arr.shape}')
        if not (np.isfinite(edge_arr).all() and (np.diff(edge_arr) > 0).all()):
            raise ValueError('edges must be finite and strictly increasing')
        n_edges = len(edge_arr)
        edge_buf = np.ascontiguousarray(np.concatenate([edge_arr, [0.0]]))      # (never empty: a NULL-free pointer)
        return self._run_scenarios(
            'mcgp_run_priors', PriorResult, 'priors / strategies', n_simulations, [self._prior_kind(priors, n_edges)],
            strategies, (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), grid_probs, state, seed,
            sim_offset, drivers, return_orders, allow_single_compound, call_wide=(n_edges, _dptr(edge_buf)),
            written={'offsets': np.float32 if return_offsets else None}, result_args={'edges': edge_arr})

    @staticmethod
    def _prior_kind(priors, n_edges):
        def pack(name, items, index):
            if len(items) > N.MAX_SCENARIO_PRIORS:
                raise ValueError(f'scenario {name!r}: at most {N.MAX_SCENARIO_PRIORS} priors, got {len(items)}')
            packed, own, grouped = [], {}, {}
            for it in items:
                for code in it.codes:
                    if str(code) not in index:
                        raise ValueError(f'scenario {name!r}: {code!r} is not one of the drivers')
                try:
                    c = it.c_struct(index)
                except ValueError as e:
                    raise ValueError(f'scenario {name!r}: {e}') from None
                if c.kind == N.PRIOR_DRIVER:
                    if c.driver in own:
                        raise ValueError(f'scenario {name!r}: {it.codes[0]} has two own priors ({own[c.driver]} and {it})')
                    own[c.driver] = it
                else:
                    for code in it.codes:
                        if index[str(code)] in grouped:
                            raise ValueError(f'scenario {name!r}: {code} is in two groups ({grouped[index[str(code)]]} and {it})')
                        grouped[index[str(code)]] = it
                packed.append(c)
            return packed

        return priors, N.McgpPacePrior, pack, ('draws', lambda S, n, L: (S, n, n_edges + 1, n))

    def run_gaps(
        self,
        n_simulations: int,
        grid_probs: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        state: 'RaceState | None' = None,
        edges=None,
        pairs=(),
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
    ) -> 'GapResult':
        """Race time gaps (include/mcgp.h: mcgp_run_gaps): histograms over `edges` (seconds, default DEFAULT_GAP_EDGES) of
        every car's gap to the leader after each lap, of the lead (the winning margin on the last lap) and of the gap
        between each of `pairs` = [(driver a, driver b), ...] (at most 64), counted on the device.  From the grid
        (grid_probs: run_monte_carlo's simulations, laps 1..L) or from a mid-race RaceState (state: run_from_state's
        simulations, the laps after the state's).  The GapResult's position histogram equals that call's.  32-bit
        deviates only; same seed rules and device sharding as run_monte_carlo.  Sets last_histogram / last_drivers."""
        src = self._source(grid_probs, state, drivers)
        drivers = src.drivers
        edge_arr = _gap_edge_array(edges)
        index = {d: i for i, d in enumerate(drivers)}
        names = [(str(a), str(b)) for a, b in pairs]
        for a, b in names:
            if a not in index or b not in index:
                raise ValueError(f'pair ({a!r}, {b!r}): not among the drivers')
            if a == b:
                raise ValueError(f'pair ({a!r}, {b!r}): a pair needs two different drivers')
        if len(names) > N.MAX_GAP_PAIRS:
            raise ValueError(f'pairs: at most {N.MAX_GAP_PAIRS}, got {len(names)}')
        n, L, E, P = len(drivers), int(self.config.total_laps), len(edge_arr), len(names)
        n_simulations = int(n_simulations)
        first_lap = src.first_lap(1)
        pair_arr = np.ascontiguousarray([[index[a], index[b]] for a, b in names], np.uint8).reshape(P, 2)
        total = self._run_entry(
            'mcgp_run_gaps', n_simulations, drivers,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), seed, sim_offset,
            lambda n: src.c_args() + (n, E, _dptr(edge_arr), P, _optr(pair_arr) if P else None),
            lambda count: _count_arrays(GapResult.empty(drivers, L, edge_arr, names, count, first_lap, np.uint64)),
            ['hist', 'lap_gap', 'lead', 'pair' if P else None])
        return GapResult(drivers=drivers, n_simulations=n_simulations if drivers and n_simulations > 0 else 0,
                         total_laps=L, edges=tuple(float(x) for x in edge_arr), pairs=names, first_lap=first_lap, **total)

    def run_pit_windows(
        self,
        n_simulations: int,
        grid_probs: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        state: 'RaceState | None' = None,
        windows=(),
        edges=None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
    ) -> 'PitWindowResult':
        """Pit windows (include/mcgp.h: mcgp_run_pit_windows): for each of `windows` = [(driver, loss in seconds or None:
        config.pit_loss), ...] (1 to 64; a driver may appear with several losses) and every lap, where the driver would
        rejoin if it stopped at the end of that lap and lost that much -- position, places lost, the car ahead and the
        gaps ahead and behind over `edges` (seconds, default DEFAULT_GAP_EDGES) --, counted on the device.  Nothing is
        re-simulated: the races are run_monte_carlo's (grid_probs, laps 1..L) or run_from_state's (state, the laps after
        the state's), unmodified, and the PitWindowResult's position histogram equals that call's; the race AFTER a stop
        is run_strategies' question.  32-bit deviates only; same seed rules and device sharding as run_gaps.  Sets
        last_histogram / last_drivers."""
        src = self._source(grid_probs, state, drivers)
        drivers = src.drivers
        edge_arr = _gap_edge_array(edges)
        index = {d: i for i, d in enumerate(drivers)}
        wins = [(str(d), float(self.config.pit_loss if loss is None else loss)) for d, loss in windows]
        if not 1 <= len(wins) <= N.MAX_PIT_WINDOWS:
            raise ValueError(f'windows: 1 to {N.MAX_PIT_WINDOWS}, got {len(wins)}')
        for d, loss in wins:
            if d not in index:
                raise ValueError(f'window ({d!r}, {loss:g}): not among the drivers')
            if not (math.isfinite(loss) and loss >= 0):
                raise ValueError(f'window ({d!r}, {loss!r}): the loss must be finite and >= 0')
        L, E, W = int(self.config.total_laps), len(edge_arr), len(wins)
        n_simulations = int(n_simulations)
        first_lap = src.first_lap(1)
        driver_arr = np.ascontiguousarray([index[d] for d, _ in wins], np.uint8)
        loss_arr = np.ascontiguousarray([loss for _, loss in wins], np.float64)
        total = self._run_entry(
            'mcgp_run_pit_windows', n_simulations, drivers,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), seed, sim_offset,
            lambda n: src.c_args() + (n, E, _dptr(edge_arr), W, _optr(driver_arr), _dptr(loss_arr)),
            lambda count: _count_arrays(PitWindowResult.empty(drivers, L, edge_arr, wins, count, first_lap, np.uint64)),
            ['hist', 'rejoin', 'lost', 'ahead', 'gap_ahead', 'gap_behind'])
        return PitWindowResult(drivers=drivers, n_simulations=n_simulations if drivers and n_simulations > 0 else 0,
                               total_laps=L, edges=tuple(float(x) for x in edge_arr), windows=wins, first_lap=first_lap,
                               **total)

    def run_stints(
        self,
        n_simulations: int,
        grid_probs: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
    ) -> 'StintResult':
        """Tyre stints (include/mcgp.h: mcgp_run_stints): on which lap the race model makes each driver's first four pit
        stops, which compound sequence the driver runs (red-flag tyre changes start a stint too) and how the finishing
        positions split by stop count, counted on the device.  From the grid (grid_probs: run_monte_carlo's simulations,
        laps 2..L) or from a mid-race RaceState (state: run_from_state's simulations, the laps after the state's; earlier
        stops are not part of a state).  The StintResult's position histogram equals that call's.  32-bit deviates only;
        same seed rules and device sharding as run_monte_carlo.  Sets last_histogram / last_drivers."""
        src = self._source(grid_probs, state, drivers)
        drivers, L, n_simulations = src.drivers, int(self.config.total_laps), int(n_simulations)
        total = self._run_entry(
            'mcgp_run_stints', n_simulations, drivers,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), seed, sim_offset,
            lambda n: src.c_args() + (n,),
            lambda count: _count_arrays(StintResult.empty(drivers, L, count, src.first_lap(), np.uint64)),
            ['hist', 'stop_lap', 'stops_pos', 'seq'])
        return StintResult(drivers=drivers, n_simulations=n_simulations if drivers and n_simulations > 0 else 0,
                           total_laps=L, first_lap=src.first_lap(), **total)

    def run_moves(
        self,
        n_simulations: int,
        grid_probs: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
    ) -> 'MoveResult':
        """Race movement (include/mcgp.h: mcgp_run_moves): the joint grid x finish table, the places won or lost at the
        start, and the model's order changes between lap ends -- passes made and lost per driver, on track and through
        the pits, per race, per lap and per pair -- counted on the device.  From the grid (grid_probs: run_monte_carlo's
        simulations, passes on laps 2..L) or from a mid-race RaceState (state: run_from_state's simulations, the laps
        after the state's; no start gain).  The MoveResult's position histogram equals that call's.  32-bit deviates
        only; same seed rules and device sharding as run_monte_carlo.  Sets last_histogram / last_drivers."""
        src = self._source(grid_probs, state, drivers)
        drivers, L, n_simulations = src.drivers, int(self.config.total_laps), int(n_simulations)
        total = self._run_entry(
            'mcgp_run_moves', n_simulations, drivers,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), seed, sim_offset,
            lambda n: src.c_args() + (n,),
            lambda count: _count_arrays(MoveResult.empty(drivers, L, count, src.first_lap(), state is None, np.uint64)),
            ['hist', 'grid_fin', 'start_gain' if state is None else None, 'passes', 'race_passes', 'lap_passes',
             'pair_passes'])
        return MoveResult(drivers=drivers, n_simulations=n_simulations if drivers and n_simulations > 0 else 0,
                          total_laps=L, first_lap=src.first_lap(), from_grid=state is None, **total)

    def run_conditions(
        self,
        n_simulations: int,
        conditions: dict,
        grid_probs: dict | None = None,
        base_pace: dict | None = None,
        tire_deg: dict | None = None,
        driver_variance: dict | None = None,
        driver_dnf_rates: dict | None = None,
        state: 'RaceState | None' = None,
        seed: int | None = None,
        track_condition: str = 'dry',
        sim_offset: int = 0,
        drivers=None,
        histograms: bool = True,
    ) -> 'ConditionResult':
        """Combination and conditional odds (include/mcgp.h: mcgp_run_conditions): `conditions` = {name: text or
        Condition} (1 to 64; the grammar is in conditions.py), each evaluated on the device inside every simulation.
        Counted per condition: the simulations that met it and, unless histograms is False (the result's cond_hist is
        then None and it has no conditional odds to give), the position histogram among those.  From the grid (grid_probs: run_monte_carlo's simulations) or from a mid-race RaceState (state:
        run_from_state's simulations; race events count from the state's lap on).  The ConditionResult's position
        histogram equals that call's.  32-bit deviates only; same seed rules and device sharding as run_monte_carlo.
        Sets last_histogram / last_drivers."""
        from . import conditions as CD
        src = self._source(grid_probs, state, drivers)
        drivers = src.drivers
        parsed = CD.parse_all(conditions, drivers)
        names = list(parsed)
        n, K = len(drivers), len(names)
        n_simulations = int(n_simulations)
        total = self._run_entry(
            'mcgp_run_conditions', n_simulations, drivers,
            (base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition), seed, sim_offset,
            lambda n: src.c_args() + (n, K, CD.c_array(parsed)),
            lambda count: dict(hist=np.zeros((n, n), np.uint64), count=np.zeros(K, np.uint64),
                               cond_hist=np.zeros((K, n, n), np.uint64) if histograms else None),
            ['hist', 'count', 'cond_hist'])
        return CD.ConditionResult(drivers=drivers, names=names, n_simulations=max(n_simulations, 0), hist=total['hist'],
                                  counts={k: int(c) for k, c in zip(names, total['count'])}, cond_hist=total['cond_hist'])

    def simulate_race(
        self,
        grid: list,
        base_pace: dict,
        tire_deg: dict,
        driver_variance: dict,
        driver_dnf_rates: dict | None = None,
        track_condition: str = 'dry',
        seed: int | None = None,
        sim_id: int = 0,
    ):
        """Simulate a single race from a fixed grid; returns [(driver, position)] (reference :147-242)."""
        drivers = [str(d) for d in grid]
        if not drivers:
            return []
        prob = self._problem(drivers, base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition)
        n = prob.n
        g = np.arange(n, dtype=np.uint8)           # driver index == grid slot here
        order = np.zeros(n, np.uint8)
        N.check(N.lib().mcgp_simulate_race(
            C.byref(prob.cfg), C.byref(prob.drv), g.ctypes.data_as(C.POINTER(C.c_uint8)), n, int(sim_id),
            self._resolve_seed(seed), self.device, order.ctypes.data_as(C.POINTER(C.c_uint8))))
        return [(drivers[int(d)], p + 1) for p, d in enumerate(order)]

    # ------------------------------------------------------------------ device grid-probability front end
    @staticmethod
    def front_end_arrays(drivers, quali_ratings, quali_features=None, penalties=None, initial_rating=1500.0):
        """Dense inputs of the device front end with the reference's .get() defaults resolved
        (src/elo.py:131 initial rating; src/predictor.py:335,352-354 features default 0; :386-390 penalties)."""
        from .predictor import _penalty_value
        quali_features, penalties = quali_features or {}, penalties or {}
        f = lambda key: np.array([quali_features.get(d, {}).get(key, 0) for d in drivers], np.float64)
        rating = np.array([quali_ratings.get(d, initial_rating) for d in drivers], np.float64)
        pen = np.array([int(_penalty_value(penalties.get(d, 0))) for d in drivers], np.int32)
        return rating, f('teammate_delta'), f('form_score'), f('circuit_affinity'), pen

    def grid_probs_on_device(self, drivers, quali_ratings, quali_features=None, penalties=None):
        """{driver: [P(grid slot)]} computed by the device front end (include/mcgp.h: mcgp_grid_probs)."""
        drivers = [str(d) for d in drivers]
        n = len(drivers)
        r, td, fs, ca, pen = self.front_end_arrays(drivers, quali_ratings, quali_features, penalties)
        out = np.zeros((n, n), np.float64)
        N.check(N.lib().mcgp_grid_probs(_dptr(r), _dptr(td), _dptr(fs), _dptr(ca),
                                        pen.ctypes.data_as(C.POINTER(C.c_int32)), n, self.device, _dptr(out)))
        return {d: [float(x) for x in out[i]] for i, d in enumerate(drivers)}

    def run_from_ratings(self, n_simulations, drivers, quali_ratings, quali_features, penalties, base_pace, tire_deg,
                         driver_variance, driver_dnf_rates=None, seed=None, track_condition='dry', sim_offset=0):
        """run_monte_carlo with the grid matrix built ON THE DEVICE from the Elo quali ratings and features and
        handed to the race kernel without a host round trip (mcgp_run_from_ratings).
        Returns (position probabilities as run_monte_carlo does, {driver: [P(grid slot)]})."""
        drivers = [str(d) for d in drivers]
        prob = self._problem(drivers, base_pace, tire_deg, driver_variance, driver_dnf_rates, track_condition)
        n = prob.n
        r, td, fs, ca, pen = self.front_end_arrays(drivers, quali_ratings, quali_features, penalties)
        hist = np.zeros((n, n), np.uint64)
        grid = np.zeros((n, n), np.float64)
        N.check(N.lib().mcgp_run_from_ratings(
            C.byref(prob.cfg), C.byref(prob.drv), _dptr(r), _dptr(td), _dptr(fs), _dptr(ca),
            pen.ctypes.data_as(C.POINTER(C.c_int32)), n, int(n_simulations), int(sim_offset), self._resolve_seed(seed),
            self.device, hist.ctypes.data_as(C.POINTER(C.c_uint64)), _dptr(grid)))
        self.last_histogram = hist.astype(np.int64)
        self.last_drivers = drivers
        return (histogram_to_probs(self.last_histogram, drivers, n_simulations),
                {d: [float(x) for x in grid[i]] for i, d in enumerate(drivers)})

    # ------------------------------------------------------------------ north-star alias
    def set_race_inputs(self, base_pace=None, tire_deg=None, driver_variance=None, driver_dnf_rates=None,
                        track_condition='dry'):
        """Per-race inputs used by run_simulations(); missing dicts fall back to the reference defaults."""
        self._race_inputs = dict(base_pace=base_pace or {}, tire_deg=tire_deg or {},
                                 driver_variance=driver_variance or {}, driver_dnf_rates=driver_dnf_rates,
                                 track_condition=track_condition)
        return self

    def run_simulations(self, grid: dict, n_sims: int, seed: int | None = None):
        """run_simulations(grid, n_sims, seed): thin wrapper over run_monte_carlo (BASELINE north star)."""
        ri = self._race_inputs or dict(base_pace={}, tire_deg={}, driver_variance={}, driver_dnf_rates=None,
                                       track_condition='dry')
        return self.run_monte_carlo(n_sims, grid, ri['base_pace'], ri['tire_deg'], ri['driver_variance'],
                                    ri['driver_dnf_rates'], seed=seed, track_condition=ri['track_condition'])


def run_monte_carlo_batch(problems, n_simulations, device=0, set_pop=None):
    """Several races in ONE launch (include/mcgp.h: mcgp_run_batch): what a backtest of the reference does race after
    race (reference src/validation.py:179-185, 10 000 simulations each, src/predictor.py:284) -- at that size a launch
    is as long as one race of one lane, and a season fits beside itself on the device.

    `problems`: a list of dicts with the keys `config` (RaceConfig) and run_monte_carlo's arguments `grid_probs`,
    `base_pace`, `tire_deg`, `driver_variance`, and optionally `driver_dnf_rates`, `seed`, `track_condition`,
    `sim_offset`, `deviates` (32 or 53).  Returns a list of (probabilities as run_monte_carlo returns them, integer
    histogram [n, n]), one per problem and bit-identical to running it alone.  Races of different field sizes go into
    one launch per size; a problem the shared launch does not take (deviates = 53, or one only the generic kernel
    serves) runs by itself inside the same call -- no problem can make another one fail."""
    set_pop = dict(set_pop or DEFAULT_SET_POP)
    lib = N.lib()
    n_simulations = int(n_simulations)
    prepared = []
    for pr in problems:
        drivers = [str(d) for d in pr['grid_probs'].keys()]
        if not (1 <= len(drivers) <= N.MAX_CARS):
            raise ValueError(f'number of drivers must be in [1, {N.MAX_CARS}], got {len(drivers)}')
        prob = _Problem(pr['config'], drivers, pr['base_pace'], pr['tire_deg'], pr['driver_variance'],
                        pr.get('driver_dnf_rates'), pr.get('track_condition', 'dry'), set_pop, pr.get('deviates', 32))
        g = RaceSimulator._grid_matrix({str(k): v for k, v in pr['grid_probs'].items()}, drivers)
        prepared.append((prob, g, RaceSimulator._resolve_seed(pr.get('seed')), int(pr.get('sim_offset', 0))))
    out = [None] * len(prepared)
    if n_simulations <= 0:
        return [({}, np.zeros((p.n, p.n), np.int64)) for p, _, _, _ in prepared]
    by_n = {}
    for i, item in enumerate(prepared):
        by_n.setdefault(item[0].n, []).append(i)
    for n, idx in by_n.items():
        k = len(idx)
        cfgs = (N.McgpConfig * k)(*[prepared[i][0].cfg for i in idx])
        drvs = (N.McgpDrivers * k)(*[prepared[i][0].drv for i in idx])
        grids = (C.POINTER(C.c_double) * k)(*[_dptr(prepared[i][1]) for i in idx])
        seeds = (C.c_uint64 * k)(*[prepared[i][2] for i in idx])
        offsets = (C.c_uint64 * k)(*[prepared[i][3] for i in idx])
        hist = np.zeros((k, n, n), np.uint64)
        N.check(lib.mcgp_run_batch(k, cfgs, drvs, grids, n, n_simulations, offsets, seeds, int(device),
                                   hist.ctypes.data_as(C.POINTER(C.c_uint64))))
        for j, i in enumerate(idx):
            h = hist[j].astype(np.int64)
            out[i] = (histogram_to_probs(h, prepared[i][0].drivers, n_simulations), h)
    return out


@dataclass
class MatchupResult:
    """What RaceSimulator.run_matchups returns.  Integer counts over n_simulations: hist [n][n] = [driver][position - 1]
    (run_monte_carlo's histogram), ahead [n][n] = [i][j] simulations in which driver i is classified ahead of driver j,
    podium [n][n][n] = [a][b][c] simulations whose first three classified cars are a, b, c in that order (None when not
    asked for or with fewer than 3 drivers).  Classified: the race model's order, which puts retired cars behind the
    finishers, as the reference does; a pair whose cars both retire counts in that order too."""
    drivers: list
    n_simulations: int
    hist: np.ndarray
    ahead: np.ndarray
    podium: np.ndarray | None = None

    @property
    def position_probabilities(self) -> dict:
        """{driver: {position: probability}}, what run_monte_carlo returns for the same arguments."""
        return histogram_to_probs(self.hist, self.drivers, self.n_simulations)

    def head_to_head(self, a, b) -> float:
        """P(driver a classified ahead of driver b)."""
        i, j = self.drivers.index(str(a)), self.drivers.index(str(b))
        return int(self.ahead[i, j]) / self.n_simulations if self.n_simulations else 0.0

    @property
    def ahead_probabilities(self) -> dict:
        """{a: {b: P(a ahead of b)}} for every ordered pair of distinct drivers."""
        n = max(self.n_simulations, 1)
        return {a: {b: int(self.ahead[i, j]) / n for j, b in enumerate(self.drivers) if j != i}
                for i, a in enumerate(self.drivers)}

    def teammate_battles(self, driver_teams: dict) -> list:
        """Every pair of drivers of one team (driver_teams: {driver: team}; drivers it does not list have no team), in
        field order: [{'team', 'drivers': [a, b], 'probabilities': [P(a ahead), P(b ahead)]}]."""
        out = []
        for i, a in enumerate(self.drivers):
            for b in self.drivers[i + 1:]:
                team = driver_teams.get(a)
                if team is not None and driver_teams.get(b) == team:
                    p = self.head_to_head(a, b)
                    out.append({'team': team, 'drivers': [a, b], 'probabilities': [p, self.head_to_head(b, a)]})
        return out

    def podium_set_probabilities(self) -> dict:
        """{frozenset of three drivers: P(those three make the podium, in any order)}, non-zero sets only."""
        self._need_podium()
        out = {}
        for a, b, c in zip(*np.nonzero(self.podium)):
            key = frozenset((self.drivers[a], self.drivers[b], self.drivers[c]))
            out[key] = out.get(key, 0) + int(self.podium[a, b, c])
        return {k: v / self.n_simulations for k, v in out.items()}

    def most_likely_podiums(self, k: int = 10) -> list:
        """The k most likely ordered podiums: [((P1, P2, P3), probability)], most likely first (ties in cell order)."""
        self._need_podium()
        flat = self.podium.ravel()
        nz = np.nonzero(flat)[0]
        top = nz[np.argsort(-flat[nz], kind='stable')][:max(int(k), 0)]
        n, d = len(self.drivers), self.drivers
        return [((d[c // (n * n)], d[c // n % n], d[c % n]), int(flat[c]) / self.n_simulations) for c in top]

    def _need_podium(self):
        if self.podium is None:
            raise ValueError('no podium counts: run_matchups(podiums=True) with at least 3 drivers')


RACE_EVENTS = ('red_flag', 'safety_car', 'vsc')          # the rows of TraceResult.events


@dataclass
class TraceResult:
    """What RaceSimulator.run_trace returns: integer counts over n_simulations of what happened lap by lap, read after the
    end of each lap (include/mcgp.h: mcgp_run_trace has the definitions).  L = total_laps, n = len(drivers):
      hist      [n][n]        [driver][position - 1], run_monte_carlo's histogram
      lap_pos   [L][n][n + 1] [lap - 1][driver][running position - 1, or n = retired]
      laps_led  [n][L + 1]    [driver][laps led]
      stops     [n][L + 1]    [driver][pit stops]
      fastest   [n]           simulations in which the driver sets the fastest lap (laps 2..L)
      events    [3][L + 1]    [red flag, safety car, VSC][number in the race]"""
    drivers: list
    n_simulations: int
    total_laps: int
    hist: np.ndarray
    lap_pos: np.ndarray
    laps_led: np.ndarray
    stops: np.ndarray
    fastest: np.ndarray
    events: np.ndarray

    @classmethod
    def empty(cls, drivers, total_laps, n_simulations=0, dtype=np.int64) -> 'TraceResult':
        n, L = len(drivers), int(total_laps)
        z = lambda *shape: np.zeros(shape, dtype)
        return cls(drivers=list(drivers), n_simulations=int(n_simulations), total_laps=L, hist=z(n, n),
                   lap_pos=z(L, n, n + 1), laps_led=z(n, L + 1), stops=z(n, L + 1), fastest=z(n), events=z(3, L + 1))

    def _p(self, counts):
        return np.asarray(counts, np.float64) / max(self.n_simulations, 1)

    @property
    def position_probabilities(self) -> dict:
        """{driver: {position: probability}}, what run_monte_carlo returns for the same arguments."""
        return histogram_to_probs(self.hist, self.drivers, self.n_simulations)

    @property
    def position_probabilities_by_lap(self) -> dict:
        """{driver: [L][n + 1] array}: P(running position p + 1 after lap k + 1), last column P(retired by then)."""
        p = self._p(self.lap_pos)
        return {d: p[:, i, :] for i, d in enumerate(self.drivers)}

    @property
    def leader_probabilities(self) -> dict:
        """{driver: [L] array}: P(leading the race after lap k + 1) -- the lap chart."""
        p = self._p(self.lap_pos[:, :, 0])
        return {d: p[:, i] for i, d in enumerate(self.drivers)}

    @property
    def retired_by_lap(self) -> dict:
        """{driver: [L] array}: P(retired by the end of lap k + 1)."""
        p = self._p(self.lap_pos[:, :, -1])
        return {d: p[:, i] for i, d in enumerate(self.drivers)}

    @property
    def laps_led_distribution(self) -> dict:
        """{driver: [L + 1] array}: P(leading exactly j laps)."""
        p = self._p(self.laps_led)
        return {d: p[i] for i, d in enumerate(self.drivers)}

    @property
    def expected_laps_led(self) -> dict:
        j = np.arange(self.total_laps + 1)
        return {d: float(self._p(self.laps_led[i]) @ j) for i, d in enumerate(self.drivers)}

    @property
    def pit_stop_distribution(self) -> dict:
        """{driver: [L + 1] array}: P(exactly j pit stops)."""
        p = self._p(self.stops)
        return {d: p[i] for i, d in enumerate(self.drivers)}

    @property
    def expected_pit_stops(self) -> dict:
        j = np.arange(self.total_laps + 1)
        return {d: float(self._p(self.stops[i]) @ j) for i, d in enumerate(self.drivers)}

    @property
    def fastest_lap_probabilities(self) -> dict:
        """{driver: P(sets the fastest lap)}; they sum to less than 1 when some races have no lap 2 completed."""
        p = self._p(self.fastest)
        return {d: float(p[i]) for i, d in enumerate(self.drivers)}

    @property
    def event_probabilities(self) -> dict:
        """{'red_flag' | 'safety_car' | 'vsc': {'probability': P(at least one), 'expected': expected number}}."""
        j = np.arange(self.total_laps + 1)
        out = {}
        for k, name in enumerate(RACE_EVENTS):
            p = self._p(self.events[k])
            out[name] = {'probability': float(1.0 - p[0]) if self.n_simulations else 0.0, 'expected': float(p @ j)}
        return out


DEFAULT_GAP_EDGES = (0.5, 1, 2, 3, 5, 7.5, 10, 15, 20, 30, 45, 60, 90, 120)      # seconds


@dataclass
class GapResult:
    """What RaceSimulator.run_gaps returns: integer counts over n_simulations of the race's time gaps, read after the end
    of each lap (include/mcgp.h: mcgp_run_gaps has the definitions).  L = total_laps, n = len(drivers), B = len(edges)
    + 1 bins: bin b holds gaps in [edges[b - 1], edges[b]), bin 0 from 0, bin B - 1 without an upper bound.
      hist     [n][n]            [driver][position - 1], run_monte_carlo's / run_from_state's histogram
      lap_gap  [L][n][B + 1]     [lap - 1][driver][bin of the gap to the leader], column B = retired
      lead     [L][B + 1]        [lap - 1][bin of second minus leader], column B = fewer than two cars running
      pair     [L][P][2B + 1]    [lap - 1][pair (a, b)][bin of b - a with a ahead | B + bin of a - b with b ahead | 2B =
                                 either retired]
    Laps before first_lap (a run from a state) are not recorded: their rows are zero.  The counts carry no value between
    two edges, so every reader answers in terms of edges and bins, never an interpolated number."""
    drivers: list
    n_simulations: int
    total_laps: int
    edges: tuple
    pairs: list
    first_lap: int
    hist: np.ndarray
    lap_gap: np.ndarray
    lead: np.ndarray
    pair: np.ndarray

    @classmethod
    def empty(cls, drivers, total_laps, edges, pairs=(), n_simulations=0, first_lap=1, dtype=np.int64) -> 'GapResult':
        n, L, B, P = len(drivers), int(total_laps), len(edges) + 1, len(pairs)
        z = lambda *shape: np.zeros(shape, dtype)
        return cls(drivers=list(drivers), n_simulations=int(n_simulations), total_laps=L,
                   edges=tuple(float(x) for x in edges), pairs=[(str(a), str(b)) for a, b in pairs],
                   first_lap=int(first_lap), hist=z(n, n), lap_gap=z(L, n, B + 1), lead=z(L, B + 1), pair=z(L, P, 2 * B + 1))

    @property
    def n_bins(self) -> int:
        return len(self.edges) + 1

    def _p(self, counts):
        return np.asarray(counts, np.float64) / max(self.n_simulations, 1)

    def _d(self, driver):
        try:
            return self.drivers.index(str(driver))
        except ValueError:
            raise ValueError(f'{driver!r} is not one of the drivers') from None

    def _lap(self, lap):
        lap = self.total_laps if lap is None else int(lap)
        if not self.first_lap <= lap <= self.total_laps:
            raise ValueError(f'lap must be in [{self.first_lap}, {self.total_laps}], got {lap}')
        return lap - 1

    def _edge(self, seconds):
        """The number of bins below `seconds`, which must be an edge: the counts cannot answer anything else."""
        for j, e in enumerate(self.edges):
            if e == float(seconds):
                return j + 1
        raise ValueError(f'{seconds!r} is not one of the edges {self.edges}: the counts cannot answer it')

    def _pair(self, a, b):
        """(index, mirrored): the pair as given, or as its mirror image."""
        a, b = str(a), str(b)
        if (a, b) in self.pairs:
            return self.pairs.index((a, b)), False
        if (b, a) in self.pairs:
            return self.pairs.index((b, a)), True
        raise ValueError(f'({a!r}, {b!r}) is not one of the pairs {self.pairs}')

    def bin_bounds(self, b) -> tuple:
        """(low, high) of bin b in seconds; the last bin's high is inf."""
        b = int(b)
        if not 0 <= b < self.n_bins:
            raise ValueError(f'bin must be in [0, {self.n_bins - 1}], got {b}')
        return (0.0 if b == 0 else self.edges[b - 1], self.edges[b] if b < len(self.edges) else math.inf)

    @property
    def position_probabilities(self) -> dict:
        """{driver: {position: probability}}, what run_monte_carlo / run_from_state returns for the same arguments."""
        return histogram_to_probs(self.hist, self.drivers, self.n_simulations)

    def gap_distribution(self, driver, lap=None) -> np.ndarray:
        """[B + 1]: P(gap to the leader in bin b after `lap`), last entry P(retired by then).  lap None: the flag (the
        finishing-gap distribution)."""
        return self._p(self.lap_gap[self._lap(lap), self._d(driver)])

    @property
    def finishing_gap_distributions(self) -> dict:
        """{driver: [B + 1] array} at the flag."""
        return {d: self.gap_distribution(d) for d in self.drivers}

    def within(self, driver, seconds, lap=None) -> float:
        """P(running and less than `seconds` behind the leader after `lap`; None: at the flag).  `seconds` must be one
        of the edges (ValueError otherwise).  The leader is within every edge."""
        j = self._edge(seconds)
        return float(self._p(self.lap_gap[self._lap(lap), self._d(driver), :j].sum()))

    @property
    def winning_margin_distribution(self) -> np.ndarray:
        """[B + 1]: P(second finishes in bin b behind the winner), last entry P(fewer than two cars finish)."""
        return self._p(self.lead[self.total_laps - 1])

    def winning_margin_under(self, seconds) -> float:
        """P(two cars finish and the margin is less than `seconds`), an edge."""
        return float(self._p(self.lead[self.total_laps - 1, :self._edge(seconds)].sum()))

    @property
    def lead_by_lap(self) -> np.ndarray:
        """[L][B + 1]: the distribution of the leader's advantage over second after every lap."""
        return self._p(self.lead)

    def median_gap_bin_by_lap(self, driver) -> list:
        """[L] of (low, high): the bounds of the bin that holds the median gap to the leader among the simulations in
        which the driver is running after that lap; None for a lap that is not recorded or on which it never runs."""
        i, B, out = self._d(driver), self.n_bins, []
        for k in range(self.total_laps):
            c = self.lap_gap[k, i, :B]
            tot = int(c.sum())
            if tot == 0:
                out.append(None)
                continue
            # the lower median: the smallest bin b with 2 x (count up to and including b) >= the number running
            b = int(np.searchsorted(2 * np.cumsum(c), tot, side='left'))
            out.append(self.bin_bounds(b))
        return out

    def pair_summary(self, a, b, lap=None) -> dict:
        """{'a_ahead', 'b_ahead', 'either_out'}: probabilities after `lap` (None: at the flag) for a requested pair, in
        either orientation."""
        p, mirrored = self._pair(a, b)
        B = self.n_bins
        c = self.pair[self._lap(lap), p]
        first, second = float(self._p(c[:B].sum())), float(self._p(c[B:2 * B].sum()))      # (counts summed, then divided)
        if mirrored:
            first, second = second, first
        return {'a_ahead': first, 'b_ahead': second, 'either_out': float(self._p(c[2 * B]))}

    def pair_within_by_lap(self, a, b, seconds) -> np.ndarray:
        """[L]: P(both running and |gap| < seconds after each lap), `seconds` an edge -- e.g. 1.0 for DRS range, or the
        pit-stop loss for "is a stop free"."""
        p, _ = self._pair(a, b)
        j, B = self._edge(seconds), self.n_bins
        return self._p(self.pair[:, p, :j].sum(axis=1) + self.pair[:, p, B:B + j].sum(axis=1))


IN_THE_LEAD = 'in the lead'            # PitWindowResult.rejoins_behind's entry for a rejoin with no car ahead


@dataclass
class PitWindowResult:
    """What RaceSimulator.run_pit_windows returns: integer counts over n_simulations of where a driver would rejoin if it
    stopped at the end of a lap and lost `loss` seconds (include/mcgp.h: mcgp_run_pit_windows has the definitions).
    Nothing is re-simulated: the races are the unmodified ones, and a window asks a question of their times after each
    lap.  L = total_laps, n = len(drivers), W = len(windows) = [(driver, loss), ...], B = len(edges) + 1 bins as
    GapResult has them.
      hist        [n][n]          [driver][position - 1], run_monte_carlo's / run_from_state's histogram
      rejoin      [L][W][n + 1]   [lap - 1][window][rejoin position, 0-based], column n = the driver has retired
      lost        [L][W][n + 1]   [lap - 1][window][places lost], column n = retired; 0 is a free stop
      ahead       [L][W][n + 2]   [lap - 1][window][index of the car ahead at rejoin], n = rejoins in the lead, n + 1 = retired
      gap_ahead   [L][W][B + 1]   [lap - 1][window][bin of the gap to the car ahead], column B = no car ahead, or retired
      gap_behind  [L][W][B + 1]   [lap - 1][window][bin of the gap to the car behind], column B = no car behind, or retired
    Laps before first_lap (a run from a state) are not recorded: their rows are zero.  Every reader that speaks of the
    rejoin is CONDITIONAL ON THE DRIVER RUNNING after that lap (a retired car has no stop to make); running_probability
    gives the condition's own probability.  A window `w` is named by its index, by (driver, loss), or by the driver alone
    where only one window names it.  The counts carry no value between two edges: `seconds` must be an edge."""
    drivers: list
    n_simulations: int
    total_laps: int
    edges: tuple
    windows: list
    first_lap: int
    hist: np.ndarray
    rejoin: np.ndarray
    lost: np.ndarray
    ahead: np.ndarray
    gap_ahead: np.ndarray
    gap_behind: np.ndarray

    @classmethod
    def empty(cls, drivers, total_laps, edges, windows, n_simulations=0, first_lap=1, dtype=np.int64) -> 'PitWindowResult':
        n, L, B, W = len(drivers), int(total_laps), len(edges) + 1, len(windows)
        z = lambda *shape: np.zeros(shape, dtype)
        return cls(drivers=list(drivers), n_simulations=int(n_simulations), total_laps=L,
                   edges=tuple(float(x) for x in edges), windows=[(str(d), float(loss)) for d, loss in windows],
                   first_lap=int(first_lap), hist=z(n, n), rejoin=z(L, W, n + 1), lost=z(L, W, n + 1), ahead=z(L, W, n + 2),
                   gap_ahead=z(L, W, B + 1), gap_behind=z(L, W, B + 1))

    _lap = GapResult._lap
    _edge = GapResult._edge

    def _w(self, w) -> int:
        if isinstance(w, (int, np.integer)):
            if not 0 <= int(w) < len(self.windows):
                raise ValueError(f'window index must be in [0, {len(self.windows) - 1}], got {w}')
            return int(w)
        if isinstance(w, str):
            hits = [i for i, (d, _) in enumerate(self.windows) if d == w]
            if len(hits) != 1:
                raise ValueError(f'{w!r} names {len(hits)} of the windows {self.windows}: give (driver, loss) or an index')
            return hits[0]
        key = (str(w[0]), float(w[1]))
        if key not in self.windows:
            raise ValueError(f'{key!r} is not one of the windows {self.windows}')
        return self.windows.index(key)

    @staticmethod
    def _given_running(counts) -> np.ndarray:
        """counts [..., k + 1] (last column: retired) -> [..., k] probabilities among the simulations in which the driver
        runs; nan where there is none (a lap that is not recorded, or a car that is always out by then)."""
        c = np.asarray(counts[..., :-1], np.float64)
        tot = c.sum(axis=-1, keepdims=True)
        return np.divide(c, tot, out=np.full(c.shape, np.nan), where=tot > 0)

    def position_probabilities(self) -> dict:
        """{driver: {position: probability}}, what run_monte_carlo / run_from_state returns for the same arguments."""
        return histogram_to_probs(self.hist, self.drivers, self.n_simulations)

    def running_probability(self, w) -> np.ndarray:
        """[L]: P(the window's driver is running after each lap) -- what the other readers are conditional on; 0 for a lap
        that is not recorded."""
        n = len(self.drivers)
        return self.rejoin[:, self._w(w), :n].sum(axis=1) / max(self.n_simulations, 1)

    def rejoin_distribution(self, w, lap) -> np.ndarray:
        """[n]: P(rejoins in position p + 1 | running) for a stop at the end of `lap`."""
        return self._given_running(self.rejoin[self._lap(lap), self._w(w)])

    def expected_rejoin_position(self, w) -> np.ndarray:
        """[L]: the expected rejoin position (1-based) for a stop at the end of each lap, given running; nan where that
        never happens."""
        p = self._given_running(self.rejoin[:, self._w(w)])
        return p @ np.arange(1, len(self.drivers) + 1, dtype=np.float64)

    def places_lost_distribution(self, w, lap) -> np.ndarray:
        """[n]: P(the stop costs j places | running) for a stop at the end of `lap`; entry 0 is the free stop."""
        return self._given_running(self.lost[self._lap(lap), self._w(w)])

    def free_stop_probability(self, w) -> np.ndarray:
        """[L]: P(the stop costs no place | running) by lap; nan where the driver never runs or the lap is not recorded."""
        return self._given_running(self.lost[:, self._w(w)])[:, 0]

    def _gap_at_least(self, counts, w, seconds, lap):
        """P(gap >= seconds, or no such car | running) from gap_ahead / gap_behind: by lap [L], or for one lap."""
        j, B, n = self._edge(seconds), len(self.edges) + 1, len(self.drivers)
        c = counts[:, self._w(w)]
        running = self.rejoin[:, self._w(w), :n].sum(axis=1)
        retired = self.rejoin[:, self._w(w), n]
        hits = c[:, j:B].sum(axis=1) + (c[:, B] - retired)         # (column B: no such car, or retired)
        out = np.divide(hits, running, out=np.full(len(hits), np.nan), where=running > 0)
        return out if lap is None else float(out[self._lap(lap)])

    def clear_air_probability(self, w, seconds, lap=None):
        """P(the car ahead at rejoin is at least `seconds` up the road, or there is none | running): [L] by lap, or one
        number for `lap`.  `seconds` must be one of the edges (ValueError otherwise, as GapResult.within)."""
        return self._gap_at_least(self.gap_ahead, w, seconds, lap)

    def safe_from_behind_probability(self, w, seconds, lap=None):
        """P(the car behind at rejoin is at least `seconds` back, or there is none | running): [L] by lap, or one number
        for `lap`.  `seconds` must be one of the edges."""
        return self._gap_at_least(self.gap_behind, w, seconds, lap)

    def rejoins_behind(self, w, lap, k=5) -> list:
        """[(driver or IN_THE_LEAD, P(that is the car ahead at rejoin | running))]: the k most likely, for a stop at the
        end of `lap`; empty where the driver never runs."""
        p = self._given_running(self.ahead[self._lap(lap), self._w(w)])
        if np.isnan(p).any():
            return []
        names = list(self.drivers) + [IN_THE_LEAD]
        first = sorted(range(len(names)), key=lambda i: (-p[i], i))[:int(k)]
        return [(names[i], float(p[i])) for i in first if p[i] > 0]

    def median_rejoin_position(self, w, lap):
        """The lower median of the rejoin position (1-based) given running, for a stop at the end of `lap`; None where
        the driver never runs."""
        c = self.rejoin[self._lap(lap), self._w(w), :len(self.drivers)]
        tot = int(c.sum())
        return int(np.searchsorted(2 * np.cumsum(c), tot, side='left')) + 1 if tot else None

    def open_laps(self, w, p=0.5) -> list:
        """The laps after which P(free stop | running) >= p."""
        free = self.free_stop_probability(w)
        return [k + 1 for k in range(self.total_laps) if free[k] >= p]         # (nan >= p is False)


STINT_LETTERS = 'SMHIW'               # one letter per compound of _native.COMPOUNDS, as strategy strings spell them
MANY_STINTS = '5+ stints'              # column 0 of StintResult.seq: more stints than a sequence code holds


def encode_stints(compounds) -> int:
    """The sequence code (include/mcgp.h: mcgp_run_stints' seq_out) of a car's stints: compounds as names ('MEDIUM'),
    letters ('M'), ids (1) or one string such as 'M-H'; sum of (id + 1) 6^j over 1 .. 4 stints, 0 for more than 4."""
    if isinstance(compounds, str):
        compounds = compounds.split('-')
    ids = []
    for c in compounds:
        if isinstance(c, str):
            name = c.strip().upper()
            if name in N.COMPOUND_ID:
                c = N.COMPOUND_ID[name]
            elif len(name) == 1 and name in STINT_LETTERS:
                c = STINT_LETTERS.index(name)
            else:
                raise ValueError(f'{c!r} is not a tyre compound')
        c = int(c)
        if not 0 <= c < len(N.COMPOUNDS):
            raise ValueError(f'compound id must be in [0, {len(N.COMPOUNDS) - 1}], got {c}')
        ids.append(c)
    if not ids:
        raise ValueError('a car has at least one stint')
    if len(ids) > N.STINT_SEQ:
        return 0
    return sum((c + 1) * 6 ** j for j, c in enumerate(ids))


def decode_stints(code: int):
    """The compound ids of a sequence code, in stint order; () for code 0 (more than 4 stints); None for a code no car
    can have (a digit 0 between stints)."""
    code = int(code)
    if not 0 <= code < N.STINT_SEQ_CODES:
        raise ValueError(f'code must be in [0, {N.STINT_SEQ_CODES - 1}], got {code}')
    digits = []
    while code:
        digits.append(code % 6)
        code //= 6
    if 0 in digits:
        return None
    return tuple(x - 1 for x in digits)


def stint_string(code: int) -> str:
    """'M-H', 'S-H-S', ...; MANY_STINTS for code 0."""
    ids = decode_stints(code)
    if ids is None:
        raise ValueError(f'{code} is not the code of a stint sequence')
    return '-'.join(STINT_LETTERS[c] for c in ids) if ids else MANY_STINTS


@dataclass
class StintResult:
    """What RaceSimulator.run_stints returns: integer counts over n_simulations (include/mcgp.h: mcgp_run_stints has the
    definitions).  L = total_laps, n = len(drivers); laps first_lap .. L are recorded (2 from the grid, the state's lap +
    1 from a state).
      hist       [n][n]          [driver][position - 1], run_monte_carlo's / run_from_state's histogram
      stop_lap   [n][4][L + 1]   [driver][k][lap of the (k + 1)-th stop], column 0 = no such stop
      stops_pos  [n][5][n]       [driver][min(stops, 4)][position - 1]
      seq        [n][1296]       [driver][sequence code (encode_stints)], column 0 = more than 4 stints"""
    drivers: list
    n_simulations: int
    total_laps: int
    first_lap: int
    hist: np.ndarray
    stop_lap: np.ndarray
    stops_pos: np.ndarray
    seq: np.ndarray

    @classmethod
    def empty(cls, drivers, total_laps, n_simulations=0, first_lap=2, dtype=np.int64) -> 'StintResult':
        n, L = len(drivers), int(total_laps)
        z = lambda *shape: np.zeros(shape, dtype)
        return cls(drivers=list(drivers), n_simulations=int(n_simulations), total_laps=L, first_lap=int(first_lap),
                   hist=z(n, n), stop_lap=z(n, N.STINT_STOPS, L + 1), stops_pos=z(n, N.STINT_STOPS + 1, n),
                   seq=z(n, N.STINT_SEQ_CODES))

    def _p(self, counts):
        return np.asarray(counts, np.float64) / max(self.n_simulations, 1)

    def _d(self, driver):
        try:
            return self.drivers.index(str(driver))
        except ValueError:
            raise ValueError(f'{driver!r} is not one of the drivers') from None

    def _k(self, k):
        k = int(k)
        if not 0 <= k < N.STINT_STOPS:
            raise ValueError(f'k must be in [0, {N.STINT_STOPS - 1}] (the first {N.STINT_STOPS} stops are recorded), got {k}')
        return k

    def position_probabilities(self) -> dict:
        """{driver: {position: probability}}, what run_monte_carlo / run_from_state returns for the same arguments."""
        return histogram_to_probs(self.hist, self.drivers, self.n_simulations)

    def stop_count_probabilities(self) -> dict:
        """{driver: [P(0 stops), P(1), P(2), P(3), P(4 or more)]} over the recorded laps."""
        return {d: [float(x) for x in self._p(self.stops_pos[i].sum(axis=1))] for i, d in enumerate(self.drivers)}

    def stop_lap_distribution(self, driver, k=0) -> np.ndarray:
        """[L + 1]: P(the driver's (k + 1)-th stop is on that lap), entry 0 = P(no such stop)."""
        return self._p(self.stop_lap[self._d(driver), self._k(k)])

    def stop_window(self, driver, k=0, lo=0.1, hi=0.9):
        """(lap_lo, lap_hi): the laps at the quantiles lo and hi of the (k + 1)-th stop's lap among the simulations that
        make that stop -- the smallest lap by which at least that share of them has stopped; None if none makes it."""
        if not 0.0 <= lo <= hi <= 1.0:
            raise ValueError(f'quantiles must satisfy 0 <= lo <= hi <= 1, got {lo}, {hi}')
        c = self.stop_lap[self._d(driver), self._k(k)].astype(np.int64).copy()
        c[0] = 0
        tot = int(c.sum())
        if tot == 0:
            return None
        cum = np.cumsum(c)
        at = lambda q: int(np.searchsorted(cum, max(q * tot, 1), side='left'))
        return at(lo), at(hi)

    def strategy_probabilities(self, driver) -> list:
        """[(strategy, probability)] sorted by probability (then by text): 'M-H', 'S-H-S', ..., '5+ stints'; only the
        sequences that occur."""
        row = self.seq[self._d(driver)]
        out = [(stint_string(code), float(self._p(row[code]))) for code in np.nonzero(row)[0]]
        return sorted(out, key=lambda kv: (-kv[1], kv[0]))

    def position_probabilities_by_stops(self, driver) -> np.ndarray:
        """[5][n]: P(position p + 1 | s stops) for s = 0 .. 3 and 4 or more; a row of zeros where no simulation makes s
        stops."""
        c = self.stops_pos[self._d(driver)].astype(np.float64)
        tot = c.sum(axis=1, keepdims=True)
        return np.divide(c, tot, out=np.zeros_like(c), where=tot > 0)

    def win_probability_given_stops(self, driver, s):
        """P(win | s stops), s in 0 .. 4 (4 = 4 or more); None where no simulation makes s stops."""
        s = int(s)
        if not 0 <= s <= N.STINT_STOPS:
            raise ValueError(f's must be in [0, {N.STINT_STOPS}], got {s}')
        row = self.stops_pos[self._d(driver), s]
        tot = int(row.sum())
        return float(row[0] / tot) if tot else None


@dataclass
class MoveResult:
    """What RaceSimulator.run_moves returns: integer counts over n_simulations (include/mcgp.h: mcgp_run_moves has the
    definitions).  L = total_laps, n = len(drivers); passes are counted on laps first_lap .. L (2 from the grid, the
    state's lap + 1 from a state).  A pass is the model's order change between two lap ends, not a claim about a
    wheel-to-wheel move.
      hist         [n][n]        [driver][position - 1], run_monte_carlo's / run_from_state's histogram
      grid_fin     [n][n][n]     [driver][grid slot][position - 1]
      start_gain   [n][2n]       [driver][slot - position after lap 1 + n - 1], column 2n - 1 = retired on lap 1; zeros
                                 from a state
      passes       [n][4][128]   [driver][kind (_native.MOVE_KINDS)][min(count, 127)]
      race_passes  [1024]        [min(on-track passes of the race, 1023)]
      lap_passes   [L + 1][2]    [lap][on track, through the pits], summed over the simulations
      pair_passes  [n][n]        [a][b]: times a took a place from b on track"""
    drivers: list
    n_simulations: int
    total_laps: int
    first_lap: int
    from_grid: bool
    hist: np.ndarray
    grid_fin: np.ndarray
    start_gain: np.ndarray
    passes: np.ndarray
    race_passes: np.ndarray
    lap_passes: np.ndarray
    pair_passes: np.ndarray

    @classmethod
    def empty(cls, drivers, total_laps, n_simulations=0, first_lap=2, from_grid=True, dtype=np.int64) -> 'MoveResult':
        n, L = len(drivers), int(total_laps)
        z = lambda *shape: np.zeros(shape, dtype)
        return cls(drivers=list(drivers), n_simulations=int(n_simulations), total_laps=L, first_lap=int(first_lap),
                   from_grid=bool(from_grid), hist=z(n, n), grid_fin=z(n, n, n), start_gain=z(n, 2 * n),
                   passes=z(n, len(N.MOVE_KINDS), N.MOVE_DRIVER_CAP + 1), race_passes=z(N.MOVE_RACE_CAP + 1),
                   lap_passes=z(L + 1, 2), pair_passes=z(n, n))

    def _p(self, counts):
        return np.asarray(counts, np.float64) / max(self.n_simulations, 1)

    def _d(self, driver):
        try:
            return self.drivers.index(str(driver))
        except ValueError:
            raise ValueError(f'{driver!r} is not one of the drivers') from None

    def _slot(self, slot):
        slot = int(slot)
        if not 1 <= slot <= len(self.drivers):
            raise ValueError(f'slot must be in [1, {len(self.drivers)}] (1 = pole), got {slot}')
        return slot - 1

    def _kind(self, kind):
        if isinstance(kind, str):
            if kind not in N.MOVE_KINDS:
                raise ValueError(f'kind must be one of {N.MOVE_KINDS}, got {kind!r}')
            return N.MOVE_KINDS.index(kind)
        kind = int(kind)
        if not 0 <= kind < len(N.MOVE_KINDS):
            raise ValueError(f'kind must be in [0, {len(N.MOVE_KINDS) - 1}], got {kind}')
        return kind

    def _needs_grid(self):
        if not self.from_grid:
            raise ValueError('a run from a race state has no start: start gains are counted from the grid only')

    def position_probabilities(self) -> dict:
        """{driver: {position: probability}}, what run_monte_carlo / run_from_state returns for the same arguments."""
        return histogram_to_probs(self.hist, self.drivers, self.n_simulations)

    def finish_given_grid(self, driver, slot):
        """[n]: P(position p + 1 | the driver starts from `slot`, 1 = pole); None where no simulation starts it there."""
        row = self.grid_fin[self._d(driver), self._slot(slot)].astype(np.float64)
        tot = row.sum()
        return row / tot if tot else None

    def win_probability_from(self, driver, slot):
        """P(win | the driver starts from `slot`, 1 = pole); None where no simulation starts it there."""
        p = self.finish_given_grid(driver, slot)
        return float(p[0]) if p is not None else None

    def positions_gained_distribution(self, driver) -> np.ndarray:
        """[2n - 1]: P(grid slot - classified position = g) at index g + n - 1, g in -(n - 1) .. n - 1 (from grid_fin;
        retirements count with their classified position)."""
        n = len(self.drivers)
        gf = self.grid_fin[self._d(driver)]
        out = np.zeros(2 * n - 1, np.float64)
        for g in range(-(n - 1), n):
            out[g + n - 1] = np.trace(gf, offset=-g)               # cells [slot][slot - g]
        return self._p(out)

    def expected_positions_gained(self) -> dict:
        """{driver: E[grid slot - classified position]}."""
        n = len(self.drivers)
        g = np.arange(-(n - 1), n)
        return {d: float((self.positions_gained_distribution(d) * g).sum()) for d in self.drivers}

    def start_gain_distribution(self, driver) -> np.ndarray:
        """[2n]: P(grid slot - position after lap 1 = g) at index g + n - 1; the last entry = P(retired on lap 1)."""
        self._needs_grid()
        return self._p(self.start_gain[self._d(driver)])

    def expected_start_gain(self) -> dict:
        """{driver: E[grid slot - position after lap 1 | running after lap 1]}; None for a driver that never is."""
        self._needs_grid()
        n = len(self.drivers)
        g = np.arange(-(n - 1), n)
        out = {}
        for i, d in enumerate(self.drivers):
            row = self.start_gain[i, :2 * n - 1].astype(np.float64)
            out[d] = float((row * g).sum() / row.sum()) if row.sum() else None
        return out

    def passes_distribution(self, driver, kind=0) -> np.ndarray:
        """[128]: P(the driver's passes of that kind in a race = c) at index c; the last entry = 127 or more.  kind: 0 ..
        3 or a name of _native.MOVE_KINDS."""
        return self._p(self.passes[self._d(driver), self._kind(kind)])

    def expected_passes(self) -> dict:
        """{driver: {kind name: expected passes per race}} (a count of 127 or more counts as 127)."""
        c = np.arange(self.passes.shape[2])
        return {d: {k: float((self._p(self.passes[i, j]) * c).sum()) for j, k in enumerate(N.MOVE_KINDS)}
                for i, d in enumerate(self.drivers)}

    def race_passes_distribution(self) -> np.ndarray:
        """[1024]: P(on-track passes of the race = c) at index c; the last entry = 1023 or more."""
        return self._p(self.race_passes)

    def race_passes_quantile(self, q) -> int:
        """The smallest count c with P(on-track passes of the race <= c) >= q."""
        if not 0.0 <= q <= 1.0:
            raise ValueError(f'q must be in [0, 1], got {q}')
        tot = int(self.race_passes.sum())
        if tot == 0:
            return 0
        return int(np.searchsorted(np.cumsum(self.race_passes), max(q * tot, 1), side='left'))

    def expected_race_passes(self) -> float:
        """Expected on-track passes per race, from the uncapped per-lap sums."""
        return float(self.lap_passes[:, 0].sum() / max(self.n_simulations, 1))

    def passes_by_lap(self) -> np.ndarray:
        """[L + 1][2]: expected passes on that lap, on track and through the pits (rows 0 and 1 are 0)."""
        return self._p(self.lap_passes)

    def most_frequent_passes(self, k=10) -> list:
        """[(a, b, expected times per race a takes a place from b on track)], the k commonest pairs, by count then name."""
        n = len(self.drivers)
        cells = [(int(self.pair_passes[a, b]), self.drivers[a], self.drivers[b]) for a in range(n) for b in range(n)
                 if self.pair_passes[a, b]]
        cells.sort(key=lambda c: (-c[0], c[1], c[2]))
        return [(a, b, float(self._p(c))) for c, a, b in cells[:int(k)]]


DEFAULT_POINTS = (25, 18, 15, 12, 10, 8, 6, 4, 2, 1)      # a Grand Prix, positions 1-10
MAX_RACES = 64                                             # include/mcgp.h: mcgp_run_championship limits
MAX_TOTAL_POINTS = 65535
MAX_POSITION_COUNT = 31
DEFAULT_FASTEST_LAP_WITHIN = 10                            # the 2019-2024 rule: classified in the top ten


@dataclass
class ChampionshipResult:
    """What run_championship returns.  Integer histograms (counts over n_simulations):
    champ_hist [n][n] = [driver][championship position - 1], team_hist [T][T] the same for the constructors,
    gain_hist [n][G + 1] = [driver][points gained in these races]; race_histograms (when asked for) = one [n][n]
    position histogram per race, what run_monte_carlo gives that race alone.  Probabilities derive from them.

    With by_round=True (None otherwise), the standings after every race r of the call (include/mcgp.h:
    mcgp_run_championship_rounds): round_hist [R][n][n] = [race][driver][standings position], contend [R][n] and
    secure [R][n] = simulations in which the driver is in contention / has the title secure after race r, and
    team_round_hist [R][T][T], team_contend [R][T], team_secure [R][T] for the constructors.

    When some race has a fastest-lap bonus (the races' `fastest_lap_points`; None otherwise, include/mcgp.h:
    mcgp_run_championship_bonus): fastest_lap_counts [R][n] = simulations in which the driver set race r's fastest lap,
    bonus_counts [R][n] = those in which the driver also took the bonus (rows of races without a bonus are zero), and
    bonus_points [R] the bonus of each race.

    With given_race (None otherwise, include/mcgp.h: mcgp_run_championship_live): title_given [n][n][n] = simulations in
    which [driver] is classified [position - 1] in race given_race and [champion] takes the title; summed over the
    champion it is that race's position histogram, summed over the driver it is champ_hist[champion][0] for every
    position."""
    drivers: list
    teams: list
    n_simulations: int
    champ_hist: np.ndarray
    team_hist: np.ndarray
    gain_hist: np.ndarray
    initial_points: dict
    race_histograms: list | None = None
    round_hist: np.ndarray | None = None
    contend: np.ndarray | None = None
    secure: np.ndarray | None = None
    team_round_hist: np.ndarray | None = None
    team_contend: np.ndarray | None = None
    team_secure: np.ndarray | None = None
    fastest_lap_counts: np.ndarray | None = None
    bonus_counts: np.ndarray | None = None
    bonus_points: list | None = None
    team_index: list | None = None           # [n] index into `teams` of each driver
    title_given: np.ndarray | None = None    # [n][n][n] = [driver][position - 1 in race given_race][champion], or None
    given_race: int | None = None            # index into the call's races

    @property
    def title_probabilities(self) -> dict:
        return {d: int(self.champ_hist[i, 0]) / self.n_simulations for i, d in enumerate(self.drivers)}

    @property
    def position_probabilities(self) -> dict:
        return histogram_to_probs(self.champ_hist, self.drivers, self.n_simulations)

    @property
    def expected_points(self) -> dict:
        """Standings carried in plus the mean points gained."""
        g = np.arange(self.gain_hist.shape[1], dtype=np.float64)
        return {d: self.initial_points.get(d, 0) + float(self.gain_hist[i] @ g) / self.n_simulations
                for i, d in enumerate(self.drivers)}

    @property
    def constructor_title_probabilities(self) -> dict:
        return {t: int(self.team_hist[i, 0]) / self.n_simulations for i, t in enumerate(self.teams)}

    @property
    def constructor_position_probabilities(self) -> dict:
        return histogram_to_probs(self.team_hist, self.teams, self.n_simulations)

    # ---- by round (run_championship(..., by_round=True)): one entry per race of the call, in race order
    def _by_round(self, counts, names, what):
        if counts is None:
            raise ValueError(f'{what} needs run_championship(..., by_round=True)')
        return [{e: int(row[i]) / self.n_simulations for i, e in enumerate(names)} for row in counts]

    def _decided(self, secure, what):
        if secure is None:
            raise ValueError(f'{what} needs run_championship(..., by_round=True)')
        return [int(row.sum()) / self.n_simulations for row in secure]

    def _clinch(self, secure, names, what):
        if secure is None:
            raise ValueError(f'{what} needs run_championship(..., by_round=True)')
        # once secure, always secure: the simulations that clinch AT race r are the growth of the row
        first = np.diff(np.asarray(secure, np.int64), axis=0, prepend=0)
        return {e: {int(r): int(first[r, i]) / self.n_simulations for r in np.nonzero(first[:, i])[0]}
                for i, e in enumerate(names)}

    @property
    def leader_probabilities_by_round(self) -> list:
        """[race] {driver: P(leads the standings after that race)}."""
        return self._by_round(None if self.round_hist is None else self.round_hist[:, :, 0], self.drivers,
                              'leader_probabilities_by_round')

    @property
    def contention_probabilities_by_round(self) -> list:
        """[race] {driver: P(still in contention after that race)}: leading, or within the points a driver can still
        take."""
        return self._by_round(self.contend, self.drivers, 'contention_probabilities_by_round')

    @property
    def decided_by_round(self) -> list:
        """[race] P(some driver's title is secure after that race); non-decreasing, 1 after the last race."""
        return self._decided(self.secure, 'decided_by_round')

    @property
    def clinch_round_probabilities(self) -> dict:
        """{driver: {race index: P(the driver's title becomes secure at that race)}}, zero entries omitted; a driver's
        entries sum to its title probability.  Index 0 includes titles already secure before the first race."""
        return self._clinch(self.secure, self.drivers, 'clinch_round_probabilities')

    @property
    def constructor_leader_probabilities_by_round(self) -> list:
        return self._by_round(None if self.team_round_hist is None else self.team_round_hist[:, :, 0], self.teams,
                              'constructor_leader_probabilities_by_round')

    @property
    def constructor_contention_probabilities_by_round(self) -> list:
        return self._by_round(self.team_contend, self.teams, 'constructor_contention_probabilities_by_round')

    @property
    def constructor_decided_by_round(self) -> list:
        return self._decided(self.team_secure, 'constructor_decided_by_round')

    @property
    def constructor_clinch_round_probabilities(self) -> dict:
        return self._clinch(self.team_secure, self.teams, 'constructor_clinch_round_probabilities')

    # ---- fastest-lap bonus (races with `fastest_lap_points`)
    def _bonus(self, what):
        if self.bonus_counts is None:
            raise ValueError(f'{what} needs a race with fastest_lap_points')
        return np.asarray(self.bonus_counts, np.int64)

    @property
    def bonus_probabilities_by_round(self) -> list:
        """[race] {driver: P(takes that race's fastest-lap bonus)}; all zero for a race without a bonus."""
        counts = self._bonus('bonus_probabilities_by_round')
        return [{d: int(row[i]) / self.n_simulations for i, d in enumerate(self.drivers)} for row in counts]

    @property
    def expected_bonus_points(self) -> dict:
        """{driver: mean bonus points over these races} (part of expected_points)."""
        counts = self._bonus('expected_bonus_points')
        e = np.asarray(self.bonus_points, np.int64) @ counts
        return {d: int(e[i]) / self.n_simulations for i, d in enumerate(self.drivers)}

    @property
    def expected_constructor_bonus_points(self) -> dict:
        """{team: mean bonus points of its drivers over these races}."""
        per_driver = self.expected_bonus_points
        out = {t: 0.0 for t in self.teams}
        for i, d in enumerate(self.drivers):
            out[self.teams[self.team_index[i]]] += per_driver[d]
        return out


    # ---- title odds by finishing position (run_championship(..., given_race=k))
    def _given(self, what):
        if self.title_given is None:
            raise ValueError(f'{what}: not counted (it needs run_championship(..., given_race=...))')
        return np.asarray(self.title_given, np.int64)

    def _driver_index(self, driver):
        if str(driver) not in self.drivers:
            raise KeyError(f'no driver {driver!r}')
        return self.drivers.index(str(driver))

    def title_probability_given(self, driver, position, champion=None):
        """P(`champion` takes the title | `driver` is classified `position` (1-based) in the given race); `champion`
        defaults to `driver`.  None when no simulation has that finish."""
        table = self._given('title_probability_given')
        d, e = self._driver_index(driver), self._driver_index(driver if champion is None else champion)
        position = int(position)
        if not 1 <= position <= len(self.drivers):
            raise ValueError(f'position must be in [1, {len(self.drivers)}], got {position}')
        finishes = int(table[d, position - 1].sum())
        return int(table[d, position - 1, e]) / finishes if finishes else None

    def title_needs(self, driver) -> dict:
        """{position: P(`driver` takes the title | `driver` is classified there in the given race)} for the positions
        that occurred."""
        table = self._given('title_needs')
        d = self._driver_index(driver)
        return {int(p) + 1: int(table[d, p, d]) / int(table[d, p].sum()) for p in np.nonzero(table[d].sum(axis=1))[0]}


def _standings_arrays(standings, drivers):
    """{driver: points} or {driver: {'points': p, 'finishes': [count of P1, P2, ...]}} -> (points [n], counts [n][n])."""
    n = len(drivers)
    pts = np.zeros(n, np.int64)
    counts = np.zeros((n, n), np.int64)
    index = {d: i for i, d in enumerate(drivers)}
    for d, v in (standings or {}).items():
        if str(d) not in index:
            raise ValueError(f'standings name {d!r}, who is not in the field')
        i = index[str(d)]
        if isinstance(v, dict):
            pts[i] = int(v.get('points', 0))
            fin = [int(x) for x in v.get('finishes', [])]
            if len(fin) > n:
                fin, extra = fin[:n], fin[n:]
                if any(extra):
                    raise ValueError(f'{d}: finishes list has counts past position {n}')
            counts[i, :len(fin)] = fin
        else:
            pts[i] = int(v)
    if (pts < 0).any() or (counts < 0).any():
        raise ValueError('standings must not be negative')
    return pts, counts


def run_championship(races, n_simulations, *, standings=None, seed=None, sim_offset=0, device=0, set_pop=None,
                     return_race_histograms=False, by_round=False, drivers=None, given_race=None) -> ChampionshipResult:
    """Drivers' and constructors' championship over a calendar of races (include/mcgp.h: mcgp_run_championship).

    `races`: a list of dicts with the keys run_monte_carlo_batch takes (`config`, `grid_probs`, `base_pace`,
    `tire_deg`, `driver_variance`, optional `driver_dnf_rates`, `seed`, `track_condition`, `deviates`), plus `points`
    (the table of positions 1, 2, ...; default 25-18-15-12-10-8-6-4-2-1), `countback` (default True; False for a
    sprint, whose results score but do not break ties), `fastest_lap_points` (default 0: the bonus for the driver who
    sets the race's fastest lap) and `fastest_lap_within` (default 10, at most the field size: the classified positions
    that take it).  A race with a bonus runs on the lap-time-tracking kernel, several times the cost of one without
    (include/mcgp.h: mcgp_run_championship_bonus); with no bonus anywhere the call is what it was.  Simulation s of the season is the tuple of what
    run_monte_carlo gives each race alone for simulation id s under that race's seed.

    The driver order is the first race's grid_probs key order; every race must have the same driver set.  Teams come
    from the first race's config.driver_teams ('Unknown' for a driver it does not list), in order of first appearance.
    `standings`: points before these races, {driver: points} or {driver: {'points': p, 'finishes': [P1s, P2s, ...]}}.
    A race without `seed` gets random.Random(seed).getrandbits(63), in race order.  `device`: an index, a list of
    indices or 'all' (simulation ids sharded over the devices, one host thread each).

    Points follow the race model's classification: retired cars are classified behind the finishers (as in the
    reference), so a retired car scores when fewer cars finish than the table pays.  Ties: more points, then more
    wins, more seconds, ... (countback races only); a full tie goes to the lower driver (team) index -- the
    regulations then use criteria this model does not have.

    `by_round=True` also counts, on the device, the standings after every race of the call (include/mcgp.h:
    mcgp_run_championship_rounds): who leads, who is still in contention and whose title is secure after each race,
    for drivers and constructors (ChampionshipResult.round_hist and the fields and properties next to it).  The other
    results are the same either way.

    Live title odds (include/mcgp.h: mcgp_run_championship_live).  races[0] may carry `state`, a RaceState, instead of
    `grid_probs`: that race is then RaceSimulator.run_from_state's from the state (32-bit deviates, no fastest-lap bonus),
    simulation i of the season taking the finishing order that call gives id sim_offset + i.  The driver order is then
    `drivers` if given, else the state's grid order (run_from_state's rule); the later races' grid_probs must have the
    same driver set.  `standings` are those before race 0: nothing is inferred from the state.  `given_race=k` also counts
    ChampionshipResult.title_given, the title odds by finishing position in races[k] (title_probability_given,
    title_needs).  Without a state and given_race the call goes where it always went."""
    races = list(races)
    if not races:
        raise ValueError('a championship needs at least one race')
    if len(races) > MAX_RACES:
        raise ValueError(f'at most {MAX_RACES} races per call, got {len(races)}')
    set_pop = dict(set_pop or DEFAULT_SET_POP)
    state = races[0].get('state')
    if state is not None and races[0].get('grid_probs') is not None:
        raise ValueError('race 0: give either state or grid_probs, not both')
    for r, race in enumerate(races[1:], 1):
        if race.get('state') is not None:
            raise ValueError(f'race {r}: only the first race of the call can start from a state')
    if drivers is not None:
        drivers = [str(d) for d in drivers]
    elif state is not None:
        drivers = [str(c.driver) for c in state.cars]
    else:
        drivers = [str(d) for d in races[0]['grid_probs'].keys()]
    n = len(drivers)
    if given_race is not None:
        given_race = int(given_race)
        if not 0 <= given_race < len(races):
            raise ValueError(f'given_race must be an index into races, in [0, {len(races) - 1}], got {given_race}')
    if not (1 <= n <= N.MAX_CARS):
        raise ValueError(f'number of drivers must be in [1, {N.MAX_CARS}], got {n}')
    rng = random.Random(seed)
    probs, grids, seeds, deviates = [], [], [], []
    points = np.zeros((len(races), n), np.int32)
    countback = np.zeros(len(races), np.uint8)
    bonus_pts = np.zeros(len(races), np.int32)
    bonus_within = np.ones(len(races), np.int32)
    for r, race in enumerate(races):
        live_race = r == 0 and state is not None
        if not live_race:
            gp = {str(k): v for k, v in race['grid_probs'].items()}
            if set(gp) != set(drivers) or len(gp) != n:
                raise ValueError(f'race {r}: its drivers differ from the first race\'s')
        elif int(race.get('deviates', 32)) != 32:
            raise ValueError('race 0: a race from a state runs with deviates=32 only')
        elif int(race.get('fastest_lap_points', 0)) > 0:
            raise ValueError('race 0: a race from a state has no fastest-lap bonus (the laps before the state are unknown)')
        probs.append(_Problem(race['config'], drivers, race['base_pace'], race['tire_deg'], race['driver_variance'],
                              race.get('driver_dnf_rates'), race.get('track_condition', 'dry'), set_pop,
                              race.get('deviates', 32)))
        grids.append(None if live_race else RaceSimulator._grid_matrix(gp, drivers))
        race_seed = race.get('seed')
        seeds.append(RaceSimulator._resolve_seed(rng.getrandbits(63) if race_seed is None else race_seed))
        table = [int(x) for x in race.get('points', DEFAULT_POINTS)]
        if any(x < 0 for x in table):
            raise ValueError(f'race {r}: points must not be negative')
        points[r, :min(n, len(table))] = table[:n]           # positions past the table score 0
        countback[r] = 1 if race.get('countback', True) else 0
        fl = int(race.get('fastest_lap_points', 0))
        within = int(race.get('fastest_lap_within', DEFAULT_FASTEST_LAP_WITHIN))
        if fl < 0 or fl > MAX_TOTAL_POINTS:
            raise ValueError(f'race {r}: fastest_lap_points must be in [0, {MAX_TOTAL_POINTS}], got {fl}')
        if fl > 0 and within < 1:
            raise ValueError(f'race {r}: fastest_lap_within must be at least 1, got {within}')
        bonus_pts[r] = fl
        bonus_within[r] = max(1, min(within, n))
    teams_of = races[0]['config'].driver_teams
    team_names = []
    for d in drivers:
        t = str(teams_of.get(d, 'Unknown'))
        if t not in team_names:
            team_names.append(t)
    team = np.array([team_names.index(str(teams_of.get(d, 'Unknown'))) for d in drivers], np.int32)
    init_pts, init_counts = _standings_arrays(standings, drivers)
    # the limits of the device's standing keys (the library rejects the same calls with MCGP_E_BAD_ARG)
    with_bonus = bool((bonus_pts > 0).any())
    G = int(points.max(axis=1).sum()) + int(bonus_pts.sum())
    if int(init_pts.max()) + G > MAX_TOTAL_POINTS:
        raise ValueError(f'a driver could reach {int(init_pts.max()) + G} points: the limit is {MAX_TOTAL_POINTS}')
    worst = int(init_counts.max()) + int(countback.sum())
    if worst > MAX_POSITION_COUNT:
        raise ValueError(f'a driver could have {worst} finishes in one position (standings plus countback races): '
                         f'the limit is {MAX_POSITION_COUNT}')
    init_pts32 = np.ascontiguousarray(init_pts, np.int32)
    init_counts32 = np.ascontiguousarray(init_counts, np.int32)
    T = len(team_names)
    R = len(races)
    n_simulations = int(n_simulations)
    if n_simulations < 0:
        raise ValueError('n_simulations must be >= 0')
    devices = RaceSimulator(races[0]['config'], device=device).devices
    lib = N.lib()
    if by_round and not hasattr(lib, 'mcgp_run_championship_rounds'):
        raise N.McgpError(-1, 'the loaded library does not export mcgp_run_championship_rounds: by_round=True needs a '
                              'library built from sources that have it')
    if with_bonus and not hasattr(lib, 'mcgp_run_championship_bonus'):
        raise N.McgpError(-1, 'the loaded library does not export mcgp_run_championship_bonus: fastest_lap_points needs '
                              'a library built from sources that have it')
    live = state is not None or given_race is not None
    if live and not hasattr(lib, 'mcgp_run_championship_live'):
        raise N.McgpError(-1, 'the loaded library does not export mcgp_run_championship_live: a state or given_race needs '
                              'a library built from sources that have it')
    state_arrays = state.arrays(drivers, races[0]['config'].total_laps) if state is not None else None
    c_state = state.c_struct(state_arrays) if state is not None else None
    cfgs = (N.McgpConfig * R)(*[p.cfg for p in probs])
    drvs = (N.McgpDrivers * R)(*[p.drv for p in probs])
    gptrs = (C.POINTER(C.c_double) * R)(*[C.POINTER(C.c_double)() if g is None else _dptr(g) for g in grids])
    seeds_c = (C.c_uint64 * R)(*seeds)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))

    def run_shard(dev, offset, count):
        ch = np.zeros((n, n), np.uint64)
        th = np.zeros((T, T), np.uint64)
        gh = np.zeros((n, G + 1), np.uint64)
        rh = np.zeros((R, n, n), np.uint64) if return_race_histograms else None
        args = (R, cfgs, drvs, gptrs, n, int(count), int(sim_offset) + int(offset), seeds_c, i32(points),
                countback.ctypes.data_as(C.POINTER(C.c_uint8)), i32(init_pts32), i32(init_counts32), i32(team), T, int(dev),
                u64(ch), u64(th), u64(gh), u64(rh) if rh is not None else None)
        rounds = bonus = given = ()
        if by_round:
            rounds = tuple(np.zeros(shape, np.uint64) for shape in ((R, n, n), (R, n), (R, n), (R, T, T), (R, T), (R, T)))
        if with_bonus:
            bonus = (np.zeros((R, n), np.uint64), np.zeros((R, n), np.uint64))          # bonus_hist, fastest_hist
        if given_race is not None:
            given = (np.zeros((n, n, n), np.uint64),)
        if live:
            rc = lib.mcgp_run_championship_live(
                *args, *([u64(a) for a in rounds] if by_round else [None] * 6),
                *([i32(bonus_pts), i32(bonus_within)] + [u64(a) for a in bonus] if with_bonus else [None] * 4),
                C.byref(c_state) if c_state is not None else None, -1 if given_race is None else given_race,
                u64(given[0]) if given else None)
        elif with_bonus:
            rc = lib.mcgp_run_championship_bonus(*args, *([u64(a) for a in rounds] if by_round else [None] * 6),
                                                 i32(bonus_pts), i32(bonus_within), *[u64(a) for a in bonus])
        elif by_round:
            rc = lib.mcgp_run_championship_rounds(*args, *[u64(a) for a in rounds])
        else:
            rc = lib.mcgp_run_championship(*args)
        return (ch, th, gh, rh) + rounds + bonus + given, rc, (lib.mcgp_last_error().decode('utf-8', 'replace') if rc != 0 else '')

    if len(devices) == 1:
        parts = [run_shard(devices[0], 0, n_simulations)]
    else:
        from concurrent.futures import ThreadPoolExecutor
        from .distributed import shard_range
        world = len(devices)
        shards = [shard_range(n_simulations, k, world) for k in range(world)]
        with ThreadPoolExecutor(world) as ex:
            parts = list(ex.map(lambda a: run_shard(a[0], *a[1]), zip(devices, shards)))
    for _, rc, msg in parts:
        if rc != 0:
            raise N.McgpError(rc, msg)
    total = lambda k: np.sum([p[0][k] for p in parts], axis=0, dtype=np.uint64).astype(np.int64)
    at_bonus = 4 + (6 if by_round else 0)            # the shard tuple: four season arrays, rounds, bonus, title_given
    return ChampionshipResult(
        drivers=drivers, teams=team_names, n_simulations=n_simulations, champ_hist=total(0), team_hist=total(1),
        gain_hist=total(2), initial_points={d: int(init_pts[i]) for i, d in enumerate(drivers)},
        race_histograms=list(total(3)) if return_race_histograms else None,
        **({k: total(4 + i) for i, k in enumerate(('round_hist', 'contend', 'secure', 'team_round_hist', 'team_contend',
                                                   'team_secure'))} if by_round else {}),
        team_index=[int(t) for t in team],
        **(dict(bonus_counts=total(at_bonus), fastest_lap_counts=total(at_bonus + 1), bonus_points=[int(b) for b in bonus_pts])
           if with_bonus else {}),
        **(dict(title_given=total(at_bonus + (2 if with_bonus else 0)), given_race=given_race)
           if given_race is not None else {}))


def histogram_to_probs(hist, drivers, n_simulations):
    """counts[driver][position-1] -> {driver: {position: count / n}} with zero cells omitted (:97-100)."""
    out = {}
    for i, d in enumerate(drivers):
        row = hist[i]
        nz = np.nonzero(row)[0]
        out[d] = {int(p) + 1: int(row[p]) / n_simulations for p in nz}
    return out


# ---------------------------------------------------------------------------------------------- pit-strategy comparison
DRY_COMPOUNDS = ('SOFT', 'MEDIUM', 'HARD')


@dataclass
class PitPlan:
    """One driver's strategy in a scenario of RaceSimulator.run_strategies: `stops` = [(lap, compound name), ...] with
    strictly increasing laps (2 .. total_laps from the grid, after the state's lap from a RaceState), at most 8; `start`
    = the starting compound name, or None for the model's start (SOFT at age 4 on the first ten grid slots, MEDIUM new
    behind them, INTERMEDIATE / WET on a damp / wet track), with `start_age` laps on it.  A planned driver never takes
    the model's own pit rule: it stops on its plan's laps and nowhere else."""
    driver: str
    stops: list = field(default_factory=list)
    start: str | None = None
    start_age: int = 0

    def c_struct(self, index, from_state=False) -> N.McgpPitPlan:
        """mcgp_pit_plan with the driver index from `index`; ValueError on an unknown compound or too many stops (the
        library checks the laps and the rest)."""
        stops = [(int(lap), str(comp)) for lap, comp in self.stops]
        if len(stops) > N.MAX_PLAN_STOPS:
            raise ValueError(f'{self.driver}: at most {N.MAX_PLAN_STOPS} stops, got {len(stops)}')
        for _, comp in stops:
            if comp not in N.COMPOUND_ID:
                raise ValueError(f'{self.driver}: compound must be one of {list(N.COMPOUNDS)}, got {comp!r}')
        if self.start is not None and self.start not in N.COMPOUND_ID:
            raise ValueError(f'{self.driver}: start must be None or one of {list(N.COMPOUNDS)}, got {self.start!r}')
        if from_state and (self.start is not None or int(self.start_age) != 0):
            raise ValueError(f'{self.driver}: a plan from a race state has no start compound or age (the state fixes '
                             'the tyres)')
        p = N.McgpPitPlan()
        p.driver = int(index[str(self.driver)])
        p.start_compound = -1 if self.start is None else N.COMPOUND_ID[self.start]
        p.start_age = int(self.start_age)
        p.n_stops = len(stops)
        for k, (lap, comp) in enumerate(stops):
            p.stop_lap[k] = lap
            p.stop_compound[k] = N.COMPOUND_ID[comp]
        return p


def check_two_compounds(plan: PitPlan, used=None, scenario=''):
    """The two-compound rule of a dry race, for a plan: ValueError unless the car is sure to run two dry compounds.
    `used`: the compounds a race state says the car has used (None: a run from the grid, where a plan without `start`
    must work for both of the model's starts, SOFT and MEDIUM)."""
    stops = {str(c) for _, c in plan.stops} & set(DRY_COMPOUNDS)
    if used is not None:
        starts = [set(used)]
    elif plan.start is not None:
        starts = [{plan.start}]
    else:
        starts = [{'SOFT'}, {'MEDIUM'}]
    for st in starts:
        if len((st & set(DRY_COMPOUNDS)) | stops) < 2:
            where = f'scenario {scenario!r}: ' if scenario else ''
            raise ValueError(f'{where}{plan.driver}: the plan runs one dry compound ({sorted(st | stops)}) on a dry '
                             'track; pass allow_single_compound=True to run it anyway')


def pit_window(driver: str, laps, compound: str, then=(), start=None, start_age=0) -> dict:
    """The optimal-pit-window sweep: one single-stop scenario per lap of `laps`, {"<driver> L<lap>": [PitPlan]}, the
    stop onto `compound`, followed by the stops of `then` ([(lap, compound)], laps after the window)."""
    return {f'{driver} L{int(lap)}': [PitPlan(driver, [(int(lap), compound)] + [(int(a), str(c)) for a, c in then],
                                              start=start, start_age=start_age)]
            for lap in laps}


@dataclass
class StrategyResult:
    """What RaceSimulator.run_strategies returns: integer counts per scenario (in `names` order) over n_simulations:
      hist    [S][n][n]       [scenario][driver][position - 1]
      delta   [S][n][2n - 1]  [scenario][driver][(pos_s - pos_0) + n - 1]: the paired change of the driver's position
                              against the first scenario in the same simulation
      orders  [S][N][n]       finishing orders (return_orders=True), else None"""
    names: list
    drivers: list
    n_simulations: int
    hist: np.ndarray
    delta: np.ndarray
    orders: np.ndarray | None = None

    def _s(self, name):
        if name is None:
            return 0
        if name not in self.names:
            raise KeyError(f'no scenario {name!r}; scenarios: {self.names}')
        return self.names.index(name)

    def _d(self, driver):
        if driver not in self.drivers:
            raise KeyError(f'no driver {driver!r}')
        return self.drivers.index(driver)

    def position_probabilities(self, name=None) -> dict:
        """{driver: {position: probability}} of scenario `name` (None: {name: that dict} for every scenario)."""
        if name is None:
            return {s: self.position_probabilities(s) for s in self.names}
        return histogram_to_probs(self.hist[self._s(name)], self.drivers, max(self.n_simulations, 1))

    def _p(self, name):
        return np.asarray(self.hist[self._s(name)], np.float64) / max(self.n_simulations, 1)

    def expected_position(self, name) -> dict:
        p = self._p(name)
        pos = np.arange(1, len(self.drivers) + 1, dtype=np.float64)
        return {d: float(p[i] @ pos) for i, d in enumerate(self.drivers)}

    def expected_points(self, name, points=DEFAULT_POINTS) -> dict:
        p = self._p(name)
        n = len(self.drivers)
        table = np.zeros(n, np.float64)
        m = min(n, len(points))
        table[:m] = np.asarray(points[:m], np.float64)
        return {d: float(p[i] @ table) for i, d in enumerate(self.drivers)}

    def win_probability(self, name, driver) -> float:
        return float(self._p(name)[self._d(driver), 0])

    def podium_probability(self, name, driver) -> float:
        return float(self._p(name)[self._d(driver), :3].sum())

    def compare(self, name, driver, against=None) -> dict:
        """Scenario `name` against `against` (default: the first scenario) for `driver`, paired by simulation:
        p_better / p_same / p_worse (finishing ahead of, level with, behind its own result under `against`), mean_gain
        (positions gained, mean) and its paired standard error `se`; `se_unpaired` is the standard error the two
        marginal histograms alone would give (independent runs).  Against the first scenario this reads `delta`; against
        another one it needs the finishing orders (return_orders=True)."""
        s, a, i = self._s(name), self._s(against if against is not None else self.names[0]), self._d(driver)
        n, N_ = len(self.drivers), self.n_simulations
        if a == 0:
            counts = np.asarray(self.delta[s, i], np.float64)
            change = np.arange(-(n - 1), n, dtype=np.float64)            # pos_s - pos_against
        else:
            if self.orders is None:
                raise ValueError('compare against a scenario other than the first needs return_orders=True')
            pos = lambda k: np.argmax(self.orders[k] == i, axis=1)
            diff = pos(s) - pos(a)
            counts = np.bincount(diff + n - 1, minlength=2 * n - 1).astype(np.float64)
            change = np.arange(-(n - 1), n, dtype=np.float64)
        tot = max(counts.sum(), 1.0)
        gain = -change
        mean = float(counts @ gain) / tot
        var = float(counts @ (gain - mean) ** 2) / max(tot - 1.0, 1.0)
        pos = np.arange(1, n + 1, dtype=np.float64)
        var_pos = lambda k: float(self.hist[k, i] @ (pos - float(self.hist[k, i] @ pos) / tot) ** 2) / max(tot - 1.0, 1.0)
        return dict(p_better=float(counts[:n - 1].sum()) / tot, p_same=float(counts[n - 1]) / tot,
                    p_worse=float(counts[n:].sum()) / tot, mean_gain=mean, se=math.sqrt(var / tot),
                    se_unpaired=math.sqrt((var_pos(s) + var_pos(a)) / tot), n_simulations=int(N_))

    def best(self, driver, by='expected_points'):
        """The scenario name that is best for `driver` by 'expected_points', 'expected_position' (lowest), 'win' or
        'podium'."""
        if by == 'expected_points':
            key = lambda s: self.expected_points(s)[driver]
        elif by == 'expected_position':
            key = lambda s: -self.expected_position(s)[driver]
        elif by == 'win':
            key = lambda s: self.win_probability(s, driver)
        elif by == 'podium':
            key = lambda s: self.podium_probability(s, driver)
        else:
            raise ValueError(f"by must be 'expected_points', 'expected_position', 'win' or 'podium', got {by!r}")
        self._d(driver)
        return max(self.names, key=key)


# ---------------------------------------------------------------------------------------------- time penalties
@dataclass
class TimePenalty:
    """One time penalty in a scenario of RaceSimulator.run_penalties: `seconds` (in (0, 1e6]) added to `driver`'s race.
    kind 'serve': a 5 s / 10 s penalty pending from lap `lap` (None: the first lap that has a pit step), served at the
    car's first pit stop from that lap on, else added at the flag; 'flag': a post-race penalty, added at the flag (`lap`
    must be None); 'lap': time lost on lap `lap` (a drive-through, a stop-go: give the loss), after any pit stop of
    that lap.  A car that retires first takes nothing."""
    driver: str
    seconds: float
    kind: str = 'serve'
    lap: int | None = None

    def c_struct(self, index, first_lap=2) -> N.McgpTimePenalty:
        """mcgp_time_penalty with the driver index from `index`; ValueError on an unknown kind or a lap that does not
        go with it (the library checks the ranges)."""
        if self.kind not in N.PENALTY_KIND:
            raise ValueError(f"{self.driver}: kind must be 'serve', 'flag' or 'lap', got {self.kind!r}")
        if self.kind == 'flag' and self.lap is not None:
            raise ValueError(f"{self.driver}: a 'flag' penalty has no lap")
        if self.kind == 'lap' and self.lap is None:
            raise ValueError(f"{self.driver}: a 'lap' penalty needs its lap")
        p = N.McgpTimePenalty()
        p.driver = int(index[str(self.driver)])
        p.kind = N.PENALTY_KIND[self.kind]
        p.lap = 0 if self.kind == 'flag' else int(first_lap) if self.lap is None else int(self.lap)
        p.seconds = float(self.seconds)
        return p


@dataclass
class PenaltyResult(StrategyResult):
    """What RaceSimulator.run_penalties returns: StrategyResult's counts and helpers, and
      fate    [S][n][4]   [scenario][driver][fate of the driver's 'serve' penalty]: 0 = it has none in the scenario,
                          1 = served at a stop, 2 = added at the flag, 3 = retired unserved; every row sums to N"""
    fate: np.ndarray | None = None

    def fate_probabilities(self, name, driver) -> dict:
        """{'none' | 'served' | 'at_flag' | 'retired': probability} of `driver`'s 'serve' penalty in scenario `name`."""
        row = np.asarray(self.fate[self._s(name), self._d(driver)], np.float64) / max(self.n_simulations, 1)
        return {k: float(v) for k, v in zip(N.PENALTY_FATES, row)}


# ---------------------------------------------------------------------------------------------- event scenarios
@dataclass
class RaceEvent:
    """One override in a scenario of RaceSimulator.run_events: on laps `lap`..`to_lap` (to_lap None: that one lap) the
    race has a safety car ('sc'), a VSC ('vsc'), a red flag ('red') or no event ('none'), whatever the lap draws.  An
    event is one lap's bunching of the field; a period of several laps is a range."""
    kind: str
    lap: int
    to_lap: int | None = None

    def c_struct(self, first_lap=2, total_laps=None) -> N.McgpLapEvent:
        """mcgp_lap_event; ValueError on an unknown kind, lap > to_lap, or a lap outside [first_lap, total_laps]."""
        if self.kind not in N.EVENT_KIND:
            raise ValueError(f"event kind must be 'sc', 'vsc', 'red' or 'none', got {self.kind!r}")
        a, b = int(self.lap), int(self.lap if self.to_lap is None else self.to_lap)
        if a > b:
            raise ValueError(f'{self.kind}@{a}-{b}: lap must not be above to_lap')
        hi = b if total_laps is None else int(total_laps)
        if a < int(first_lap) or b > hi:
            raise ValueError(f'{self.kind}@{a}' + (f'-{b}' if b != a else '') +
                             f': laps must be in [{int(first_lap)}, {hi}]' +
                             (' (lap 1 has no event)' if int(first_lap) == 2 else " (after the state's lap)"))
        e = N.McgpLapEvent()
        e.first_lap, e.last_lap, e.kind = a, b, N.EVENT_KIND[self.kind]
        return e


@dataclass
class EventResult(StrategyResult):
    """What RaceSimulator.run_events returns: StrategyResult's counts and helpers, and
      events  [S][3][L + 1]   [scenario][red flag, safety car, VSC][number of such laps over the laps run]: the
                              simulations with that many, forced and drawn alike; every row sums to N"""
    events: np.ndarray | None = None

    def _k(self, kind):
        if kind not in N.EVENT_ROWS:
            raise KeyError(f"kind must be one of {N.EVENT_ROWS}, got {kind!r}")
        return N.EVENT_ROWS.index(kind)

    def event_count_distribution(self, name) -> dict:
        """{'red' | 'sc' | 'vsc': probabilities by number of such laps} of scenario `name`."""
        rows = np.asarray(self.events[self._s(name)], np.float64) / max(self.n_simulations, 1)
        return {k: rows[i] for i, k in enumerate(N.EVENT_ROWS)}

    def expected_events(self, name) -> dict:
        """{'red' | 'sc' | 'vsc': mean number of such laps} of scenario `name`."""
        count = np.arange(self.events.shape[2], dtype=np.float64)
        return {k: float(p @ count) for k, p in self.event_count_distribution(name).items()}

    def probability_of(self, name, kind, at_least=1) -> float:
        """P(at least `at_least` laps of `kind`) in scenario `name`."""
        p = self.event_count_distribution(name)[N.EVENT_ROWS[self._k(kind)]]
        return float(p[max(int(at_least), 0):].sum())


# ---------------------------------------------------------------------------------------------- pace scenarios
@dataclass
class PaceOffset:
    """One lap-time offset in a scenario of RaceSimulator.run_paces: `seconds` (finite, |seconds| <= 60; negative =
    faster) added to `driver`'s base pace, either on laps a..b (laps=(a, b)) or from lap p until the pit step of the car's
    next stop (until_stop_from=p): exactly one of the two is given.  The offset enters where the model reads the base
    pace: the lap time, and the pace of the overtake model."""
    driver: str
    seconds: float
    laps: tuple | None = None
    until_stop_from: int | None = None

    def c_struct(self, index, first_lap=1, total_laps=None) -> N.McgpPaceOffset:
        """mcgp_pace_offset with the driver index from `index`; ValueError unless exactly one of laps / until_stop_from
        is given, on a > b, on a lap outside [first_lap, total_laps] and on seconds out of range."""
        who = f'{self.driver}:{self.seconds}'
        if (self.laps is None) == (self.until_stop_from is None):
            raise ValueError(f'{who}: give either laps=(a, b) or until_stop_from=lap')
        sec = float(self.seconds)
        if not math.isfinite(sec) or abs(sec) > N.MAX_PACE_SECONDS:
            raise ValueError(f'{who}: seconds must be finite and in [-60, 60]')
        if self.laps is not None:
            a, b = (int(x) for x in self.laps)
            if a > b:
                raise ValueError(f'{who}@{a}-{b}: the first lap must not be above the last')
        else:
            a = b = int(self.until_stop_from)
        hi = b if total_laps is None else int(total_laps)
        if a < int(first_lap) or b > hi:
            raise ValueError(f'{who}@{a}' + (f'-{b}' if self.laps is not None else '+') +
                             f': laps must be in [{int(first_lap)}, {hi}]' +
                             ('' if int(first_lap) == 1 else " (after the state's lap)"))
        p = N.McgpPaceOffset()
        p.driver = int(index[str(self.driver)])
        p.kind = N.PACE_LAPS if self.laps is not None else N.PACE_UNTIL_STOP
        p.first_lap, p.last_lap = a, b if self.laps is not None else 0
        p.seconds = sec
        return p


@dataclass
class PaceResult(StrategyResult):
    """What RaceSimulator.run_paces returns: StrategyResult's counts and helpers, and
      carried  [S][n][L + 1]  [scenario][driver][laps whose lap time carried the driver's until-stop offset]: from its
                              first lap p, q - p + 1 for a stop on lap q, r - p for a retirement on lap r > p (else 0),
                              L - p + 1 unstopped to the flag; column 0 for a driver without one; every row sums to N"""
    carried: np.ndarray | None = None
    until_from: dict | None = None          # {(scenario name, driver): the first lap of its until-stop offset}

    def carried_distribution(self, name, driver) -> np.ndarray:
        """Probabilities by number of laps carried of `driver`'s until-stop offset in scenario `name`."""
        return np.asarray(self.carried[self._s(name), self._d(driver)], np.float64) / max(self.n_simulations, 1)

    def expected_laps_carried(self, name, driver) -> float:
        p = self.carried_distribution(name, driver)
        return float(p @ np.arange(p.shape[0], dtype=np.float64))

    def probability_cleared_by(self, name, driver, lap) -> float:
        """P(`driver`'s until-stop offset of scenario `name`, which begins on lap p, is carried on at most lap - p + 1
        laps): by the end of `lap` a stop has cleared it or the car is out (a retirement on lap + 1 carries as many laps
        and counts too).  0.0 before p; at the last lap 1.0.  KeyError if the driver has no until-stop offset there."""
        key = (name if name is not None else self.names[0], driver)
        self._s(name), self._d(driver)
        if key not in (self.until_from or {}):
            raise KeyError(f'{driver!r} has no until-stop offset in scenario {key[0]!r}')
        c = int(lap) - self.until_from[key] + 1
        return float(self.carried_distribution(name, driver)[:max(c + 1, 0)].sum()) if c >= 1 else 0.0


# ---------------------------------------------------------------------------------------------- weather scenarios
# The project's own assumption, not the reference's (which has no lap-time cost for the wrong tyres): seconds a lap.
# Slicks lose more the wetter the track and the harder the compound; wet-weather tyres overheat on a dry track; WET on a
# merely damp track and INTERMEDIATE on a fully wet one lose a little to the right tyre.
DEFAULT_WRONG_TYRE_SECONDS = {
    'dry': {'SOFT': 0.0, 'MEDIUM': 0.0, 'HARD': 0.0, 'INTERMEDIATE': 3.0, 'WET': 6.0},
    'damp': {'SOFT': 4.0, 'MEDIUM': 5.0, 'HARD': 6.0, 'INTERMEDIATE': 0.0, 'WET': 1.5},
    'wet': {'SOFT': 12.0, 'MEDIUM': 14.0, 'HARD': 16.0, 'INTERMEDIATE': 2.0, 'WET': 0.0},
}


@dataclass
class TrackChange:
    """One change of the track condition in a scenario of RaceSimulator.run_weather: laps first_lap..last_lap have
    `condition` ('dry', 'damp' or 'wet') instead of the race's track_condition."""
    first_lap: int
    last_lap: int
    condition: str

    def c_struct(self, first_lap=2, total_laps=None) -> N.McgpTrackChange:
        """mcgp_track_change; ValueError on an unknown condition, first_lap > last_lap, or a lap outside [first_lap,
        total_laps]."""
        if self.condition not in N.TRACK_ID:
            raise ValueError(f"condition must be 'dry', 'damp' or 'wet', got {self.condition!r}")
        a, b = int(self.first_lap), int(self.last_lap)
        if a > b:
            raise ValueError(f'{self.condition}@{a}-{b}: first_lap must not be above last_lap')
        hi = b if total_laps is None else int(total_laps)
        if a < int(first_lap) or b > hi:
            raise ValueError(f'{self.condition}@{a}' + (f'-{b}' if b != a else '') +
                             f': laps must be in [{int(first_lap)}, {hi}]' +
                             (" (lap 1 has the configuration's condition)" if int(first_lap) == 2
                              else " (after the state's lap)"))
        c = N.McgpTrackChange()
        c.first_lap, c.last_lap, c.condition = a, b, N.TRACK_ID[self.condition]
        return c


@dataclass
class WeatherModel:
    """The seconds a lap a car loses on a compound under a track condition, for RaceSimulator.run_weather:
    wrong_tyre_seconds = {condition: {compound: seconds}} (finite, in [0, 60]; a cell left out is 0.0).  None: the
    project's default table, DEFAULT_WRONG_TYRE_SECONDS -- an assumption of this project, not a figure of the reference
    model, which has no such cost.  The table is read whether or not the class is wrong."""
    wrong_tyre_seconds: dict | None = None

    def table(self) -> np.ndarray:
        """[3][5] seconds by condition and compound id; ValueError on an unknown name or a value out of range."""
        given = DEFAULT_WRONG_TYRE_SECONDS if self.wrong_tyre_seconds is None else self.wrong_tyre_seconds
        out = np.zeros((3, 5), np.float64)
        for cond, row in given.items():
            if cond not in N.TRACK_ID:
                raise ValueError(f"wrong_tyre_seconds: condition must be 'dry', 'damp' or 'wet', got {cond!r}")
            for comp, sec in row.items():
                if comp not in N.COMPOUND_ID:
                    raise ValueError(f'wrong_tyre_seconds[{cond!r}]: compound must be one of {list(N.COMPOUNDS)}, got {comp!r}')
                sec = float(sec)
                if not math.isfinite(sec) or not 0.0 <= sec <= N.MAX_WRONG_TYRE_SECONDS:
                    raise ValueError(f'wrong_tyre_seconds[{cond!r}][{comp!r}]: seconds must be finite and in [0, 60]')
                out[N.TRACK_ID[cond], N.COMPOUND_ID[comp]] = sec
        return out

    def c_struct(self) -> N.McgpWeatherModel:
        m = N.McgpWeatherModel()
        for c, row in enumerate(self.table()):
            for k, sec in enumerate(row):
                m.wrong_tyre_sec[c][k] = float(sec)
        return m


@dataclass
class WeatherResult(StrategyResult):
    """What RaceSimulator.run_weather returns: StrategyResult's counts and helpers, and
      wrong_laps  [S][n][L + 1]  [scenario][driver][laps whose lap time was computed with the car on the wrong tyres]:
                                 the simulations with that many; every row sums to N"""
    wrong_laps: np.ndarray | None = None

    def wrong_tyre_laps_distribution(self, name, driver) -> np.ndarray:
        """Probabilities by number of laps on the wrong tyres of `driver` in scenario `name`."""
        return np.asarray(self.wrong_laps[self._s(name), self._d(driver)], np.float64) / max(self.n_simulations, 1)

    def expected_wrong_tyre_laps(self, name, driver) -> float:
        p = self.wrong_tyre_laps_distribution(name, driver)
        return float(p @ np.arange(p.shape[0], dtype=np.float64))


# ---------------------------------------------------------------------------------------------- grid scenarios
# The project's own assumption, not the reference's (which has no pit-lane start: it maps 'pitlane_start' to a 20-place
# drop): the seconds a car that starts from the pit lane loses on lap 1 to one that starts from the last grid slot.
DEFAULT_PIT_LANE_SECONDS = 2.5


@dataclass
class GridEdit:
    """One driver's edit of the starting grid in a scenario of RaceSimulator.run_grids: kind 'drop' (value: places, 1 to
    255), 'pin' (value: the slot, 1-based) or 'pit_lane' (seconds added to lap 1).  Use the constructors drop, back, pin
    and pit_lane.  The pit-lane default, DEFAULT_PIT_LANE_SECONDS, is an assumption of this project, not a figure of
    the reference model, which has no pit-lane start."""
    driver: str
    kind: str
    value: int = 0
    seconds: float = 0.0

    KINDS = {'drop': N.GRID_DROP, 'pin': N.GRID_PIN, 'pit_lane': N.GRID_PIT_LANE}

    @classmethod
    def drop(cls, driver, places) -> 'GridEdit':
        """`places` down the drawn grid: an int in [1, 255] or a PENALTY_TYPES name ('engine', 'full_pu', 'gearbox',
        'pitlane_start': the reference's 20-place drop, not a pit-lane start)."""
        if isinstance(places, str):
            from .predictor import PENALTY_TYPES
            if places not in PENALTY_TYPES:
                raise ValueError(f'places must be an int or one of {sorted(PENALTY_TYPES)}, got {places!r}')
            places = PENALTY_TYPES[places]
        return cls(str(driver), 'drop', int(places))

    @classmethod
    def back(cls, driver) -> 'GridEdit':
        """To the back of the grid (in front of any pit-lane starter): the largest drop."""
        return cls(str(driver), 'drop', N.MAX_GRID_DROP)

    @classmethod
    def pin(cls, driver, slot) -> 'GridEdit':
        """On grid slot `slot` (1-based) in every simulation."""
        return cls(str(driver), 'pin', int(slot))

    @classmethod
    def pit_lane(cls, driver, seconds=DEFAULT_PIT_LANE_SECONDS) -> 'GridEdit':
        """From the pit lane: behind the whole grid, and `seconds` more on lap 1."""
        return cls(str(driver), 'pit_lane', 0, float(seconds))

    def __str__(self):
        return (f'{self.driver}:pit_lane+{self.seconds:g}s' if self.kind == 'pit_lane'
                else f'{self.driver}:{self.kind} {self.value}')

    def c_struct(self, index) -> N.McgpGridEdit:
        """mcgp_grid_edit; ValueError on an unknown kind, a value outside its range or seconds where they do not belong."""
        if self.kind not in self.KINDS:
            raise ValueError(f"{self.driver}: kind must be 'drop', 'pin' or 'pit_lane', got {self.kind!r}")
        value, seconds = int(self.value), float(self.seconds)
        if self.kind == 'drop' and not 1 <= value <= N.MAX_GRID_DROP:
            raise ValueError(f'{self}: places must be in [1, {N.MAX_GRID_DROP}]')
        if self.kind == 'pin' and not 1 <= value <= len(index):
            raise ValueError(f'{self}: the slot must be in [1, {len(index)}]')
        if self.kind == 'pit_lane':
            if value != 0:
                raise ValueError(f'{self}: a pit-lane start has no value')
            if not math.isfinite(seconds) or not 0.0 <= seconds <= N.MAX_PIT_LANE_SECONDS:
                raise ValueError(f'{self.driver}: pit-lane seconds must be finite and in [0, 1e6], got {self.seconds!r}')
        elif seconds != 0.0:
            raise ValueError(f'{self}: only a pit-lane start has seconds')
        c = N.McgpGridEdit()
        c.driver, c.kind, c.value, c.seconds = index[str(self.driver)], self.KINDS[self.kind], value, seconds
        return c


@dataclass
class GridResult(StrategyResult):
    """What RaceSimulator.run_grids returns: StrategyResult's counts and helpers, and
      start  [S][n][n]       [scenario][driver][start slot - 1 after the edits]; rows and columns sum to N
      gain   [S][n][2n - 1]  [scenario][driver][(start slot - classified position) + n - 1]: above the centre, places
                             gained from the edited grid; every row sums to N"""
    start: np.ndarray | None = None
    gain: np.ndarray | None = None

    def start_probabilities(self, name=None) -> dict:
        """{driver: {slot: probability}} of scenario `name` (None: {name: that dict} for every scenario)."""
        if name is None:
            return {s: self.start_probabilities(s) for s in self.names}
        return histogram_to_probs(self.start[self._s(name)], self.drivers, max(self.n_simulations, 1))

    def expected_start(self, name) -> dict:
        """{driver: mean start slot (1-based)} of scenario `name`."""
        p = np.asarray(self.start[self._s(name)], np.float64) / max(self.n_simulations, 1)
        slot = np.arange(1, len(self.drivers) + 1, dtype=np.float64)
        return {d: float(p[i] @ slot) for i, d in enumerate(self.drivers)}

    def places_gained_distribution(self, name, driver) -> dict:
        """{places gained from the start slot (negative: lost): probability} of `driver` in scenario `name`."""
        n = len(self.drivers)
        row = np.asarray(self.gain[self._s(name), self._d(driver)], np.float64) / max(self.n_simulations, 1)
        return {int(k - (n - 1)): float(p) for k, p in enumerate(row)}

    def expected_places_gained(self, name, driver) -> float:
        n = len(self.drivers)
        row = np.asarray(self.gain[self._s(name), self._d(driver)], np.float64) / max(self.n_simulations, 1)
        return float(row @ np.arange(-(n - 1), n, dtype=np.float64))


# ---------------------------------------------------------------------------------------------- pace uncertainty
@dataclass
class PacePrior:
    """One item in a scenario of RaceSimulator.run_priors: the standard deviation `sigma` (seconds a lap, in [0, 10]) of
    the error that every simulation draws for the base pace of one driver (PacePrior.driver) or, as one shared draw, of
    the drivers of a group such as a team (PacePrior.group).  A driver's drawn error is the sum of its own and its
    group's."""
    codes: tuple
    sigma: float
    shared: bool = False

    @classmethod
    def driver(cls, code, sigma) -> 'PacePrior':
        return cls((str(code),), float(sigma), False)

    @classmethod
    def group(cls, codes, sigma) -> 'PacePrior':
        return cls(tuple(str(c) for c in codes), float(sigma), True)

    def c_struct(self, index) -> N.McgpPacePrior:
        """mcgp_pace_prior with the driver indices from `index`; ValueError on an empty or repeating group or a sigma
        outside [0, 10]."""
        if not (math.isfinite(self.sigma) and 0.0 <= self.sigma <= N.MAX_PRIOR_SIGMA):
            raise ValueError(f'{"+".join(self.codes)}: sigma must be finite and in [0, {N.MAX_PRIOR_SIGMA:g}], got {self.sigma!r}')
        if not self.codes or len(set(self.codes)) != len(self.codes):
            raise ValueError(f'{"+".join(self.codes)}: a group needs at least one driver, each once')
        p = N.McgpPacePrior()
        p.sigma = float(self.sigma)
        if self.shared:
            p.kind, p.driver = N.PRIOR_GROUP, 0
            p.members = sum(1 << int(index[c]) for c in self.codes)
        else:
            p.kind, p.driver, p.members = N.PRIOR_DRIVER, int(index[self.codes[0]]), 0
        return p


@dataclass
class PriorResult(StrategyResult):
    """What RaceSimulator.run_priors returns: StrategyResult's counts and helpers, and
      draws    [S][n][B][n]  [scenario][driver][bin of the driver's own drawn error][position - 1], B = len(edges) + 1;
                             every [scenario][driver] block sums to N
      edges    [B - 1]       the bins' edges, seconds a lap: bin b holds edges[b - 1] <= x < edges[b]
      offsets  [S][N][n]     the drawn errors (return_offsets=True), else None"""
    draws: np.ndarray | None = None
    offsets: np.ndarray | None = None
    edges: np.ndarray | None = None

    def bin_bounds(self, b) -> tuple:
        """(low, high) of bin `b` in seconds a lap: low <= x < high, -inf and inf at the ends."""
        B = len(self.edges) + 1
        if not 0 <= int(b) < B:
            raise IndexError(f'bin {b} of {B}')
        b = int(b)
        return (float(self.edges[b - 1]) if b > 0 else -math.inf, float(self.edges[b]) if b < B - 1 else math.inf)

    def _block(self, name, driver):
        return np.asarray(self.draws[self._s(name), self._d(driver)], np.float64)

    def draw_probabilities(self, name, driver) -> np.ndarray:
        """[B]: the probability that `driver`'s own drawn error fell into each bin, in scenario `name`."""
        return self._block(name, driver).sum(axis=1) / max(self.n_simulations, 1)

    def position_probabilities_by_draw(self, name, driver) -> np.ndarray:
        """[B][n]: `driver`'s finishing distribution given the bin of its own drawn error; NaN rows for empty bins."""
        block = self._block(name, driver)
        tot = block.sum(axis=1, keepdims=True)
        return np.where(tot > 0, block / np.where(tot > 0, tot, 1.0), np.nan)

    def win_probability_by_draw(self, name, driver) -> np.ndarray:
        """[B]: P(win | bin of the own drawn error); NaN for empty bins."""
        return self.position_probabilities_by_draw(name, driver)[:, 0]

    def expected_points_by_draw(self, name, driver, points=DEFAULT_POINTS) -> np.ndarray:
        """[B]: expected points given the bin of the own drawn error; NaN for empty bins."""
        n = len(self.drivers)
        table = np.zeros(n, np.float64)
        m = min(n, len(points))
        table[:m] = np.asarray(points[:m], np.float64)
        return self.position_probabilities_by_draw(name, driver) @ table


# ---------------------------------------------------------------------------------------------- combined scenarios
@dataclass
class CombinedResult(PenaltyResult, EventResult, PaceResult):
    """What RaceSimulator.run_combined returns: StrategyResult's counts and helpers with PenaltyResult's `fate`,
    EventResult's `events` and PaceResult's `carried` and `until_from`, and the helpers of all three."""
