"""mcgp_run_championship_bonus on the device: every output equals championship_bonus_ref fed with the CPU oracle's
finishing orders and per-lap traces, cell for cell, after the reference alone has shown that the case reaches what it is
there for.  No tolerance anywhere.

Wall time on one MI355X: 1.5 s for the 23 tests, none above 0.2 s (the oracle's traced runs included)."""
import copy
import ctypes as C

import numpy as np
import pytest

import championship_bonus_ref as BR
import championship_cases as CC
import championship_rounds_ref as RR
import oracle_py as O
import resume_ref as RS
import trace_ref as TR
from monte_carlo_gp_amd import RaceConfig, run_championship
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

F1 = [25, 18, 15, 12, 10, 8, 6, 4, 2, 1]
SPRINT = [8, 7, 6, 5, 4, 3, 2, 1]
SEASON = ('champ_hist', 'team_hist', 'gain_hist', 'race_hist')
ROUNDS = RR.KEYS
BONUS = ('bonus_hist', 'fastest_hist')
ALL = SEASON + ROUNDS + BONUS
KERNEL = 'mcgp::race_fastest_kernel'


class Season:
    """A calendar for the C ABI: cases (one per race, the same drivers), seeds, tables, countback, bonuses, standings."""

    def __init__(self, cases, seeds, tables, cb, bonus, within, ip=None, ic=None):
        self.cases, self.seeds_py, self.tables, self.cb_py = cases, [int(s) for s in seeds], tables, [int(c) for c in cb]
        self.bonus_py, self.within_py = [int(b) for b in bonus], [int(w) for w in within]
        self.drivers = list(cases[0]['grid_probs'])
        n, R = self.n, self.R = len(self.drivers), len(cases)
        self.team, self.T = CC.team_of(dict(case=cases[0]))
        self.keep = [(RS.problem(c), np.ascontiguousarray(O.Problem(c).grid_probs, np.float64)) for c in cases]
        self.cfgs = (N.McgpConfig * R)(*[p.cfg for p, _ in self.keep])
        self.drvs = (N.McgpDrivers * R)(*[p.drv for p, _ in self.keep])
        self.grids = (C.POINTER(C.c_double) * R)(*[g.ctypes.data_as(C.POINTER(C.c_double)) for _, g in self.keep])
        self.seeds = (C.c_uint64 * R)(*self.seeds_py)
        self.points = np.zeros((R, n), np.int32)
        for r, t in enumerate(tables):
            self.points[r, :min(n, len(t))] = t[:n]
        self.cb = np.ascontiguousarray(self.cb_py, np.uint8)
        self.team32 = np.ascontiguousarray(self.team, np.int32)
        self.ip = None if ip is None else np.ascontiguousarray(ip, np.int32)
        self.ic = None if ic is None else np.ascontiguousarray(ic, np.int32)
        self.bonus = np.ascontiguousarray(self.bonus_py, np.int32)
        self.within = np.ascontiguousarray(self.within_py, np.int32)
        self.G0 = int(self.points.max(axis=1).sum())
        self.G = self.G0 + sum(self.bonus_py)

    def arrays(self, fill=0, G=None):
        R, n, T, G = self.R, self.n, self.T, self.G if G is None else G
        shapes = dict(champ_hist=(n, n), team_hist=(T, T), gain_hist=(n, G + 1), race_hist=(R, n, n), round_hist=(R, n, n),
                      contend=(R, n), secure=(R, n), team_round_hist=(R, T, T), team_contend=(R, T), team_secure=(R, T),
                      bonus_hist=(R, n), fastest_hist=(R, n))
        return {k: np.full(s, fill, np.uint64) for k, s in shapes.items()}

    def run(self, n_sims, offset=0, out=None, drop=(), entry='bonus', device=0):
        """(rc, message, arrays as int64).  drop: output names passed as NULL."""
        out = out if out is not None else self.arrays(G=self.G if entry == 'bonus' else self.G0)
        i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        ptr = lambda k: None if k in drop else out[k].ctypes.data_as(C.POINTER(C.c_uint64))
        lib = N.lib()
        args = [self.R, self.cfgs, self.drvs, self.grids, self.n, int(n_sims), int(offset), self.seeds, i32(self.points),
                self.cb.ctypes.data_as(C.POINTER(C.c_uint8)), i32(self.ip), i32(self.ic), i32(self.team32), self.T, device]
        args += [ptr(k) for k in SEASON]
        if entry == 'plain':
            rc = lib.mcgp_run_championship(*args)
        elif entry == 'rounds':
            rc = lib.mcgp_run_championship_rounds(*args, *[ptr(k) for k in ROUNDS])
        else:
            rc = lib.mcgp_run_championship_bonus(*args, *[ptr(k) for k in ROUNDS], i32(self.bonus), i32(self.within),
                                                 *[ptr(k) for k in BONUS])
        return rc, lib.mcgp_last_error().decode(), {k: v.astype(np.int64) for k, v in out.items()}

    def reference(self, n_sims, offset=0, races=None):
        races = races or [BR.race(c, n_sims, s, offset) for c, s in zip(self.cases, self.seeds_py)]
        ref = BR.season(races, self.tables, self.cb_py, self.team, self.T, self.bonus_py, self.within_py,
                        None if self.ip is None else self.ip.astype(np.int64), None if self.ic is None else self.ic.astype(np.int64))
        return races, ref


def _assert_equal(got, ref, keys=ALL, what=''):
    for k in keys:
        assert np.array_equal(got[k], ref[k]), (what, k)


def _kernel():
    return N.lib().mcgp_last_kernel_name(0).decode()


@pytest.fixture(scope='module')
def s60_races():
    """The oracle's S60 under seeds 1, 2, 3, 256 simulations, with their fastest laps: shared, never changed."""
    case = O.load_case('S60')
    return case, [BR.race(case, 256, s) for s in (1, 2, 3)]


# ---------------------------------------------------------------- 1
def test_zero_bonus_equals_the_existing_calls(require_gpu):
    """3 races, 20 cars, 1000 simulations, no bonus anywhere: the by-round call's outputs, and with the round trio NULL
    the plain call's; the two bonus histograms stay as they were."""
    cases = [O.load_case(k) for k in ('S60', 'S78', 'S50')]
    s = Season(cases, [11, 12, 13], [F1, SPRINT, F1], [1, 0, 1], [0, 0, 0], [10, 0, -3], ip=np.arange(20) * 3)
    rc, err, got = s.run(1000, 77, out=s.arrays(fill=5))
    assert rc == 0, err
    rc, err, rounds = s.run(1000, 77, out=s.arrays(fill=5), entry='rounds')
    assert rc == 0, err
    _assert_equal(got, rounds, SEASON + ROUNDS)
    assert (got['bonus_hist'] == 5).all() and (got['fastest_hist'] == 5).all()
    assert _kernel() != KERNEL                                      # every race went through mcgp_run's launch path
    trio = ROUNDS
    rc, err, got = s.run(1000, 77, drop=trio)
    assert rc == 0, err
    rc, err, plain = s.run(1000, 77, drop=trio, entry='plain')
    assert rc == 0, err
    _assert_equal(got, plain, SEASON)
    assert all(not got[k].any() for k in ROUNDS) and got['champ_hist'].sum() == 20 * 1000


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize('within', [10, 3])
def test_the_rule_on_s60(require_gpu, s60_races, within):
    """S60 x seeds 1, 2, 3, 256 simulations, 1 point within the top ten: the bonus changes the champion in 6 simulations.
    Within the top three, 67 of the 768 fastest laps are not eligible (2 at within 10)."""
    case, races = s60_races
    s = Season([case] * 3, [1, 2, 3], [F1] * 3, [1] * 3, [1] * 3, [within] * 3)
    _, ref = s.reference(256, races=races)
    changed = BR.changed_by_the_bonus(races, s.tables, s.cb_py, s.team, s.T, s.bonus_py, s.within_py)
    outside = int((ref['fastest_hist'] - ref['bonus_hist']).sum())
    if within == 10:
        assert changed['champions'] == 6 and changed['champ_cells'] == 37 and outside == 2
    else:
        assert changed['champions'] >= 1 and outside == 67
    rc, err, got = s.run(256)
    assert rc == 0, err
    _assert_equal(got, ref)
    assert _kernel() == KERNEL


# ---------------------------------------------------------------- 3
def test_fastest_laps_by_cars_that_retire_later(require_gpu):
    """EVT at seed 42: 31 fastest laps by cars that retire afterwards, 13 classified inside the top ten (they take the
    point) and 18 outside."""
    case = O.load_case('EVT')
    s = Season([case], [42], [F1], [1], [1], [10])
    races, ref = s.reference(256)
    late = races[0]['fl_retired']
    assert (int((late & (races[0]['fl_pos'] < 10)).sum()), int((late & (races[0]['fl_pos'] >= 10)).sum())) == (13, 18)
    rc, err, got = s.run(256)
    assert rc == 0, err
    _assert_equal(got, ref)


# ---------------------------------------------------------------- 4
def _layout_season(n, top=0x7FFF):
    """Two races of field_case(n), table 5-3-1, race 0 with a bonus of 7 within n // 2, race 1 with 40 within n.  Every
    driver carries in top - (17 .. 39): tables and the first bonus (17 at most) never reach `top`, the second bonus
    always passes it."""
    rng = np.random.default_rng(900 + n)
    case = RS.field_case(n)
    ip = top - rng.integers(17, 40, n)
    ic = rng.integers(0, 30, (n, n))
    return Season([case, case], [31 + n, 62 + n], [[5, 3, 1]] * 2, [1, 1], [7, 40], [max(1, n // 2), n], ip, ic)


@pytest.mark.parametrize('n', [9, 10, 11, 12, 22, 23, 24, 25, 32])
def test_key_layout(require_gpu, n):
    """The bonus add carries across bit 15 of the points field in every key that takes race 1's bonus and in no other;
    at n = 10, 11, 12, 23, 24, 25 the field straddles a word (14, 9, 4, 13, 8, 3 bits in the lower one) and the same add
    carries across the word boundary.  Team keys are built from these: team_hist and the team rounds equal the ref."""
    s = _layout_season(n)
    races, ref = s.reference(200)
    pts = ref['final'][0]
    took = np.zeros(pts.shape, bool)
    hit = np.nonzero(races[1]['fl_driver'] >= 0)[0]
    took[hit, races[1]['fl_driver'][hit]] = True
    assert took.any() and np.array_equal(pts > 0x7FFF, took)           # bit 15 set by the bonus add alone
    low = CC.points_low_bits(n)
    assert (low > 0) == (n in CC.POINTS_STRADDLE)
    if low:
        before = pts[took] - 40
        assert ((before & ((1 << low) - 1)) + 40 >= (1 << low)).all()   # ... which also leaves the lower word
    rc, err, got = s.run(200)
    assert rc == 0, err
    _assert_equal(got, ref)


def test_key_layout_at_exactly_65535(require_gpu):
    """23 cars (points field across two words): whoever wins both races and takes both bonuses ends on exactly 65 535;
    one more carried-in point is MCGP_E_BAD_ARG and leaves the outputs untouched."""
    n = 23
    s = _layout_season(n)
    s.ip = np.full(n, 65535 - s.G, np.int32)
    races, ref = s.reference(600)
    assert (ref['final'][0] == 65535).any()
    rc, err, got = s.run(600)
    assert rc == 0, err
    _assert_equal(got, ref)
    s.ip[n - 1] += 1
    out = s.arrays(fill=9)
    rc, err, got = s.run(600, out=out)
    assert rc == -1 and '65535' in err and all((v == 9).all() for v in got.values())


# ---------------------------------------------------------------- 5
def test_races_of_one_lap_have_no_fastest_lap(require_gpu):
    case = copy.deepcopy(O.load_case('S60'))
    case['config']['total_laps'] = 1
    # a bonus in every race: against the ref (the bounds count bonuses nobody can take); both histograms stay zero
    s = Season([case] * 3, [5, 6, 7], [F1] * 3, [1, 0, 1], [1, 2, 3], [10, 10, 10])
    races, ref = s.reference(300)
    assert all((r['fl_driver'] == BR.NONE).all() for r in races)
    rc, err, got = s.run(300)
    assert rc == 0, err
    _assert_equal(got, ref)
    assert not got['bonus_hist'].any() and not got['fastest_hist'].any() and _kernel() == KERNEL
    # a bonus in the first race only, so that no bound changes: everything else equals the zero-bonus call
    s = Season([case] * 3, [5, 6, 7], [F1] * 3, [1, 0, 1], [4, 0, 0], [10, 10, 10])
    zero = Season([case] * 3, [5, 6, 7], [F1] * 3, [1, 0, 1], [0, 0, 0], [10, 10, 10])
    rc, err, got = s.run(300)
    assert rc == 0, err
    rc, err, base = zero.run(300)
    assert rc == 0, err
    _assert_equal(got, base, ('champ_hist', 'team_hist', 'race_hist') + ROUNDS)
    assert np.array_equal(got['gain_hist'][:, :zero.G + 1], base['gain_hist']) and not got['gain_hist'][:, zero.G + 1:].any()
    assert not got['bonus_hist'].any() and not got['fastest_hist'].any()


# ---------------------------------------------------------------- 6
def test_edges_of_within(require_gpu):
    """Ten cars, within 10: every fastest lap takes the bonus.  Within 1: only winners.  One car: always."""
    case = O.load_case('N10')
    s = Season([case, case], [42, 43], [F1, F1], [1, 1], [1, 2], [10, 1])
    races, ref = s.reference(256)
    assert np.array_equal(ref['bonus_hist'][0], ref['fastest_hist'][0]) and ref['fastest_hist'][0].sum() == 256
    winners = int(((races[1]['fl_pos'] == 0)).sum())
    assert 0 < winners < 256 and ref['bonus_hist'][1].sum() == winners
    rc, err, got = s.run(256)
    assert rc == 0, err
    _assert_equal(got, ref)
    one = RS.field_case(1)
    s = Season([one, one], [3, 4], [[5], [5]], [1, 1], [2, 3], [1, 1], ip=[65535 - 15])
    races, ref = s.reference(100)
    assert ref['bonus_hist'].sum() > 0 and ref['final'][0].max() == 65535
    rc, err, got = s.run(100)
    assert rc == 0, err
    _assert_equal(got, ref)


# ---------------------------------------------------------------- 7
def test_mixed_calendar_and_optional_outputs(require_gpu, s60_races):
    """A sprint (no countback, no bonus), then a Grand Prix with the point: only the Grand Prix rows are written, into
    buffers that held 7s; then bonus_hist NULL, then fastest_hist NULL."""
    case, races = s60_races
    s = Season([case, case], [1, 2], [SPRINT, F1], [0, 1], [0, 1], [10, 10])
    _, ref = s.reference(256, races=races[:2])
    assert not ref['bonus_hist'][0].any() and ref['fastest_hist'][1].sum() == 256
    rc, err, got = s.run(256, out=s.arrays(fill=7))
    assert rc == 0, err
    for k in ALL:
        assert np.array_equal(got[k], ref[k] + 7), k
    assert (got['bonus_hist'][0] == 7).all() and (got['fastest_hist'][0] == 7).all()
    for drop in BONUS:
        rc, err, got = s.run(256, drop=(drop,))
        assert rc == 0, err
        _assert_equal(got, ref, [k for k in ALL if k != drop])
        assert not got[drop].any()


# ---------------------------------------------------------------- 8
def test_identities_at_20000_simulations(require_gpu):
    """fastest_hist is mcgp_run_trace's fastest lap count and race_hist mcgp_run's histogram, race by race."""
    n_sims, offset = 20000, 1234
    cases = [O.load_case('S60'), O.load_case('EVT')]
    s = Season(cases, [42, 43], [F1, F1], [1, 1], [1, 1], [10, 5])
    rc, err, got = s.run(n_sims, offset)
    assert rc == 0, err
    for r, (case, (prob, grid)) in enumerate(zip(cases, s.keep)):
        rc, trace = TR.run_c(case, n_sims, s.seeds_py[r], offset, prob=prob)
        assert rc == 0
        assert np.array_equal(got['fastest_hist'][r], trace['fastest'])
        hist = np.zeros((20, 20), np.uint64)
        assert N.lib().mcgp_run(C.byref(prob.cfg), C.byref(prob.drv), grid.ctypes.data_as(C.POINTER(C.c_double)), 20, n_sims,
                                offset, s.seeds_py[r], 0, hist.ctypes.data_as(C.POINTER(C.c_uint64)), None) == 0
        assert np.array_equal(got['race_hist'][r], hist.astype(np.int64))
    assert (got['bonus_hist'] <= got['fastest_hist']).all()
    assert (got['bonus_hist'].sum(axis=1) <= got['fastest_hist'].sum(axis=1)).all() and (got['fastest_hist'].sum(axis=1) <= n_sims).all()
    assert 0 < got['bonus_hist'][1].sum() < got['fastest_hist'][1].sum()
    assert (got['gain_hist'].sum(axis=1) == n_sims).all()
    RR.assert_identities(got, n_sims, got['champ_hist'], got['team_hist'])


# ---------------------------------------------------------------- 9
def test_in_contention_only_because_of_the_bonus_to_come(require_gpu):
    """Six cars in pairs, three races of 3-2-1 with a point each, driver 0 carrying in 7: after a race a rival (a team)
    trails by more than the tables still pay and by no more than tables plus bonuses -- in contention by the bonus
    alone."""
    case = CC.field(6, team=[0, 0, 1, 1, 2, 2])
    s = Season([case] * 3, [21, 22, 23], [[3, 2, 1]] * 3, [1, 1, 1], [1, 1, 1], [6, 6, 6], ip=[7, 0, 0, 0, 0, 0])
    races, ref = s.reference(400)
    M0, B0 = RR.remaining(s.tables, 6, s.team, s.T)                  # without the bonuses
    drivers = teams = 0
    for r, per in enumerate(ref['per'][:-1]):
        gap = per['pts'].max(axis=1)[:, None] - per['pts']
        drivers += int(((gap > M0[r]) & (gap <= per['M']) & (per['pos'] != 0)).sum())
        tgap = per['tp'].max(axis=1)[:, None] - per['tp']
        teams += int(((tgap > B0[r][None, :]) & (tgap <= per['B'][None, :]) & (per['tpos'] != 0)).sum())
        assert per['M'] == M0[r] + (2 - r)
    assert drivers >= 1 and teams >= 1, (drivers, teams)
    rc, err, got = s.run(400)
    assert rc == 0, err
    _assert_equal(got, ref)
    assert np.array_equal(got['secure'][-1], got['champ_hist'][:, 0])
    assert np.array_equal(got['team_secure'][-1], got['team_hist'][:, 0])
    assert (np.diff(got['secure'], axis=0) >= 0).all() and (np.diff(got['team_secure'], axis=0) >= 0).all()


# ---------------------------------------------------------------- 10
def test_accumulation_and_an_odd_split(require_gpu, s60_races):
    """Two calls split at 101 of 256 into buffers that held 3s equal the ref + 3."""
    case, races = s60_races
    s = Season([case] * 3, [1, 2, 3], [F1] * 3, [1] * 3, [1, 0, 1], [10, 10, 10], ip=np.arange(20))
    _, ref = s.reference(256, races=races)
    out = s.arrays(fill=3)
    assert s.run(101, 0, out=out)[0] == 0
    rc, err, got = s.run(155, 101, out=out)
    assert rc == 0, err
    for k in ALL:
        assert np.array_equal(got[k], ref[k] + 3), k


def test_python_surface_on_two_shards(require_gpu, s60_races):
    """run_championship with the two per-race keys, sharded over device=[0, 0], equals the ref."""
    case, races = s60_races
    race = lambda seed, **kw: dict(config=RaceConfig(**case['config']), grid_probs=case['grid_probs'], base_pace=case['base_pace'],
                                   tire_deg=case['tire_deg'], driver_variance=case['driver_variance'],
                                   driver_dnf_rates=case['driver_dnf_rates'], track_condition=case['track_condition'],
                                   seed=seed, **kw)
    calendar = [race(1, fastest_lap_points=1), race(2), race(3, fastest_lap_points=2, fastest_lap_within=3)]
    s = Season([case] * 3, [1, 2, 3], [F1] * 3, [1] * 3, [1, 0, 2], [10, 10, 3])
    _, ref = s.reference(256, races=races)
    for device, by_round in ((0, False), ([0, 0], True)):
        res = run_championship(calendar, 256, set_pop=RS.SET_POP, device=device, return_race_histograms=True, by_round=by_round)
        assert np.array_equal(res.champ_hist, ref['champ_hist']) and np.array_equal(res.team_hist, ref['team_hist'])
        assert np.array_equal(res.gain_hist, ref['gain_hist']) and np.array_equal(np.array(res.race_histograms), ref['race_hist'])
        assert np.array_equal(res.bonus_counts, ref['bonus_hist']) and np.array_equal(res.fastest_lap_counts, ref['fastest_hist'])
        if by_round:
            for k in ROUNDS:
                assert np.array_equal(getattr(res, k), ref[k]), k
    exp = res.expected_bonus_points
    assert sum(exp.values()) == pytest.approx((ref['bonus_hist'][0].sum() + 2 * ref['bonus_hist'][2].sum()) / 256)
    g = np.arange(res.gain_hist.shape[1])
    assert sum(res.expected_points.values()) == pytest.approx(float((res.gain_hist * g).sum()) / 256)


def test_across_the_chunk_boundary(require_gpu):
    """2^22 + 1000 simulations of a 4-car, 25-lap field, two races with a bonus: the whole run equals two calls split at
    2^22 (the second chunk starts its keys from the standings again, in buffers the first chunk has used), and the
    1000 simulations behind the boundary equal the ref."""
    case = CC.field(4)
    s = Season([case, case], [8, 9], [[3, 2, 1]] * 2, [1, 1], [1, 2], [2, 4], ip=[3, 0, 0, 0])
    cut, n_sims = 1 << 22, (1 << 22) + 1000
    rc, err, whole = s.run(n_sims, 5)
    assert rc == 0, err
    parts = s.arrays()
    assert s.run(cut, 5, out=parts)[0] == 0
    first = {k: v.copy() for k, v in parts.items()}
    rc, err, both = s.run(1000, 5 + cut, out=parts)
    assert rc == 0, err
    _assert_equal(whole, both)
    _, ref = s.reference(1000, 5 + cut)
    for k in ALL:
        assert np.array_equal(both[k] - first[k].astype(np.int64), ref[k]), k
    assert (whole['gain_hist'].sum(axis=1) == n_sims).all() and (whole['fastest_hist'].sum(axis=1) <= n_sims).all()
    RR.assert_identities(whole, n_sims, whole['champ_hist'], whole['team_hist'])


def test_every_bad_argument_leaves_the_outputs_untouched(require_gpu):
    case = RS.field_case(3)
    good = dict(bonus=[1, 0], within=[3, 0])
    bad = [dict(bonus=[-1, 0]), dict(bonus=[1, 65536]), dict(within=[0, 0]), dict(within=[4, 0]), dict(bonus=[0, 1], within=[3, 9])]
    for kw in bad:
        a = dict(good, **kw)
        s = Season([case, case], [1, 2], [[3, 2, 1]] * 2, [1, 1], a['bonus'], a['within'])
        s.G = s.G0 + 2
        rc, err, got = s.run(500, out=s.arrays(fill=11))
        assert rc == -1 and ('bonus_points[' in err or 'bonus_within[' in err), (kw, err)
        assert all((v == 11).all() for v in got.values()), kw
    s = Season([case, case], [1, 2], [[3, 2, 1]] * 2, [1, 1], [1, 0], [3, 0])
    for drop in (('round_hist',), ('contend',), ROUNDS[:3], ('champ_hist',)):
        rc, err, got = s.run(500, out=s.arrays(fill=11), drop=drop)
        assert rc == -1, (drop, err)
        assert all((v == 11).all() for v in got.values()), drop
    wide = copy.deepcopy(case)
    p = Season([wide, wide], [1, 2], [[3, 2, 1]] * 2, [1, 1], [0, 1], [1, 1])
    p.keep[1][0].cfg.deviates = 1
    p.cfgs[1].deviates = 1
    rc, err, got = p.run(500, out=p.arrays(fill=11))
    assert rc == -1 and 'bonus_points[1]' in err and 'MCGP_DEVIATES_32' in err
    assert all((v == 11).all() for v in got.values())
