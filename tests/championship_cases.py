"""Seasons that take the standings kernels to the limits of their key layout (csrc/championship.hip.h), and the proof,
from championship_ref alone, that a season got there.

TEST INFRASTRUCTURE, shared by the device tests (test_gpu_championship_limits.py), the host build of the kernels
(test_champ_host_build.py), the by-round call's device and host-build tests (test_gpu_championship_rounds_limits.py,
test_champ_rounds_host_build.py; their proofs read championship_rounds_ref's per-simulation view, "by round" below) and
the builders' own tests (test_championship_host.py).  A season is a dict:
case (an n-car race, S60's parameters), plan [(case, seed, 32, points table, countback)] as test_gpu_championship._check
takes it, standings {driver: {'points', 'finishes'}}, n_sims, sim_offset.  Teams are case['config']['driver_teams'], in
order of first appearance.

The layout restated (driver keys: 16-bit points above n 5-bit counts, the count of position p + 1 at bit
5 (n - 1 - p)): a field that straddles a 64-bit word is where a carry leaves a word and where a field is read in two
pieces.  Count fields straddle at bit 60 (position index n - 13, 4 low bits) and bit 125 (n - 26, 3 low bits); the points
field straddles for n in POINTS_STRADDLE, with `points_low_bits(n)` bits in the lower word.
"""
import json

import numpy as np

import championship_ref as CR
import championship_rounds_ref as RR
import oracle_py as O

F1 = [25, 18, 15, 12, 10, 8, 6, 4, 2, 1]
SPRINT = [8, 7, 6, 5, 4, 3, 2, 1]
SHORT = [3, 2, 1]
POINTS_STRADDLE = (10, 11, 12, 23, 24, 25)
MAX_POINTS, MAX_COUNT = 65535, 31


def points_low_bits(n):
    """Bits of the points field in the lower of its two words, or 0 when it lies in one word."""
    b = (5 * n) % 64
    return 64 - b if b + 16 > 64 else 0


def field(n, pace_step=0.02, variance=0.2, dnf=0.01, team=None, one_hot_grid=False, laps=25):
    """An n-car race with S60's parameters: base pace 90 s + pace_step per driver index.  team: a team index per
    driver, numbered in order of first appearance (default: driver index mod 10)."""
    rng = np.random.default_rng(n)
    drivers = [f'D{i:02d}' for i in range(n)]
    base = O.load_case('S60')
    team = [i % 10 for i in range(n)] if team is None else [int(t) for t in team]
    seen = []
    for t in team:
        if t not in seen:
            seen.append(t)
    assert seen == list(range(len(seen))), 'teams are numbered in order of first appearance'
    names = [f'T{t:02d}' for t in range(len(seen))]
    case = dict(base)
    case['config'] = dict(base['config'], total_laps=laps, driver_teams={d: names[team[i]] for i, d in enumerate(drivers)},
                          dnf_rates={t: 0.0 for t in names})
    if one_hot_grid:
        g = np.eye(n)
    else:
        g = rng.random((n, n))
        g[:, n // 2] = 0.0
    case['grid_probs'] = {d: [float(x) for x in g[i]] for i, d in enumerate(drivers)}
    case['base_pace'] = {d: 90.0 + pace_step * i for i, d in enumerate(drivers)}
    case['tire_deg'] = {d: 0.05 for d in drivers}
    case['driver_variance'] = {d: variance for d in drivers}
    case['driver_dnf_rates'] = {d: dnf for d in drivers}
    return case


def team_of(season):
    """(team index per driver, number of teams) of a season."""
    case = season['case']
    names, team = [], []
    for d in case['grid_probs']:
        t = case['config']['driver_teams'][d]
        if t not in names:
            names.append(t)
        team.append(names.index(t))
    return team, len(names)


def standings_arrays(season):
    drivers = list(season['case']['grid_probs'])
    n = len(drivers)
    p, c = np.zeros(n, np.int64), np.zeros((n, n), np.int64)
    for d, v in season['standings'].items():
        i = drivers.index(d)
        p[i] = v['points']
        c[i, :len(v['finishes'])] = v['finishes']
    return p, c


def tie_rich_points(n, points=40000):
    """The carried-in total of the tie-rich season: `points`, but where the points field straddles a word its lower
    piece is 3 short of full, so that a gain of 3 or more carries into the next word and a smaller one does not."""
    low = points_low_bits(n)
    return points if not low else (points >> low << low) + (1 << low) - 3


def tie_rich(n, team=None, n_sims=500, races=5, table=SHORT, points=None, counts=None, seed=2000, sim_offset=7,
             countback=None):
    """Every driver carries in the same large points total and the same counts, the field is close (0.02 s a step) and
    the table is short: standings tie on points and on the leading counts, so that the ranking is decided in every
    field.  counts {position index: count}; default 15 at n - 13 and 7 at n - 26 (the straddling count fields, one
    short of carrying)."""
    case = field(n, team=team)
    drivers = list(case['grid_probs'])
    if counts is None:
        counts = {p: c for p, c in ((n - 13, 15), (n - 26, 7)) if p >= 0}
    fin = [int(counts.get(p, 0)) for p in range(n)]
    pts = tie_rich_points(n) if points is None else points
    pts = [int(x) for x in pts] if isinstance(pts, (list, tuple)) else [int(pts)] * n
    # the last race is a sprint: it scores and does not count back, so that equal points, wins and seconds do not
    # already mean equal thirds under a three-place table
    cb = [True] * (races - 1) + [False] if countback is None else list(countback)
    tables = table if isinstance(table[0], (list, tuple)) else [table] * races
    plan = [(case, seed + 31 * n + r, 32, list(tables[r]), bool(cb[r])) for r in range(races)]
    G = sum(max(list(t[:n]) + [0]) for t in tables)
    assert max(pts) + G <= MAX_POINTS and max(fin + [0]) + sum(cb) <= MAX_COUNT
    return dict(case=case, plan=plan, standings={d: {'points': pts[i], 'finishes': fin} for i, d in enumerate(drivers)},
                n_sims=n_sims, sim_offset=sim_offset)


def procession(n, n_sims=200, seed=500):
    """31 Grands Prix that the cars finish in grid order nearly every time: driver 0, who carries in 65 535 - 31 x 25
    points, ends most seasons on a count of 31 wins and on 65 535 points, both limits of a driver key."""
    case = field(n, pace_step=1.0, variance=0.05, dnf=0.0, one_hot_grid=True)
    drivers = list(case['grid_probs'])
    plan = [(case, seed + n + r, 32, F1, True) for r in range(31)]
    return dict(case=case, plan=plan, standings={drivers[0]: {'points': MAX_POINTS - 31 * 25, 'finishes': []}},
                n_sims=n_sims, sim_offset=0)


def long_calendar(n=5, n_sims=300, seed=640):
    """64 races, the most a call takes: 31 Grands Prix (the most that count back) and 33 sprints, interleaved."""
    case = field(n)
    drivers = list(case['grid_probs'])
    plan = []
    for r in range(64):
        gp = r % 2 == 0 and r < 62
        plan.append((case, seed + r, 32, F1 if gp else SPRINT, gp))
    return dict(case=case, plan=plan, standings={drivers[1]: {'points': 9, 'finishes': [0, 0, 0]}}, n_sims=n_sims,
                sim_offset=3)


def uneven_teams(n_sims=600, seed=4000):
    """Seven cars in teams of 3, 2, 1 and 1, so that the points a team can still take (B_r(e), championship_rounds_ref)
    differ from team to team: [43 35 22 22] after race 0, falling to [3 3 2 2] after race 4.  Five short Grands Prix
    and a two-place sprint; the single-driver teams, the slowest cars, carry in 5 points each and the pair 2 + 2, so
    that team totals stay within a few points of each other's bounds."""
    team = [0, 0, 0, 1, 1, 2, 3]
    case = field(7, pace_step=0.05, team=team)
    drivers = list(case['grid_probs'])
    tables = [[5, 3, 2, 1]] * 5 + [[2, 1]]
    plan = [(case, seed + r, 32, tables[r], r < 5) for r in range(6)]
    carried = [0, 0, 0, 2, 2, 5, 5]
    return dict(case=case, plan=plan, standings={d: {'points': carried[i], 'finishes': []} for i, d in enumerate(drivers)},
                n_sims=n_sims, sim_offset=3)


DUEL_GAP, DUEL_ROW = 103, 20


def procession_duel(n, n_sims=200, seed=500):
    """procession(n) with a rival: driver 1 carries in 103 points fewer than driver 0.  In a procession driver 0 gains
    25 a race and driver 1 gains 18, so after race index 20 the gap is 103 + 7 x 21 = 250 = 25 x 10 = M_20, exactly the
    bound, and one race later driver 1 is out.  There both totals are above 65 000: bit 15 of both points fields is
    set, and lead - points is a difference of two such fields."""
    season = procession(n, n_sims=n_sims, seed=seed)
    drivers = list(season['case']['grid_probs'])
    lead = season['standings'][drivers[0]]['points']
    assert lead == MAX_POINTS - 775 and DUEL_GAP + 7 * (DUEL_ROW + 1) == 25 * (30 - DUEL_ROW)
    season['standings'][drivers[1]] = {'points': lead - DUEL_GAP, 'finishes': []}
    return season


# ------------------------------------------------------------------------------------------------ team layouts
def bits(x):
    b = 1
    while x >> b:
        b += 1
    return b


def team_layout(season):
    """(count bits, words) of the season's team keys by the documented rule (include/mcgp.h): a count field holds the
    largest carried-in team count plus the countback races, the points field the largest carried-in team total plus
    min(members x G, the points the races award in all)."""
    team, T = team_of(season)
    n = len(team)
    ip, ic = standings_arrays(season)
    tables = [list(p[3][:n]) + [0] * (n - len(p[3][:n])) for p in season['plan']]
    G, awarded, n_cb = sum(max(t) for t in tables), sum(sum(t) for t in tables), sum(int(p[4]) for p in season['plan'])
    max_p = max_c = 0
    for t in range(T):
        mem = [d for d in range(n) if team[d] == t]
        max_p = max(max_p, int(ip[mem].sum()) + min(len(mem) * G, awarded))
        max_c = max(max_c, int(ic[mem].sum(axis=0).max()) + n_cb)
    return bits(max_c), (bits(max_p) + bits(max_c) * n + 63) // 64


def team_points_bits(season):
    """Bits of the points field of the season's team keys by team_layout's rule: what the largest total a team can
    reach needs.  The field starts at bit n x count bits."""
    team, T = team_of(season)
    n = len(team)
    ip, _ = standings_arrays(season)
    tables = [list(p[3][:n]) + [0] * (n - len(p[3][:n])) for p in season['plan']]
    G, awarded = sum(max(t) for t in tables), sum(sum(t) for t in tables)
    return bits(max(int(ip[[d for d in range(n) if team[d] == t]].sum()) + min(team.count(t) * G, awarded) for t in range(T)))


def rank_lds_bytes(n, T, team_words, gain_cols, gain_in_lds):
    """champ_rank_lds (csrc/championship.hip.h) restated: the rank kernel's LDS."""
    words = (16 + 5 * n + 63) // 64
    b = words * n * 64 * 8 + team_words * T * 64 * 8 + n * n * 4 + T * T * 4 + (n * gain_cols * 4 if gain_in_lds else 0)
    return (b + 15) // 16 * 16


def round_lds_bytes(n, T, team_words):
    """champ_round_lds (csrc/champ_rounds.hip.h) restated: the by-round kernel's LDS.  Driver keys, team keys, six rows
    of 64 u32 per simulation, and the u32 histograms n x n + 2 n + T x T + 2 T.  T = 0: drivers only."""
    words = (16 + 5 * n + 63) // 64
    b = words * n * 64 * 8 + team_words * T * 64 * 8 + 6 * 64 * 4 + (n * n + 2 * n + T * T + 2 * T) * 4
    return (b + 15) // 16 * 16


def gain_path(season, lds_per_block):
    """'lds' or 'global': where the library counts the gain histogram on a device with lds_per_block bytes of LDS per
    block (mcgp_run_championship: in LDS when the block then still takes no more than half of it)."""
    team, T = team_of(season)
    n = len(team)
    G = sum(max(list(p[3][:n]) + [0]) for p in season['plan'])
    return 'lds' if rank_lds_bytes(n, T, team_layout(season)[1], G + 1, True) <= lds_per_block // 2 else 'global'


def pairs(n):
    return [i // 2 for i in range(n)]


def big_team(n=32):
    """One team of n - 2 and two single-driver teams (the last two drivers, close on pace): the two contest second
    place among themselves."""
    return [0] * (n - 2) + [1, 2]


def team_seasons_words():
    return {k: v[1] for k, v in team_seasons().items()}


# name: (season, its team words).  Tie-rich seasons, so that team compares go deep.
def team_seasons():
    n = 32
    return {
        # 30 drivers x 27 = 810 carried-in finishes in one position (+ 4 races: 10-bit counts) and 30 x 65 000 points
        # (21 bits): 21 + 10 x 32 = 341 bits.  The 10-bit count fields of positions 26, 20, 13 and 7 straddle a word with
        # 4, 8, 2 and 6 bits in the lower one: the carried-in counts sit in the last two, so the single-driver teams'
        # counts there (27 to 31) need both pieces
        'six_words': (tie_rich(n, team=big_team(n), points=65000, counts={12: 27, 6: 27, n - 1: 26}), 6),
        'one_team_32': (tie_rich(n, team=[0] * n), 5),                 # 32 x 15 + 4: 9-bit counts, 21-bit points: 309 bits
        'pairs_32': (tie_rich(n, team=pairs(n)), 4),                   # 2 x 15 + 4: 6-bit counts, 17-bit points: 209 bits
        'singletons_32': (tie_rich(n, team=list(range(n))), 3),        # 5-bit counts, 16-bit points: 176 bits
        'one_team_20': (tie_rich(20, team=[0] * 20), 4),               # 20 x 15 + 4: 9-bit counts, 20-bit points: 200 bits
        'pairs_20': (tie_rich(20, team=pairs(20)), 3),                 # 6-bit counts, 17-bit points: 137 bits
        # every second pair carries in 500 points less: the order of the teams' totals (80 0xx against 79 0xx) is not the
        # order of their low bits, so a points field cut short ranks them wrongly
        'uneven_pairs_20': (tie_rich(20, team=pairs(20), points=[40000 - 250 * (i // 2 % 2) for i in range(20)]), 3),
        'singletons_9': (tie_rich(9, team=list(range(9))), 1),         # no carried-in counts: 3-bit counts, 16 + 27 bits
        'quads_27': (tie_rich(27, team=[i // 4 for i in range(27)]), 4),   # 4 x 15 + 4: 7-bit counts, 18-bit points: 207 bits
    }


def team_points_borrow(n=20):
    """Pairs whose totals start 4 short of 2^16 (32 766 a driver), tie-rich: within two races the leading team is past
    65 536 with rivals still below it and within the bound, so lead - points borrows across bit 16 of a 17-bit points
    field -- and across the word boundary, since the field starts at bit 120 (6-bit counts x 20) and has its 8 low
    bits in the lower word.  The seasons of team_seasons() carry in 40 000 a driver: their teams' totals, level to
    within a few points, never lie on two sides of such a boundary, and there a points field read short gives the
    same difference as the whole one."""
    return tie_rich(n, team=pairs(n), points=(1 << 15) - 2)


# ------------------------------------------------------------------------------------------------ the reference
_orders = {}


def oracle_orders(season):
    """The CPU oracle's finishing orders [sims][n] of every race of the season (kept: several tests share a season)."""
    key = json.dumps([season['case'], [p[1:3] for p in season['plan']], season['n_sims'], season['sim_offset']],
                     sort_keys=True)
    if key not in _orders:
        prob = O.Problem(season['case'])
        out = []
        for case, seed, dev, _, _ in season['plan']:
            assert case is season['case']
            rng = O.RNG_PHILOX53 if dev == 53 else O.RNG_PHILOX
            out.append(prob.run(season['n_sims'], rng=rng, seed=seed, sim_offset=season['sim_offset'],
                                want_orders=True)['orders'])
        _orders[key] = out
    return list(_orders[key])


def reference_standings(season, orders):
    """(points [s][n], counts [s][n][n], team points [s][T], team counts [s][T][n]) by championship_ref."""
    ip, ic = standings_arrays(season)
    pts, cnt = CR.standings(orders, [p[3] for p in season['plan']], [int(p[4]) for p in season['plan']], ip, ic)
    team, T = team_of(season)
    tp, tc = CR.team_standings(pts, cnt, team, T)
    return pts, cnt, tp, tc


# ------------------------------------------------------------------------------------------------ edges reached
def assert_tie_rich_edges(n, pts, cnt, init_points):
    """The tie-rich season of n cars reached the word boundaries of its driver keys."""
    if n >= 13:         # the count field at bit 60 carried out of its 4 low bits in at least 100 keys, and not in others
        c = cnt[:, :, n - 13]
        assert (c >= 16).sum() >= 100 and (c == 15).sum() >= 100, ((c >= 16).sum(), (c == 15).sum())
    if n >= 26:         # ... the one at bit 125 out of its 3 low bits
        c = cnt[:, :, n - 26]
        assert (c >= 8).sum() >= 100 and (c == 7).sum() >= 100, ((c >= 8).sum(), (c == 7).sum())
    low = points_low_bits(n)
    if low:             # the points field: read in two pieces with a non-zero upper piece; its lower piece carried
        assert ((pts >> low) > 0).all()
        carried = (pts >> low) != (np.asarray(init_points)[None, :] >> low)
        assert carried.sum() >= 100 and (~carried).sum() >= 100, (carried.sum(), (~carried).sum())
    if n >= 8:          # adjacent entrants of the final ranking decided at every field from the points to position n - 2
        depth = CR.decision_depth(pts, cnt)
        assert (depth[:n - 1] > 0).all(), depth


def assert_procession_edges(pts, cnt):
    """Driver 0 ends at least 100 seasons on exactly 31 wins and exactly 65 535 points."""
    both = (cnt[:, 0, 0] == MAX_COUNT) & (pts[:, 0] == MAX_POINTS)
    assert both.sum() >= 100, both.sum()


def assert_team_edges(name, season, tp, tc):
    """The team standings of a season of team_seasons() go where its layout is delicate."""
    team, T = team_of(season)
    n = len(team)
    cbits, words = team_layout(season)
    assert words == team_seasons_words()[name], (name, cbits, words)
    # the widest fields are needed: a count field one bit narrower would not hold the largest count, and the points
    # field holds a total within its top bit
    assert int(tc.max()) >> (cbits - 1) == 1, (tc.max(), cbits)
    if T == 1:
        return
    pos = CR.rank(tp, tc)
    depth = CR.decision_depth(tp, tc, pos)
    if name == 'six_words':
        # the two single-driver teams finish in both orders, and what separates them lies in the count fields
        a, b = int((pos[:, 1] < pos[:, 2]).sum()), int((pos[:, 2] < pos[:, 1]).sum())
        assert a >= 100 and b >= 100, (a, b)
        assert (depth[1:n] > 0).sum() >= 15, depth
    else:
        # adjacent teams are told apart by the points and by each of the first eight count fields
        assert (depth[:min(9, n - 1)] > 0).all(), depth


# ------------------------------------------------------------------------------------------------ by round
def season_args(season):
    """(tables, countback, team, T, initial points, initial counts) as championship_rounds_ref takes them."""
    team, T = team_of(season)
    ip, ic = standings_arrays(season)
    return [p[3] for p in season['plan']], [int(p[4]) for p in season['plan']], team, T, ip, ic


_rounds = {}


def reference_rounds(season):
    """championship_rounds_ref.per_simulation of the season on the oracle's orders (kept, like the orders; read only)."""
    key = json.dumps([season['case'], [p[1:] for p in season['plan']], season['standings'], season['n_sims'],
                      season['sim_offset']], sort_keys=True)
    if key not in _rounds:
        _rounds[key] = RR.per_simulation(oracle_orders(season), *season_args(season))
    return _rounds[key]


def assert_uneven_team_edges(per):
    """uneven_teams() tells a team's own bound B_r(e) from any other team's.  Over the rows before the last, among the
    non-leading teams: those exactly on their own bound, and the in-or-out decisions that come out differently when the
    bound is the leader's, the round's largest, the round's smallest.  Measured on the CPU oracle: 151, 899, 916 and
    262, with some but not all team titles secure in rows 2, 3 and 4."""
    sizes = {tuple(int(b) for b in s['B']) for s in per[:-1]}
    assert all(len(set(b)) > 1 for b in sizes), sizes                      # the bounds differ within every such row
    on = by_leader = by_largest = by_smallest = 0
    for s in per[:-1]:
        lead = s['tp'].max(axis=1)
        gap = lead[:, None] - s['tp']
        non = s['tpos'] != 0
        leader = np.argmax(s['tpos'] == 0, axis=1)
        own = gap <= s['B'][None, :]
        assert np.array_equal(own | ~non, s['tcontend'])
        on += int(((gap == s['B'][None, :]) & non).sum())
        by_leader += int(((own != (gap <= s['B'][leader][:, None])) & non).sum())
        by_largest += int(((own != (gap <= s['B'].max())) & non).sum())
        by_smallest += int(((own != (gap <= s['B'].min())) & non).sum())
    e = dict(on_own_bound=on, differ_under_leaders_bound=by_leader, differ_under_largest_bound=by_largest,
             differ_under_smallest_bound=by_smallest)
    assert min(e.values()) >= 50, e
    n_sims = len(per[0]['tp'])
    assert sum(0 < int(s['tsecure'].sum()) < n_sims for s in per) >= 3, 'three partly decided rounds'
    return e


def assert_duel_edges(per):
    """procession_duel(n): in at least 100 seasons driver 1 is in contention through row 20 and out from row 21, sits
    exactly on the bound M_20 = 250 behind the leading driver 0 in row 20, and driver 0 ends on 65 535 points; in those
    seasons both points fields of row 20 have bit 15 set.  Measured on the CPU oracle: all 200 seasons, at 20 and at
    32 cars."""
    assert len(per) == 31
    inside = np.array([s['contend'][:, 1] for s in per])
    through = inside[:DUEL_ROW + 1].all(axis=0) & ~inside[DUEL_ROW + 1:].any(axis=0)
    s = per[DUEL_ROW]
    assert s['M'] == 25 * (30 - DUEL_ROW)
    on = (s['pos'][:, 0] == 0) & (s['pts'][:, 0] - s['pts'][:, 1] == s['M'])
    all_three = through & on & (per[-1]['pts'][:, 0] == MAX_POINTS)
    assert all_three.sum() >= 100, (through.sum(), on.sum(), all_three.sum())
    assert ((s['pts'][all_three][:, :2] >> 15) == 1).all()
    return int(all_three.sum())


def assert_team_round_edges(name, season, per):
    """What the by-round kernel alone reads of a team key, the points field above n count fields, matters in the team
    seasons: in some row before the last the leading team's total needs the top bit of the layout's points field, and
    it exceeds 65 535 wherever that field is wider than 16 bits, so a read cut to 16 bits or to one word changes
    lead - points.  uneven_pairs_20 and quads_27: some non-leading team is in contention in some simulations of a row
    and out in others."""
    cbits, words = team_layout(season)
    assert words == team_seasons_words()[name]
    pbits = team_points_bits(season)
    assert (pbits + cbits * len(team_of(season)[0]) + 63) // 64 == words
    leads = [s['tp'].max(axis=1) for s in per]
    for s, lead in zip(per, leads):
        assert np.array_equal(lead, (s['tp'] * (s['tpos'] == 0)).sum(axis=1))
    assert any(((lead >> (pbits - 1)) == 1).any() for lead in leads[:-1]), pbits
    if pbits > 16:
        assert all((lead > MAX_POINTS).all() for lead in leads), pbits
    if name in ('uneven_pairs_20', 'quads_27'):
        mixed = 0
        for s in per[:-1]:
            non = s['tpos'] != 0
            inside, outside = (s['tcontend'] & non).sum(axis=0), (~s['tcontend'] & non).sum(axis=0)
            mixed += int(((inside > 0) & (outside > 0)).sum())
        assert mixed >= 1, name
    return pbits


def assert_team_borrow_edges(season, per):
    """team_points_borrow(): the team points field is wider than 16 bits and straddles a word, and over the rows before
    the last at least 50 non-leading teams are in contention with a total below 2^16 under a leader at or above it:
    the difference of the two fields' low 16 bits, or of their pieces in the lower word, is not lead - points.
    Measured on the CPU oracle: 882, 3603, 3905 and 637 such cells in rows 0 to 3."""
    cbits, words = team_layout(season)
    pbits, off = team_points_bits(season), cbits * len(team_of(season)[0])
    low = 64 - off % 64
    assert pbits > 16 and 0 < low < pbits and low <= 16, (pbits, off)
    across = 0
    for s in per[:-1]:
        lead = s['tp'].max(axis=1)[:, None]
        hit = s['tcontend'] & (s['tpos'] != 0) & (lead >= 1 << 16) & (s['tp'] < 1 << 16)
        assert ((lead - s['tp'])[hit] <= s['B'][None, :].repeat(len(lead), 0)[hit]).all()
        assert (((lead & 0xFFFF) < (s['tp'] & 0xFFFF)) | ~hit).all() and (((lead >> low) != (s['tp'] >> low)) | ~hit).all()
        across += int(hit.sum())
    assert across >= 50, across
    return across


def assert_long_calendar_rounds(per, n_sims):
    """64 rows, M falling to 0, and the drivers' title secure in some but not all seasons in at least three rows."""
    assert len(per) == 64 and per[0]['M'] > per[32]['M'] > per[62]['M'] > per[63]['M'] == 0
    assert sum(0 < int(s['secure'].sum()) < n_sims for s in per) >= 3


def assert_some_in_some_out(s):
    """One row of per_simulation: among the non-leaders, drivers and teams, some are in contention and some are out."""
    for pos, con in ((s['pos'], s['contend']), (s['tpos'], s['tcontend'])):
        non = pos != 0
        assert (con & non).sum() >= 100 and (~con & non).sum() >= 100, ((con & non).sum(), (~con & non).sum())


def tail_bytes(n, n_sims):
    """Bytes of the last tile's orders past its whole 32-bit words: champ_accumulate and race_matchups copy these one
    by one (tiles of 256 simulations, n bytes each)."""
    return (n_sims % 256) * n % 4


# ------------------------------------------------------------------------------------------------ gain paths, tails
def gain_seasons():
    """name: (season, the gain histogram's path on any device with 64 to 160 KiB of LDS per block)."""
    return {
        # G = 6: 5 x 7 cells
        'small_in_lds': (tie_rich(5, races=2), 'lds'),
        # G = 40 000: 5 x 40 001 x 4 bytes = 800 KB of cells, and 2.5 MB at 32 cars: global atomics whatever the LDS
        'wide_global': (tie_rich(5, races=2, table=[20000, 2, 1], points=25000, countback=[True, True]), 'global'),
        'wide_global_32': (tie_rich(32, races=1, table=[20000, 2, 1], points=45000, countback=[True]), 'global'),
    }


def tail_season(n, n_sims):
    """Tie-rich, with a table that pays every position: a wrong byte at the end of a finishing order moves points."""
    return tie_rich(n, n_sims=n_sims, races=3, table=list(range(n, 0, -1)), countback=[True, True, False])
