"""Seasons that take the standings kernels to the limits of their key layout (csrc/championship.hip.h), and the proof,
from championship_ref alone, that a season got there.

TEST INFRASTRUCTURE, shared by the device tests (test_gpu_championship_limits.py), the host build of the kernels
(test_champ_host_build.py) and the builders' own tests (test_championship_host.py).  A season is a dict:
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


def rank_lds_bytes(n, T, team_words, gain_cols, gain_in_lds):
    """champ_rank_lds (csrc/championship.hip.h) restated: the rank kernel's LDS."""
    words = (16 + 5 * n + 63) // 64
    b = words * n * 64 * 8 + team_words * T * 64 * 8 + n * n * 4 + T * T * 4 + (n * gain_cols * 4 if gain_in_lds else 0)
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
