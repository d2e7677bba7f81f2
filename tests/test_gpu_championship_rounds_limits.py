"""mcgp_run_championship_rounds at the limits of its key layout: what champ_round (csrc/champ_rounds.hip.h) does and
champ_rank never does.  It reads the points field of team keys (up to 21 bits above up to 320 bits of counts, in two
pieces where it straddles a word), subtracts two points fields, indexes the teams' bounds per team, hands the leader
and the contender count from wave to wave through LDS and reuses that LDS from tile to tile.  Every count of every round
equals championship_rounds_ref fed with the CPU oracle's finishing orders, and the four season outputs equal the plain
call's; no tolerance anywhere.

The seasons come from championship_cases.py.  Each test first proves FROM THE REFERENCE ALONE that its season reached
the edge it is there for; the same seasons run after the same proofs through the host build of the kernel
(test_champ_rounds_host_build.py), and the proofs alone in test_championship_host.py.

Wall time on one MI355X, with the two other championship limit files in one pytest command: 18.7 s for the 19 tests
here, the oracle's and the reference's share included.  15.4 s of that is test_grid_stride_against_the_reference, of
which 8 s is the reference's lexsort of 65 893 simulations x 23 cars x 2 rounds and 2 s the first import of torch; no
other test takes more than 0.5 s.
"""
import ctypes as C

import numpy as np
import pytest

import championship_cases as CC
import championship_rounds_ref as RR
import oracle_py as O
from monte_carlo_gp_amd import RaceConfig, RaceSimulator
from test_gpu_championship_rounds import SET_POP, _Abi, _assert_old_outputs_equal, _compare_season, _run_season

pytestmark = pytest.mark.gpu

LDS_PER_BLOCK = 163840          # what the library reads from an MI355X's properties (160 KiB)


@pytest.mark.parametrize('name', list(CC.team_seasons()))
def test_team_layouts_by_round(require_gpu, name):
    """Team keys of 1, 3, 4, 5 and 6 words: the team points field of 16 to 21 bits, read above 27 to 320 bits of
    counts; the leading team's total needs the field's top bit and, where the field is wider than 16 bits, exceeds
    65 535."""
    season, _ = CC.team_seasons()[name]
    CC.assert_team_round_edges(name, season, CC.reference_rounds(season))
    _compare_season(season)


def test_team_points_borrow_across_bit_16_and_a_word(require_gpu):
    """Pairs that start 4 points short of 2^16: rivals below it, within the bound of a leader above it, so that
    lead - points borrows across bit 16 of the 17-bit team points field and across the word boundary inside it.  In the
    nine seasons above the teams' totals never lie on two sides of such a boundary, and a field read short gives the
    same difference there as the whole one."""
    season = CC.team_points_borrow()
    CC.assert_team_borrow_edges(season, CC.reference_rounds(season))
    _compare_season(season)


def test_uneven_team_bounds(require_gpu):
    """Teams of 3, 2, 1 and 1: team_rem is read per team.  The leader's bound, the round's largest and the round's
    smallest would each decide hundreds of cells differently."""
    season = CC.uneven_teams()
    CC.assert_uneven_team_edges(CC.reference_rounds(season))
    _compare_season(season)


@pytest.mark.parametrize('n', [20, 32])
def test_procession_duel_at_the_points_limit(require_gpu, n):
    """A leader that ends on 65 535 points, a rival 250 = M_20 behind in row 20 and out in row 21, both points fields
    with bit 15 set."""
    season = CC.procession_duel(n)
    CC.assert_duel_edges(CC.reference_rounds(season))
    res, _ = _compare_season(season)
    assert (res.contend[:21, 1] >= 100).all() and (res.contend[21:, 1] <= 100).all()


def test_calendar_of_64_races_by_round(require_gpu):
    """64 champ_round launches, 64 rows of every output, 31 races that count back."""
    season = CC.long_calendar()
    CC.assert_long_calendar_rounds(CC.reference_rounds(season), season['n_sims'])
    res, _ = _compare_season(season)
    assert res.round_hist.shape[0] == 64 and res.secure.shape[0] == 64
    assert (np.diff(res.secure, axis=0) >= 0).all()


@pytest.mark.parametrize('n_sims', [501, 502, 503])
def test_byte_tail_by_round(require_gpu, n_sims):
    """23 cars and a last tile of 53, 54 and 55 lanes behind seven full ones, the staged orders ending 1, 2 or 3 bytes
    past a word, a table that pays every position."""
    n = 23
    assert n_sims // 64 == 7 and n_sims % 64 in (53, 54, 55) and CC.tail_bytes(n, n_sims) != 0
    _compare_season(CC.tail_season(n, n_sims))


def test_grid_stride_against_the_reference(require_gpu):
    """23 cars (3-word driver and team keys, a straddling points field), two races, and more than twice the tiles
    champ_round's largest grid holds, the last one partial: every block takes several tiles through the same LDS, and
    the counts equal the reference's.  Orders from run_monte_carlo(return_orders=True), pinned to the oracle; the
    reference in blocks of 2^15 simulations."""
    import torch
    n = 23
    rng = np.random.default_rng(300 + n)
    points = [int(CC.tie_rich_points(n) - x) for x in rng.integers(0, 10, n)]
    probe = CC.tie_rich(n, races=2, countback=[True, True], sim_offset=0, points=points)
    team, T = CC.team_of(probe)
    lds = CC.round_lds_bytes(n, T, CC.team_layout(probe)[1])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    round_cap = cus * min(8, LDS_PER_BLOCK // lds)
    n_sims = 2 * round_cap * 64 + 5 * 64 + 37
    assert n_sims > round_cap * 64 and n_sims % 64 != 0
    season = CC.tie_rich(n, n_sims=n_sims, races=2, countback=[True, True], sim_offset=0, points=points)
    case = season['case']
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=SET_POP)
    orders = [sim.run_monte_carlo(n_sims, case['grid_probs'], case['base_pace'], case['tire_deg'],
                                  case['driver_variance'], case['driver_dnf_rates'], seed=seed,
                                  track_condition=case['track_condition'], return_orders=True)[1]
              for _, seed, _, _, _ in season['plan']]
    first = O.Problem(case).run(2000, rng=O.RNG_PHILOX, seed=season['plan'][0][1], want_orders=True)['orders']
    assert np.array_equal(orders[0][:2000], first)
    args = CC.season_args(season)
    block, tot = 1 << 15, None
    for s0 in range(0, n_sims, block):
        part_orders = [o[s0:s0 + block] for o in orders]
        per = RR.per_simulation(part_orders, *args)
        part = RR.rounds(part_orders, *args[:4], sims=per)
        tot = part if tot is None else {k: tot[k] + part[k] for k in RR.KEYS}
        if s0 == 0:
            CC.assert_some_in_some_out(per[0])
    res = _run_season(season)
    for k in RR.KEYS:
        assert np.array_equal(getattr(res, k), tot[k]), k
    RR.assert_identities({k: getattr(res, k) for k in RR.KEYS}, n_sims, res.champ_hist, res.team_hist)
    _assert_old_outputs_equal(res, _run_season(season, by_round=False))


class _DriversOnlyAbi(_Abi):
    """_Abi, and the call with the team trio NULL: the kernel then runs with n_teams == 0."""

    def run_drivers_only(self, arrays, n_sims, offset=0):
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        from monte_carlo_gp_amd import _native as N
        lib = N.lib()
        assert len(arrays) == 10
        rc = lib.mcgp_run_championship_rounds(self.R, self.cfgs, self.drvs, self.grids, 3, n_sims, offset, self.seeds,
                                              i32(self.points), self.cb.ctypes.data_as(C.POINTER(C.c_uint8)), i32(self.ip),
                                              None, i32(self.team), 2, 0,
                                              *[a.ctypes.data_as(C.POINTER(C.c_uint64)) for a in arrays[:7]], None, None, None)
        return rc, lib.mcgp_last_error().decode()


def test_drivers_only_on_the_device(require_gpu):
    """Without the team trio: round_hist, contend and secure equal the reference on the oracle's orders and what the
    call with teams gives; the season outputs, the teams' final histogram among them, are the same too."""
    abi = _DriversOnlyAbi()
    n_sims, offset = 1000, 5
    case = CC.field(3, laps=5, team=[0, 1, 0])
    prob = O.Problem(case)
    orders = [prob.run(n_sims, rng=O.RNG_PHILOX, seed=71 + r, sim_offset=offset, want_orders=True)['orders']
              for r in range(abi.R)]
    tables, cb, team, ip = [list(t) for t in abi.points], [int(c) for c in abi.cb], [int(t) for t in abi.team], abi.ip
    per = RR.per_simulation(orders, tables, cb, team, 2, ip)
    ref = RR.rounds(orders, tables, cb, team, 2, sims=per)
    assert 0 < ref['secure'][0].sum() < n_sims and 0 < (per[0]['contend'] & (per[0]['pos'] != 0)).sum() < 2 * n_sims
    alone, both = abi.arrays(), abi.arrays()
    rc, err = abi.run_drivers_only(alone, n_sims, offset)
    assert rc == 0, err
    assert abi.run(both, n_sims, offset)[0] == 0
    for i, k in ((4, 'round_hist'), (5, 'contend'), (6, 'secure')):
        assert np.array_equal(alone[i].astype(np.int64), ref[k]), k
    for i, k in ((7, 'team_round_hist'), (8, 'team_contend'), (9, 'team_secure')):
        assert np.array_equal(both[i].astype(np.int64), ref[k]), k
        assert not alone[i].any()
    for a, b in zip(alone[:7], both[:7]):
        assert np.array_equal(a, b)
