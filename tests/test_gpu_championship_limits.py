"""mcgp_run_championship at the limits of its key layout: word boundaries, field limits, wide team keys, both paths of
the gain histogram, the staging copy's byte tail, grid-striding with 3-word keys.  Every histogram equals
championship_ref fed with the CPU oracle's finishing orders, count for count; no tolerance anywhere.

The seasons come from championship_cases.py.  Each test first proves FROM THE REFERENCE ALONE that its season reached
the edge it is there for (the same assertions run without a device in test_championship_host.py), then compares.
"""
import numpy as np
import pytest

import championship_cases as CC
import championship_ref as CR
import oracle_py as O
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, run_championship
from test_gpu_championship import _check, _race

pytestmark = pytest.mark.gpu

SET_POP = O.load_cases()['set_pop']


def _run(season):
    races = [_race(case, seed, points=table, countback=cb) for case, seed, _, table, cb in season['plan']]
    return run_championship(races, season['n_sims'], standings=season['standings'], sim_offset=season['sim_offset'],
                            set_pop=SET_POP, return_race_histograms=True)


def _compare(season, orders):
    res = _run(season)
    _check(res, {}, season['plan'], season['n_sims'], season['sim_offset'], season['standings'], orders=orders)
    return res


@pytest.mark.parametrize('n', list(range(1, 33)))
def test_tie_rich_standings_at_every_field_size(require_gpu, n):
    """Equal carried-in points (with a lower piece about to carry where the points field straddles a word: n = 10, 11,
    12, 23, 24, 25), counts of 15 and 7 in the count fields at bits 60 and 125, a three-place table: keys carry out of
    every straddling field, and the ranking is decided in every field from the points to position n - 2."""
    season = CC.tie_rich(n)
    orders = CC.oracle_orders(season)
    pts, cnt, _, _ = CC.reference_standings(season, orders)
    CC.assert_tie_rich_edges(n, pts, cnt, CC.standings_arrays(season)[0])
    _compare(season, orders)


@pytest.mark.parametrize('n', [20, 32])
def test_procession_reaches_31_wins_and_65535_points(require_gpu, n):
    season = CC.procession(n)
    orders = CC.oracle_orders(season)
    pts, cnt, _, _ = CC.reference_standings(season, orders)
    CC.assert_procession_edges(pts, cnt)
    _compare(season, orders)


def test_calendar_of_64_races(require_gpu):
    """The most races a call takes: 31 that count back and 33 sprints."""
    season = CC.long_calendar()
    assert len(season['plan']) == 64 and sum(p[4] for p in season['plan']) == 31
    orders = CC.oracle_orders(season)
    pts, cnt, _, _ = CC.reference_standings(season, orders)
    assert cnt.sum(axis=2).max() == 31 and len(np.unique(pts)) > 100
    _compare(season, orders)


@pytest.mark.parametrize('name', list(CC.team_seasons()))
def test_team_layouts(require_gpu, name):
    """Team keys of 1, 3, 4, 5 and 6 words (one team, singletons, pairs, fours, a team of 30 beside two contested
    singletons): count fields of up to 10 bits that straddle words, totals in the top bit of their fields."""
    season, _ = CC.team_seasons()[name]
    orders = CC.oracle_orders(season)
    _, _, tp, tc = CC.reference_standings(season, orders)
    CC.assert_team_edges(name, season, tp, tc)
    _compare(season, orders)


@pytest.mark.parametrize('name', list(CC.gain_seasons()))
def test_gain_histogram_paths(require_gpu, name):
    """The gain histogram is counted in the block's LDS when champ_rank_lds with it stays within half the device's LDS
    per block, else by global atomics.  An MI355X reports 163 840 bytes (160 KiB) per block, the value the library
    reads from the device's properties; the rule gives these seasons the same answer for any budget from 64 to 160 KiB:
    small_in_lds (5 cars, G = 6: 13 KB of LDS with the gain cells) counts in LDS; wide_global (5 cars, G = 40 000:
    800 KB of cells) and wide_global_32 (32 cars, G = 20 000: 2.5 MB) by global atomics.  In each, some driver gains
    nothing and some driver gains G: both ends of the histogram's rows are written."""
    season, path = CC.gain_seasons()[name]
    assert CC.gain_path(season, 64 * 1024) == path and CC.gain_path(season, 160 * 1024) == path
    orders = CC.oracle_orders(season)
    pts, _, _, _ = CC.reference_standings(season, orders)
    gain = pts - CC.standings_arrays(season)[0][None, :]
    G = sum(max(p[3]) for p in season['plan'])
    assert (gain == 0).sum() >= 50 and (gain == G).sum() >= 50
    res = _compare(season, orders)
    assert res.gain_hist.shape[1] == G + 1 and res.gain_hist[:, 0].sum() > 0 and res.gain_hist[:, G].sum() > 0


@pytest.mark.parametrize('n_sims', [501, 502, 503])
@pytest.mark.parametrize('n', [9, 23, 31])
def test_byte_tail_of_the_staged_orders(require_gpu, n, n_sims):
    """An odd field and a last tile whose orders end 1, 2 or 3 bytes past a whole word; every position scores, so a
    wrong byte there moves points."""
    assert CC.tail_bytes(n, n_sims) != 0
    assert sorted(CC.tail_bytes(n, k) for k in (501, 502, 503)) == [1, 2, 3]
    season = CC.tail_season(n, n_sims)
    _compare(season, CC.oracle_orders(season))


def test_grid_stride_with_three_word_keys(require_gpu):
    """23 cars (odd, 3-word keys, a straddling points field) and more simulations than champ_accumulate's largest grid
    covers in one pass (compute units x 8 blocks x 256), not a multiple of 256: both kernels grid-stride, champ_rank
    reusing its LDS histograms across tiles.  Reference orders from run_monte_carlo(return_orders=True), themselves
    pinned to the oracle; ranking by championship_ref's lexsort, in blocks."""
    import torch
    n = 23
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_sims = cus * 8 * 256 + 5 * 256 + 77
    season = CC.tie_rich(n, n_sims=n_sims, races=2, countback=[True, True], sim_offset=0)
    assert n_sims > cus * 8 * 256 and n_sims % 256 and CC.tail_bytes(n, n_sims)
    case = season['case']
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=SET_POP)
    orders = [sim.run_monte_carlo(n_sims, case['grid_probs'], case['base_pace'], case['tire_deg'],
                                  case['driver_variance'], case['driver_dnf_rates'], seed=seed,
                                  track_condition=case['track_condition'], return_orders=True)[1]
              for _, seed, _, _, _ in season['plan']]
    probe = O.Problem(case).run(2000, rng=O.RNG_PHILOX, seed=season['plan'][0][1], want_orders=True)['orders']
    assert np.array_equal(orders[0][:2000], probe)
    team, T = CC.team_of(season)
    ip, ic = CC.standings_arrays(season)
    tables, cb = [p[3] for p in season['plan']], [int(p[4]) for p in season['plan']]
    block, tot, carried = 1 << 15, None, 0
    for s0 in range(0, n_sims, block):
        part_orders = [o[s0:s0 + block] for o in orders]
        part = CR.championship(part_orders, tables, cb, team, T, init_points=ip, init_counts=ic, grouped='lexsort')
        tot = part if tot is None else tuple(a + b for a, b in zip(tot, part))
        if s0 == 0:             # the edge, proven on the first block: the count field at bit 60 carried
            pts, cnt = CR.standings(part_orders, tables, cb, ip, ic)
            carried = int((cnt[:, :, n - 13] >= 16).sum())
    assert carried >= 100
    res = _run(season)
    champ, teams, gain, races = tot
    assert np.array_equal(res.champ_hist, champ)
    assert np.array_equal(res.team_hist, teams)
    assert np.array_equal(res.gain_hist, gain)
    assert all(np.array_equal(a, b) for a, b in zip(res.race_histograms, races))
