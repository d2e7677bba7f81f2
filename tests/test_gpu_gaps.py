"""Race time gaps on the GPU (mcgp_run_gaps / RaceSimulator.run_gaps): every count equals, cell for cell, what the numpy
restatement (gaps_ref) derives from the CPU oracle's per-lap trace of the same simulations -- the first comparison of a
TIME computed on the device with the oracle's, not only of the orders times produce.  From the grid and from mid-race
states; coverage conditions asserted from the reference before comparing, so that equality is not vacuous; split, shard
and staging-chunk invariance; consistency at 10^6 simulations with mcgp_run_trace; the CLI.  All comparisons are integer
equality."""
import dataclasses
import json

import numpy as np
import pytest

import gaps_ref as GR
import oracle_py as O
import resume_ref as RR
import trace_ref as TR
from helpers import product_run
from monte_carlo_gp_amd import DEFAULT_GAP_EDGES, RaceConfig, RaceSimulator, cli, _native as N
from monte_carlo_gp_amd.predictor import F1Predictor
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP

pytestmark = pytest.mark.gpu

KEYS = ('hist', 'lap_gap', 'lead', 'pair')
B = len(GR.DEFAULT_EDGES) + 1
# per golden case two drivers whose finishing row, in the reference at 512 simulations and seed 7, shows both orders and
# the retired column (asserted below); on N10 driver 1 never finishes ahead of driver 0 there
PAIR = {'S60': (0, 1), 'S78': (0, 1), 'N10': (2, 3), 'HET': (0, 1), 'EVT': (0, 1), 'DMP': (0, 1), 'WET': (0, 1)}


def _equal(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        bad = np.argwhere(a[k] != b[k])
        assert bad.size == 0, (what, k, bad[:5].tolist(), a[k][tuple(bad[0])], b[k][tuple(bad[0])])


def _err():
    return N.lib().mcgp_last_error()


# ---------------------------------------------------------------- from the grid
@pytest.mark.parametrize('name,m,offset', [('S60', 1024, 0), ('S78', 512, 0), ('N10', 1024, 0), ('HET', 512, 0),
                                           ('EVT', 1024, 0), ('DMP', 512, 0), ('WET', 512, 12345)])
def test_golden_cases_equal_the_oracle_times(require_gpu, name, m, offset):
    case = O.load_case(name)
    a, b = PAIR[name]
    pairs = [(a, b), (b, a)]
    ref512 = GR.gap_counts(case, 512, seed=7, pairs=[(a, b)])
    row = ref512['pair'][-1, 0]
    assert row[:B].sum() > 0 and row[B:2 * B].sum() > 0 and row[2 * B] > 0, (name, row.tolist())
    if name == 'S60':
        assert (int(row[:B].sum()), int(row[B:2 * B].sum()), int(row[2 * B])) == (304, 155, 53)
    ref = GR.gap_counts(case, m, seed=7, sim_offset=offset, pairs=pairs)
    # coverage (a cap, not a measurement): no empty column where the issue names one
    if name == 'S60':
        assert ref['lap_gap'][-1].sum(axis=0).tolist() == [1044, 44, 250, 829, 1099, 1211, 1215, 2144, 1545, 2303, 2321,
                                                           2034, 2207, 811, 268, 1155]
    if name == 'N10':
        assert ref['lead'][-1].tolist() == [1, 3, 8, 16, 33, 36, 27, 100, 84, 132, 204, 122, 105, 56, 95, 2]
    rc, got = GR.run_c(case, m, seed=7, sim_offset=offset, pairs=pairs)
    assert rc == 0, _err()
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_gaps_kernel'
    _equal(got, ref, name)
    hist, _, _ = product_run(case, m, 7, sim_offset=offset)              # the histogram is mcgp_run's
    assert np.array_equal(got['hist'], hist)


@pytest.mark.parametrize('n', [1, 2, 32])
def test_synthetic_fields_equal_the_oracle_times(require_gpu, n):
    case = RR.field_case(n)
    pairs = [(0, n - 1), (n - 1, 0)] if n > 1 else []
    rc, got = GR.run_c(case, 512, seed=3, pairs=pairs)
    assert rc == 0, _err()
    _equal(got, GR.gap_counts(case, 512, seed=3, pairs=pairs), f'n={n}')


def test_edge_counts_at_the_limits(require_gpu):
    """1 edge and 63 edges with 64 pairs: the widest rows the counting kernel takes (129 values)."""
    case = O.load_case('S60')
    fine = tuple(float(x) for x in np.concatenate([np.arange(1, 41) * 0.25, np.arange(1, 24) * 5.0 + 10.0]))
    pairs = [(a, b) for a in range(8) for b in range(8) if a < b] + [(b, a) for a in range(8) for b in range(8) if a < b]
    pairs += [(19, 0), (0, 19), (18, 19), (19, 18), (10, 12), (12, 10), (5, 15), (15, 5)]
    assert len(fine) == 63 and len(pairs) == 64
    ref = RR.traced_run(case, 512, 7)
    for edges, prs in (((4.0,), pairs[:2]), (fine, pairs), (fine, [])):
        rc, got = GR.run_c(case, 512, seed=7, edges=edges, pairs=prs)
        assert rc == 0, _err()
        _equal(got, GR.gap_counts(case, 512, seed=7, edges=edges, pairs=prs, ref=ref), (len(edges), len(prs)))


# ---------------------------------------------------------------- from a state
def test_oracle_states_continue_into_the_oracle_trace(require_gpu):
    """Oracle states continued as their own simulation: rows k + 1 .. L equal the oracle trace's, earlier rows stay as
    passed, the histogram is mcgp_run_from_state's."""
    total = with_dd = 0
    for name in ('S60', 'EVT', 'N10', 'WET'):
        case = O.load_case(name)
        L, seed, base = case['config']['total_laps'], 11, 500
        a, b = PAIR[name]
        pairs = [(a, b), (b, a)]
        ref = RR.traced_run(case, 6, seed, base)
        prob = RR.problem(case)
        for i in range(6):
            e = RR.first_event_lap(case, seed, base + i)
            for k in sorted({1, L // 2, L - 1, L} | ({e} if e is not None else set())):
                dd = RR.drs_disabled_until(case, seed, base + i, k)
                st = (RR.state_arrays(ref, i, k), k, dd)
                rc, got = GR.run_c(case, 1, seed, sim_offset=base + i, pairs=pairs, state=st, prob=prob)
                assert rc == 0, _err()
                _equal(got, GR.continued_counts(ref, [i], k, pairs=pairs), (name, i, k))
                rc, hist, _ = RR.run_c(prob, [st], 1, [base + i], seed, orders=False)
                assert rc == 0 and np.array_equal(got['hist'], hist[0])
                total += 1
                with_dd += dd > 0
    assert total >= 16 and with_dd >= 1


def test_one_state_continued_as_many_equals_the_restatement(require_gpu):
    case = O.load_case('S60')
    seed, k, m = 13, 31, 256
    ref = RR.traced_run(case, 3, seed)
    st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, seed, 2, k))
    pairs = [(0, 1), (1, 0), (3, 7)]
    want = GR.restated_counts(case, m, seed, sim_offset=1000, state=st, pairs=pairs)
    assert (want['lap_gap'][k:].sum(axis=2) == m).all() and not want['lap_gap'][:k].any()
    assert (want['lap_gap'][-1].sum(axis=0) > 0).sum() >= 12         # the futures spread over the bins
    into = {key: np.full_like(v, 5, dtype=np.uint64) for key, v in want.items()}
    rc, got = GR.run_c(case, m, seed, sim_offset=1000, pairs=pairs, state=st, into=into)
    assert rc == 0, _err()
    for key in ('lap_gap', 'lead', 'pair'):
        assert (got[key][:k] == 5).all(), key                         # earlier laps: as the caller passed them
    _equal({key: v - 5 for key, v in got.items()}, want, 'many from one')
    rc, hist, _ = RR.run_c(RR.problem(case), [st], m, [1000], seed, orders=False)
    assert rc == 0 and np.array_equal(got['hist'] - 5, hist[0])


# ---------------------------------------------------------------- invariance
def _sum(a, b):
    return {k: a[k] + b[k] for k in KEYS}


def test_split_and_shards_equal_one_call_across_chunks(require_gpu):
    case = O.load_case('S60')
    pairs = [(0, 1), (1, 0)]
    rc, _ = GR.run_c(case, 10 ** 6, seed=9, pairs=pairs)             # a full launch: the device's round
    assert rc == 0, _err()
    chunk = GR.chunk_sims(20, 60, 2, TR.device_round())
    assert GR.budget_sims(20, 60, 2) == (512 << 20) // (60 * 23) // 256 * 256 and 2 * chunk < 10 ** 6
    N_ = chunk + 70001                                # one call crosses a chunk boundary, the halves do not
    rc, whole = GR.run_c(case, N_, seed=9, sim_offset=100, pairs=pairs)
    assert rc == 0, _err()
    h = N_ // 2
    rc1, a = GR.run_c(case, h, seed=9, sim_offset=100, pairs=pairs)
    rc2, b = GR.run_c(case, N_ - h, seed=9, sim_offset=100 + h, pairs=pairs)
    assert rc1 == rc2 == 0
    _equal(whole, _sum(a, b), 'split')
    # two-device-style shards through the simulator surface: device [0, 0] shards by offset
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    names = list(case['grid_probs'])
    named = [(names[0], names[1]), (names[1], names[0])]
    one = RaceSimulator(RaceConfig(**case['config']), device=0, set_pop=RR.SET_POP).run_gaps(
        30001, *args, pairs=named, seed=9, sim_offset=100)
    two = RaceSimulator(RaceConfig(**case['config']), device=[0, 0], set_pop=RR.SET_POP).run_gaps(
        30001, *args, pairs=named, seed=9, sim_offset=100)
    rc, direct = GR.run_c(case, 30001, seed=9, sim_offset=100, pairs=pairs)
    assert rc == 0
    for k in KEYS:
        assert np.array_equal(getattr(one, k), getattr(two, k)) and np.array_equal(getattr(one, k), direct[k]), k


def test_from_a_state_across_chunks(require_gpu):
    """A resumed run records L - k laps, so its chunk is larger; a call crossing it equals its halves."""
    case = O.load_case('N10')
    L, seed, k = case['config']['total_laps'], 4, 60
    ref = RR.traced_run(case, 1, seed)
    st = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, 0, k))
    rc, _ = GR.run_c(case, 10 ** 6, seed, state=st)
    assert rc == 0, _err()
    chunk = GR.chunk_sims(10, L - k, 0, TR.device_round())
    N_ = chunk + 5003
    rc, whole = GR.run_c(case, N_, seed, state=st)
    rc1, a = GR.run_c(case, chunk - 11, seed, state=st)
    rc2, b = GR.run_c(case, N_ - (chunk - 11), seed, sim_offset=chunk - 11, state=st)
    assert rc == rc1 == rc2 == 0
    _equal(whole, _sum(a, b), 'state split')
    assert (whole['lap_gap'][k:].sum(axis=2) == N_).all() and not whole['lap_gap'][:k].any()


# ---------------------------------------------------------------- consistency at a million
def test_consistency_at_a_million(require_gpu):
    case = O.load_case('S60')
    N_, n, L = 10 ** 6, 20, 60
    pairs = [(0, 1), (1, 0), (4, 17), (17, 4)]
    rc, g = GR.run_c(case, N_, seed=21, pairs=pairs)
    assert rc == 0, _err()
    rc, t = TR.run_c(case, N_, seed=21)
    assert rc == 0, _err()
    assert np.array_equal(g['hist'], t['hist'])
    assert (g['lap_gap'].sum(axis=2) == N_).all()
    assert np.array_equal(g['lap_gap'][:, :, B], t['lap_pos'][:, :, n])          # retired is retired
    assert (g['lap_gap'][:, :, 0] >= t['lap_pos'][:, :, 0]).all()                # the leader is in bin 0
    assert (g['lead'].sum(axis=1) == N_).all()
    assert (np.diff(g['lead'][:, B]) >= 0).all()                                 # the number of runners only falls
    assert (g['pair'].sum(axis=2) == N_).all()
    for p in (0, 2):                                                             # (a, b) and (b, a) mirror each other
        assert np.array_equal(g['pair'][:, p, :B], g['pair'][:, p + 1, B:2 * B])
        assert np.array_equal(g['pair'][:, p, B:2 * B], g['pair'][:, p + 1, :B])
        assert np.array_equal(g['pair'][:, p, 2 * B], g['pair'][:, p + 1, 2 * B])
    # the second car's own gap is the lead: in every bin, as many seconds as leads
    assert np.array_equal(g['lead'][:, :B].sum(axis=1), t['lap_pos'][:, :, 1].sum(axis=1))
    # the run spans at least 2 staging chunks of the documented rule
    assert GR.budget_sims(n, L, 4) == (512 << 20) // (60 * 25) // 256 * 256
    assert 2 * GR.chunk_sims(n, L, 4, TR.device_round()) <= N_


# ---------------------------------------------------------------- the surface and the CLI
def test_simulator_surface_and_optional_outputs(require_gpu):
    case = O.load_case('EVT')
    names = list(case['grid_probs'])
    rc, full = GR.run_c(case, 4000, seed=2, pairs=[(0, 1)])
    rc2, part = GR.run_c(case, 4000, seed=2, lead=False)
    assert rc == rc2 == 0
    assert np.array_equal(full['lap_gap'], part['lap_gap']) and not part['lead'].any()
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=RR.SET_POP)
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    res = sim.run_gaps(4000, *args, pairs=[(names[0], names[1])], seed=2, track_condition=case['track_condition'])
    for k in KEYS:
        assert np.array_equal(getattr(res, k), full[k]), k
    assert np.array_equal(sim.last_histogram, res.hist) and res.first_lap == 1
    probs = sim.run_monte_carlo(4000, *args, seed=2, track_condition=case['track_condition'])
    assert res.position_probabilities == probs
    assert res.within(names[0], 5.0) == full['lap_gap'][-1, 0, :5].sum() / 4000
    import ctypes as C
    f = C.c_float()
    assert N.lib().mcgp_last_kernel_ms(0, C.byref(f)) == 0 and f.value > 0


def _cli_case():
    inp = F1Predictor().simulator_inputs(cli.synthetic_fixture(), 'Bahrain')
    cfg = dataclasses.asdict(inp['config'])
    return dict(config=cfg, grid_probs=inp['grid_probs'], base_pace=inp['base_pace'], tire_deg=inp['tire_deg'],
                driver_variance=inp['driver_variance'], driver_dnf_rates=inp['driver_dnf_rates'],
                track_condition=inp['track_condition'])


def test_cli_gaps_end_to_end(require_gpu, tmp_path, capsys):
    """predict --gaps and in-race --gaps on the offline fixture: the probabilities are reference counts / N."""
    case = _cli_case()
    drivers = list(case['grid_probs'])
    m, seed = 2000, 5
    a, b = drivers[0], drivers[1]
    ref_run = O.Problem(case, set_pop=DEFAULT_SET_POP).run(m, rng=O.RNG_PHILOX, seed=seed, want_orders=True,
                                                           want_grids=True, n_trace=m)
    ref = GR.gap_counts(case, m, seed, pairs=[(0, 1)], ref=ref_run)
    out = tmp_path / 'gaps.json'
    assert cli.main(['predict', '--race', 'Bahrain', '--season', '2024', '--offline', '--simulations', str(m), '--seed',
                     str(seed), '--gaps', '--gap-pair', f'{a}:{b}', '--json', str(out)]) == 0
    text = capsys.readouterr().out
    for title in ('WINNING MARGIN', 'WITHIN OF THE WINNER AT THE FLAG', 'PAIR GAPS AT THE FLAG', '< 1 s', '< 5 s', '< 20 s'):
        assert title in text, title
    g = json.loads(out.read_text())['gaps']
    edges = [float(x) for x in DEFAULT_GAP_EDGES]
    assert g['edges'] == edges and g['winning_margin'] == (ref['lead'][-1] / m).tolist()
    for i, d in enumerate(drivers):
        assert g['finishing_gap'][d] == (ref['lap_gap'][-1, i] / m).tolist(), d
        for j, e in enumerate(edges):
            assert g['within_at_flag'][d][str(e)] == ref['lap_gap'][-1, i, :j + 1].sum() / m
    pr = g['pairs'][0]
    row = ref['pair'][-1, 0]
    assert (pr['a'], pr['b']) == (a, b)
    assert (pr['a_ahead'], pr['b_ahead'], pr['either_out']) == (row[:B].sum() / m, row[B:2 * B].sum() / m, row[2 * B] / m)
    assert pr['within_by_lap']['1.0'] == ((ref['pair'][:, 0, :2].sum(axis=1) + ref['pair'][:, 0, B:B + 2].sum(axis=1)) / m).tolist()
    assert f"{a:4} ahead {pr['a_ahead']:6.1%}" in text
    # in-race: simulation 0's state after lap 30 continued as 1 simulation is the oracle's trace of simulation 0
    k = 30
    state = RR.race_state(RR.state_arrays(ref_run, 0, k), k, RR.drs_disabled_until(case, seed, 0, k), drivers)
    path, out2 = tmp_path / 'lap30.json', tmp_path / 'inrace.json'
    path.write_text(json.dumps(state.to_json()))
    assert cli.main(['in-race', '--race', 'Bahrain', '--season', '2024', '--offline', '--state', str(path),
                     '--simulations', '1', '--seed', str(seed), '--gaps', '--gap-pair', f'{a}:{b}', '--json', str(out2)]) == 0
    text = capsys.readouterr().out
    assert 'WINNING MARGIN' in text and 'PAIR GAPS AT THE FLAG' in text
    g = json.loads(out2.read_text())[0]['gaps']
    want = GR.continued_counts(ref_run, [0], k, pairs=[(0, 1)])
    assert g['first_lap'] == k + 1 and g['winning_margin'] == want['lead'][-1].astype(float).tolist()
    for i, d in enumerate(drivers):
        assert g['finishing_gap'][d] == want['lap_gap'][-1, i].astype(float).tolist(), d
    row = want['pair'][-1, 0]
    assert (g['pairs'][0]['a_ahead'], g['pairs'][0]['b_ahead'], g['pairs'][0]['either_out']) == (
        float(row[:B].sum()), float(row[B:2 * B].sum()), float(row[2 * B]))
