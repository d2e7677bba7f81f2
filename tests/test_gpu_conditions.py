"""Combination and conditional odds on the GPU (mcgp_run_conditions / RaceSimulator.run_conditions): every count and every
cell of the conditional histograms equals what the numpy restatement (conditions_ref) derives from the CPU oracle's run
of the same simulations, from the grid and from mid-race states, with and without the histograms; accumulation, split,
shard and staging-chunk invariance; identities at 10^6 simulations against the device-counted results of other entry
points (matchups, trace); the Python and CLI path.  Every compared condition is shown informative by the reference first
(met by some, not by all simulations), so no comparison is between two zero arrays.  All comparisons are integer
equality."""
import ctypes as C
import dataclasses
import json

import numpy as np
import pytest

import conditions_ref as CR
import generic_cases as G
import oracle_py as O
import resume_ref as RR
import trace_ref as TR
from helpers import product_run
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, cli, conditions as CD, _native as N
from monte_carlo_gp_amd.predictor import F1Predictor
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP

pytestmark = pytest.mark.gpu

KEYS = ('hist', 'count', 'cond_hist')
CASES = ('S60', 'EVT', 'WET', 'HET', 'N10')


def _equal(a, b, what, keys=KEYS):
    for k in keys:
        assert a[k].shape == b[k].shape, (what, k)
        bad = np.argwhere(a[k] != b[k])
        assert bad.size == 0, (what, k, bad[:5].tolist(), a[k][tuple(bad[0])], b[k][tuple(bad[0])])


def _err():
    return N.lib().mcgp_last_error()


def _conditions(facts, n, L, seed, most=61):
    """Informative simple and eight-atom conditions chosen on the reference's facts, then the empty condition, an
    always-true and an always-false bound; and the indices of those three."""
    simple = CR.pick(facts, CR.simple_candidates(n, L), most // 2)
    wide = CR.pick(facts, CR.wide_candidates(n, L, np.random.default_rng(seed), 800), most - len(simple))
    conds = simple + wide
    k = len(conds)
    return conds + [CR.EMPTY, CR.ALWAYS, CR.NEVER], (k, k + 1, k + 2)


def _lap1_corner():
    for name, case in G.fuzz_cases().items():
        if name == 'X_all_out_lap1' or len(case['grid_probs']) < 4:
            continue
        f = CR.oracle_facts(case, 64, case['seed'], 3)
        if (f['out'] == 1).sum() >= 8 and (f['out'] != 1).sum() >= 8:
            return name, case, case['seed']
    raise AssertionError('no fuzz configuration with lap-1 retirements')


def _case(name):
    if name == 'corner':
        return _lap1_corner()[1:]
    if name in CASES:
        return O.load_case(name), 42
    return RR.field_case(int(name[1:])), 5


# ---------------------------------------------------------------- from the grid
@pytest.mark.parametrize('name,m,offset', [('S60', 1024, 0), ('EVT', 1024, 0), ('WET', 512, 12345), ('HET', 512, 0),
                                           ('N10', 1024, 0), ('corner', 512, 7), ('n1', 512, 0), ('n2', 512, 0),
                                           ('n3', 512, 0), ('n22', 512, 0), ('n32', 512, 0)])
def test_counts_equal_the_reference_from_the_grid(require_gpu, name, m, offset):
    case, seed = _case(name)
    n, L = len(case['grid_probs']), case['config']['total_laps']
    ref_run = RR.traced_run(case, m, seed, offset)
    facts = CR.oracle_facts(case, m, seed, offset, ref=ref_run)
    conds, constant = _conditions(facts, n, L, seed)
    CR.assert_informative(facts, conds, constant)
    if n >= 3:
        assert len(conds) >= 30, len(conds)
    if name == 'corner':
        assert (facts['out'] == 1).any()
    want = CR.counts(facts, conds)
    assert np.array_equal(want['hist'], ref_run['hist'])
    rc, got = CR.run_c(case, conds, m, seed, sim_offset=offset)
    assert rc == 0, _err()
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_conditions_kernel'
    _equal(got, want, name)
    assert (got['cond_hist'].sum(axis=2) == got['count'][:, None]).all()
    k = constant[0]
    assert np.array_equal(got['cond_hist'][k], got['hist'])                  # the empty condition's histogram
    assert got['count'][k + 1] == m and got['count'][k + 2] == 0
    rc, only = CR.run_c(case, conds, m, seed, sim_offset=offset, cond_hist=False)      # cond_hist_out NULL
    assert rc == 0, _err()
    _equal(only, want, (name, 'counts only'), keys=('hist', 'count'))
    assert not only['cond_hist'].any()
    hist, _, _ = product_run(case, m, seed, sim_offset=offset)               # the histogram is mcgp_run's
    assert np.array_equal(got['hist'], hist)


def test_sixty_four_conditions_of_eight_atoms(require_gpu):
    case, seed, m = O.load_case('EVT'), 42, 2048
    n, L = len(case['grid_probs']), case['config']['total_laps']
    facts = CR.oracle_facts(case, m, seed)
    conds = CR.pick(facts, CR.wide_candidates(n, L, np.random.default_rng(7), 4000), 64)
    assert len(conds) == 64 and all(len(c) == 8 for c in conds)
    CR.assert_informative(facts, conds)
    assert CR.facts_used(conds) == set(CR.FACT_NAMES)
    rc, got = CR.run_c(case, conds, m, seed)
    assert rc == 0, _err()
    _equal(got, CR.counts(facts, conds), 'EVT64')


# ---------------------------------------------------------------- from a state
@pytest.mark.parametrize('name', ['S60', 'EVT', 'WET', 'HET', 'N10', 'corner', 'n1', 'n2', 'n3', 'n22', 'n32'])
def test_oracle_states_continue_into_the_oracle_facts(require_gpu, name):
    """Oracle states continued as their own simulation give that simulation's facts, events from the state's lap on; the
    histogram is mcgp_run_from_state's."""
    case, seed = _case(name)
    n, L, base = len(case['grid_probs']), case['config']['total_laps'], 500
    ref = RR.traced_run(case, 6, seed, base)
    runs = []
    for i in range(6):
        e = RR.first_event_lap(case, seed, base + i)
        for k in sorted({1, L // 2, L - 1, L} | ({e} if e is not None else set())):
            runs.append((i, k, (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k))))
    parts = [CR.oracle_facts(case, 0, seed, base, ref=ref, sims=[i], lap0=k) for i, k, _ in runs]
    facts = {key: np.concatenate([p[key] for p in parts], axis=0) for key in parts[0]}
    conds, constant = _conditions(facts, n, L, seed + 1)
    CR.assert_informative(facts, conds, constant)
    prob = RR.problem(case)
    for (i, k, st), f in zip(runs, parts):
        rc, got = CR.run_c(case, conds, 1, seed, sim_offset=base + i, state=st, prob=prob)
        assert rc == 0, _err()
        _equal(got, CR.counts(f, conds), (name, i, k))
        rc, hist, _ = RR.run_c(prob, [st], 1, [base + i], seed, orders=False)
        assert rc == 0 and np.array_equal(got['hist'], hist[0])
    assert len(runs) >= 16


def test_one_state_continued_as_many_and_accumulation(require_gpu):
    """Many simulations from one state against the wrapped Python restatement, accumulated into non-zero buffers; with and
    without the histograms."""
    case = O.load_case('S60')
    seed, k, m = 13, 31, 256
    n, L = 20, 60
    ref = RR.traced_run(case, 3, seed)
    st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, seed, 2, k))
    facts = CR.restated_facts(case, m, seed, sim_offset=1000, state=st)
    conds, constant = _conditions(facts, n, L, 3)
    CR.assert_informative(facts, conds, constant)
    assert len(conds) >= 30 and len(np.unique(facts['orders'], axis=0)) > m // 2       # the futures differ
    want = CR.counts(facts, conds)
    into = {key: np.full_like(v, 5, dtype=np.uint64) for key, v in want.items()}
    rc, got = CR.run_c(case, conds, m, seed, sim_offset=1000, state=st, into=into)
    assert rc == 0, _err()
    _equal({key: v - 5 for key, v in got.items()}, want, 'many from one')
    rc, got = CR.run_c(case, conds, m, seed, sim_offset=1000, state=st, into=into, cond_hist=False)
    assert rc == 0, _err()
    _equal({'hist': got['hist'] - 5, 'count': got['count'] - 5, 'cond_hist': got['cond_hist'] - 5},
           {'hist': 2 * want['hist'], 'count': 2 * want['count'], 'cond_hist': want['cond_hist']}, 'accumulated twice')
    rc, hist, _ = RR.run_c(RR.problem(case), [st], m, [1000], seed, orders=False)
    assert rc == 0 and np.array_equal(want['hist'], hist[0])


# ---------------------------------------------------------------- invariance
def _sum(a, b):
    return {k: a[k] + b[k] for k in KEYS}


def _named(case, facts_m=512, seed=9):
    """A set of conditions for the large runs, informative on the oracle's first simulations of the seed."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    facts = CR.oracle_facts(case, facts_m, seed, 100)
    conds, constant = _conditions(facts, n, L, 17)
    CR.assert_informative(facts, conds, constant)
    return conds


def test_any_split_sums_to_one_call(require_gpu):
    case = O.load_case('S60')
    conds = _named(case)
    total = 50001
    rc, whole = CR.run_c(case, conds, total, seed=9, sim_offset=100)
    assert rc == 0, _err()
    for cuts in ([1], [25000], [7, 4096, 30000, 50000]):
        acc = {k: np.zeros_like(v) for k, v in whole.items()}
        edges = [0] + cuts + [total]
        for a, b in zip(edges, edges[1:]):
            rc, part = CR.run_c(case, conds, b - a, seed=9, sim_offset=100 + a)
            assert rc == 0, _err()
            acc = _sum(acc, part)
        _equal(acc, whole, cuts)
    # two-device-style shards through the simulator surface: device [0, 0] shards by offset
    names = list(case['grid_probs'])
    texts = {'win': f'{names[0]}.wins', 'both': f'{names[0]}.podium & {names[1]}.podium', 'sc': 'sc>=1'}
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    one = RaceSimulator(RaceConfig(**case['config']), device=0, set_pop=RR.SET_POP).run_conditions(
        30001, texts, *args, seed=9, sim_offset=100)
    two = RaceSimulator(RaceConfig(**case['config']), device=[0, 0], set_pop=RR.SET_POP).run_conditions(
        30001, texts, *args, seed=9, sim_offset=100)
    assert one.counts == two.counts and all(0 < c < 30001 for c in one.counts.values())
    assert np.array_equal(one.hist, two.hist) and np.array_equal(one.cond_hist, two.cond_hist)


def test_a_run_longer_than_one_staging_chunk(require_gpu):
    case = O.load_case('N10')
    n, seed = 10, 4
    conds = _named(case, seed=seed)
    rc, _ = CR.run_c(case, conds, 10 ** 6, seed)                       # a full launch: the device's round
    assert rc == 0, _err()
    chunk = CR.chunk_sims(n, TR.device_round())
    assert CR.budget_sims(n) == (256 << 20) // 18 // 256 * 256 and chunk > 10 ** 6
    total = chunk + 70001                                              # one call crosses a chunk boundary, the halves do not
    rc, whole = CR.run_c(case, conds, total, seed, sim_offset=100)
    assert rc == 0, _err()
    h = total // 2
    assert h < chunk
    rc1, a = CR.run_c(case, conds, h, seed, sim_offset=100)
    rc2, b = CR.run_c(case, conds, total - h, seed, sim_offset=100 + h)
    assert rc1 == rc2 == 0
    _equal(whole, _sum(a, b), 'chunks')
    assert whole['count'][-2] == total and (whole['cond_hist'].sum(axis=2) == whole['count'][:, None]).all()


def _launch_info():
    g, b, l = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert N.lib().mcgp_last_launch_info(0, C.byref(g), C.byref(b), C.byref(l)) == 0
    return g.value, b.value


def test_forced_small_chunks_are_observed_and_sum_to_one_call(require_gpu, monkeypatch):
    """The chunk loop itself, seen from outside: a launch cap of 4096 simulations (the library's own test hook) makes a
    chunk 4096 simulations, and the first chunk's race launch then has ceil(4096 / block) blocks -- which
    mcgp_last_launch_info reports -- where the uncapped call has hundreds.  13 chunks, the last one partial, with the
    staging overwritten every time, equal the one-chunk call cell for cell."""
    case = O.load_case('S60')
    conds = _named(case)
    total = 12 * 4096 + 1234
    rc, one = CR.run_c(case, conds, total, seed=9, sim_offset=100)
    assert rc == 0, _err()
    grid_one, block = _launch_info()
    assert grid_one * block >= total                                  # one chunk: the whole run in one launch's grid
    monkeypatch.setenv('MCGP_MAX_SIMS_PER_LAUNCH', '4096')
    rc, many = CR.run_c(case, conds, total, seed=9, sim_offset=100)
    assert rc == 0, _err()
    grid_many, block_many = _launch_info()
    monkeypatch.delenv('MCGP_MAX_SIMS_PER_LAUNCH')
    assert block_many == block and grid_many == -(-4096 // block) < grid_one      # the first chunk held 4096 simulations
    _equal(many, one, 'forced chunks')
    rc, only = CR.run_c(case, conds, total, seed=9, sim_offset=100, cond_hist=False)
    assert rc == 0, _err()
    _equal(only, one, 'after the cap is lifted', keys=('hist', 'count'))


# ---------------------------------------------------------------- identities at a million
def test_identities_against_other_entry_points_at_a_million(require_gpu):
    case = O.load_case('S60')
    N_, n, L, seed = 10 ** 6, 20, 60, 21
    A, B, D = 0, 1, 2
    HI, LO = CR.HI, CR.LO
    conds = [[(CR.AHEAD_BY, A, B, 1, HI, 0)],                                            # 0  A.beats.B
             [(CR.AHEAD_BY, B, A, 1, HI, 0)],                                            # 1  B.beats.A
             [(CR.POSITION, A, 0, 1, 1, 0), (CR.POSITION, B, 0, 2, 2, 0), (CR.POSITION, D, 0, 3, 3, 0)],   # 2  podium A B D
             [(CR.POSITION, B, 0, 1, 1, 0), (CR.POSITION, D, 0, 2, 2, 0), (CR.POSITION, A, 0, 3, 3, 0)],   # 3  podium B D A
             [(CR.SAFETY_CARS, 0, 0, 0, 0, 0)], [(CR.SAFETY_CARS, 0, 0, 1, 1, 0)],       # 4, 5, 6  sc in k..k
             [(CR.SAFETY_CARS, 0, 0, 2, 2, 0)],
             [(CR.RED_FLAGS, 0, 0, 1, 1, 0)], [(CR.VSCS, 0, 0, 1, 1, 0)],                # 7, 8
             [(CR.RETIRED_LAP, D, 0, 1, HI, 0)], [(CR.RETIRED_LAP, n - 1, 0, 1, HI, 0)],   # 9, 10  D.dnf
             [(CR.RETIRED_LAP, D, 0, 1, HI, 1)],                                         # 11 !D.dnf
             [(CR.GAINED, A, 0, 3, HI, 0)], [(CR.GAINED, A, 0, 3, HI, 1)],               # 12, 13  c and !c
             [(CR.FINISHERS, 0, 0, LO, 15, 0)], [(CR.FINISHERS, 0, 0, 16, HI, 0)],       # 14, 15
             CR.EMPTY]                                                                   # 16
    small = CR.oracle_facts(case, 2048, seed)                          # informative already on the first 2048 simulations
    CR.assert_informative(small, conds, constant=(16,))
    rc, got = CR.run_c(case, conds, N_, seed)
    assert rc == 0, _err()
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=RR.SET_POP)
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    m = sim.run_matchups(N_, *args, seed=seed, track_condition=case['track_condition'])
    rc, t = TR.run_c(case, N_, seed)
    assert rc == 0, _err()
    cnt = got['count']
    assert np.array_equal(got['hist'], m.hist) and np.array_equal(got['hist'], t['hist'])
    assert cnt[0] == m.ahead[A, B] and cnt[1] == m.ahead[B, A] and cnt[0] + cnt[1] == N_
    assert cnt[2] == m.podium[A, B, D] > 0 and cnt[3] == m.podium[B, D, A] > 0
    assert [cnt[4], cnt[5], cnt[6]] == t['events'][1, :3].tolist()
    assert cnt[7] == t['events'][0, 1] and cnt[8] == t['events'][2, 1]
    assert cnt[9] == t['lap_pos'][L - 1, D, n] and cnt[10] == t['lap_pos'][L - 1, n - 1, n]
    assert cnt[9] + cnt[11] == N_ and cnt[12] + cnt[13] == N_ and cnt[14] + cnt[15] == N_
    assert cnt[16] == N_ and np.array_equal(got['cond_hist'][16], got['hist'])
    assert np.array_equal(got['cond_hist'][12] + got['cond_hist'][13], got['hist'])
    assert (got['cond_hist'].sum(axis=2) == cnt[:, None]).all()
    # a podium condition's histogram is one cell per driver of the podium
    assert got['cond_hist'][2][A, 0] == got['cond_hist'][2][B, 1] == got['cond_hist'][2][D, 2] == cnt[2]
    f = C.c_float()
    assert N.lib().mcgp_last_kernel_ms(0, C.byref(f)) == 0 and f.value > 0


# ---------------------------------------------------------------- the surface and the CLI
def test_simulator_surface(require_gpu):
    case = O.load_case('EVT')
    names = list(case['grid_probs'])
    m, seed = 4000, 2
    a, b = names[0], names[1]
    texts = {'double': f'{a}.wins & {b}.podium', 'sc': 'sc>=1', 'pole': f'{a}.pole', 'out': f'{b}.dnf',
             'gain': f'{b}.gain>=3', 'few': 'finishers<16', 'beats': f'{b}.beats.{a}', 'never': 'finishers<0'}
    tuples = [[dataclasses.astuple(at)[:5] + (int(at.negate),) for at in CD.parse(t, names).atoms] for t in texts.values()]
    facts = CR.oracle_facts(case, m, seed)
    CR.assert_informative(facts, tuples, constant=(7,))
    want = CR.counts(facts, tuples)
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=RR.SET_POP)
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    res = sim.run_conditions(m, texts, *args, seed=seed, track_condition=case['track_condition'])
    assert [res.counts[k] for k in texts] == want['count'].tolist()
    assert np.array_equal(res.cond_hist, want['cond_hist']) and np.array_equal(res.hist, want['hist'])
    assert np.array_equal(sim.last_histogram, res.hist)
    probs = sim.run_monte_carlo(m, *args, seed=seed, track_condition=case['track_condition'])
    assert res.position_probabilities() == probs
    assert res.probability('sc') == want['count'][1] / m
    assert res.win_probability('sc', a) == want['cond_hist'][1][0, 0] / want['count'][1]
    assert res.podium_probability('pole', a) == want['cond_hist'][2][0, :3].sum() / want['count'][2]
    with pytest.raises(ValueError, match='never'):
        res.win_probability('never', a)
    light = sim.run_conditions(m, texts, *args, seed=seed, track_condition=case['track_condition'], histograms=False)
    assert light.counts == res.counts and light.cond_hist is None and light.probability('sc') == res.probability('sc')
    with pytest.raises(ValueError, match='not collected'):
        light.win_probability('sc', a)


def _cli_case():
    inp = F1Predictor().simulator_inputs(cli.synthetic_fixture(), 'Bahrain')
    cfg = dataclasses.asdict(inp['config'])
    return dict(config=cfg, grid_probs=inp['grid_probs'], base_pace=inp['base_pace'], tire_deg=inp['tire_deg'],
                driver_variance=inp['driver_variance'], driver_dnf_rates=inp['driver_dnf_rates'],
                track_condition=inp['track_condition'])


def test_cli_conditions_end_to_end(require_gpu, tmp_path, capsys):
    """predict --if and in-race --if on the offline fixture: the probabilities are reference counts / N."""
    case = _cli_case()
    drivers = list(case['grid_probs'])
    m, seed = 2000, 5
    a, b = drivers[0], drivers[1]
    texts = [f'{a}.wins & {b}.podium', 'sc>=1', f'{b}.pole']
    tuples = [[dataclasses.astuple(at)[:5] + (int(at.negate),) for at in CD.parse(t, drivers).atoms] for t in texts]
    ref_run = O.Problem(case, set_pop=DEFAULT_SET_POP).run(m, rng=O.RNG_PHILOX, seed=seed, want_orders=True,
                                                           want_grids=True, n_trace=m)
    facts = CR.oracle_facts(case, m, seed, ref=ref_run)
    CR.assert_informative(facts, tuples)
    want = CR.counts(facts, tuples)
    out = tmp_path / 'cond.json'
    argv = ['predict', '--race', 'Bahrain', '--season', '2024', '--offline', '--simulations', str(m), '--seed', str(seed)]
    for t in texts:
        argv += ['--if', t]
    assert cli.main(argv + ['--json', str(out)]) == 0
    text = capsys.readouterr().out
    assert 'CONDITIONS' in text and texts[0] in text
    block = json.loads(out.read_text())['conditions']
    for c, t in enumerate(texts):
        assert block[t]['count'] == want['count'][c] and block[t]['probability'] == want['count'][c] / m
        for i, d in enumerate(drivers):
            assert block[t]['win'][d]['given'] == want['cond_hist'][c][i, 0] / want['count'][c]
            assert block[t]['win'][d]['unconditional'] == want['hist'][i, 0] / m
            assert block[t]['podium'][d]['given'] == want['cond_hist'][c][i, :3].sum() / want['count'][c]
    # in-race: simulation 0's state after lap 30 continued as 1 simulation is the oracle's simulation 0, events from lap 31
    k = 30
    state = RR.race_state(RR.state_arrays(ref_run, 0, k), k, RR.drs_disabled_until(case, seed, 0, k), drivers)
    path, out2 = tmp_path / 'lap30.json', tmp_path / 'inrace.json'
    path.write_text(json.dumps(state.to_json()))
    argv = ['in-race', '--race', 'Bahrain', '--season', '2024', '--offline', '--state', str(path), '--simulations', '1',
            '--seed', str(seed)]
    for t in texts:
        argv += ['--if', t]
    assert cli.main(argv + ['--json', str(out2)]) == 0
    assert 'CONDITIONS' in capsys.readouterr().out
    block = json.loads(out2.read_text())[0]['conditions']
    one = CR.counts(CR.oracle_facts(case, 0, seed, ref=ref_run, sims=[0], lap0=k), tuples)
    assert [block[t]['count'] for t in texts] == one['count'].tolist()
