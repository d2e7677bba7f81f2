"""Pit windows on the GPU (mcgp_run_pit_windows / RaceSimulator.run_pit_windows / python -m monte_carlo_gp_amd.pit_window):
every count equals, cell for cell, what the numpy restatement (window_ref) derives from the CPU oracle's per-lap trace of
the same simulations.  From the grid and from mid-race states; 1 and 64 windows and the counts around the register
group; losses at which the grid slots decide; coverage conditions asserted from the reference before comparing, so that
equality is not vacuous; split, shard and staging-chunk invariance; the fuzz inputs; the command.  All comparisons are
integer equality.  The traced runs are made once and shared (_traced)."""
import ctypes as C
import dataclasses
import functools
import importlib
import json

import numpy as np
import pytest

import gaps_ref as GR
import generic_cases as G
import oracle_py as O
import resume_ref as RR
import trace_ref as TR
import window_ref as WR
from helpers import product_run
from monte_carlo_gp_amd import PitWindowResult, RaceConfig, RaceSimulator, cli, _native as N
from monte_carlo_gp_amd import predictor as P
from monte_carlo_gp_amd.predictor import F1Predictor
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP, _Problem

pytestmark = pytest.mark.gpu

B = len(WR.DEFAULT_EDGES) + 1
GROUP = 8               # csrc/pit_window.hip.h: kWindowGroup
LOSS = {'S60': 21.0, 'N10': 20.0, 'EVT': None, 'WET': None}          # the issue's coverage losses; None: the configured one


def _equal(a, b, what):
    for k in WR.KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        bad = np.argwhere(a[k] != b[k])
        assert bad.size == 0, (what, k, bad[:5].tolist(), a[k][tuple(bad[0])], b[k][tuple(bad[0])])


def _err():
    return N.lib().mcgp_last_error()


def _case(name):
    return G.fuzz_cases()[name] if name.startswith(('X_', 'F')) else O.load_case(name)


@functools.lru_cache(maxsize=None)
def _traced(name, m, seed, offset=0):
    """The oracle's traced run of a named case, made once: (case, run, slots)."""
    case = _case(name)
    ref = RR.traced_run(case, m, seed, offset)
    return case, ref, GR.slots_of(ref['grids'])


def _reference(name, m, seed, windows, offset=0, edges=WR.DEFAULT_EDGES):
    case, ref, slot = _traced(name, m, seed, offset)
    vals = WR.values_from_times(ref['trace']['cum'], ref['trace']['dnf'], slot, windows, edges)
    return case, ref, WR.window_counts(case, m, seed, offset, windows, edges, ref=ref, vals=vals)


def _free(counts, w, lap, n):
    """P(free stop | running) of window w for a stop at the end of `lap`, from the counts."""
    return counts['lost'][lap - 1, w, 0] / counts['lost'][lap - 1, w, :n].sum()


# ---------------------------------------------------------------- from the grid
@pytest.mark.parametrize('name', ['S60', 'N10', 'EVT', 'WET'])
def test_golden_cases_one_window_and_sixty_four(require_gpu, name):
    """512 simulations, seed 7: one window (driver 0 at the case's loss), then 64 (every driver at that loss, at none
    and at the run's own commonest time differences, where the grid slots decide the side of the rejoin)."""
    m, seed = 512, 7
    case, ref, _ = _traced(name, m, seed)
    tr = ref['trace']
    n = len(case['grid_probs'])
    pit_loss = float(case['config']['pit_loss'])
    loss = LOSS[name] or pit_loss
    losses = [loss, 0.0] + WR.own_losses(tr['cum'][:128], tr['dnf'][:128], most=1)
    losses += [x for x in (0.5, 11.0, 5.0, 1e6, 2.0) if x not in losses]
    per = 64 // n                                                      # whole rounds of the drivers, then a few more windows
    every = WR.every_driver(n, losses[:per]) + [(d, losses[per]) for d in range(64 - per * n)]
    assert len(every) == 64 and len(set(every)) == 64 and per >= 3
    losses = losses[:per]
    _, _, want = _reference(name, m, seed, every)
    # ---- coverage, from the reference alone
    ties = sum(WR.tie_cells(tr['cum'], tr['dnf'], x) for x in losses[1:])
    assert ties > 0, name                                              # the grid-slot half of the key is exercised
    if name in ('S60', 'N10', 'EVT'):
        assert WR.tie_cells(tr['cum'], tr['dnf'], pit_loss) == 0       # ... and only there: the configured loss ties nowhere
    if name == 'S60':
        assert losses[0] == 21.0 and every[0] == (0, 21.0) and every[19 * len(losses)] == (19, 21.0)
        assert (want['rejoin'][59, 0, 2:20] > 0).all() and want['lost'][59, 0, 19] > 0
        assert round(_free(want, 19 * len(losses), 30, n), 2) == 0.85
        assert _free(want, 0, 10, n) == 0 and _free(want, 0, 30, n) == 0
    if name == 'N10':
        assert every[0] == (0, 20.0) and round(_free(want, 0, case['config']['total_laps'], n), 2) == 0.73
    width = WR.widths(n, len(WR.DEFAULT_EDGES))
    for key in ('rejoin', 'lost', 'ahead'):                            # every position, count and car; retired; in the lead
        assert (want[key].sum(axis=(0, 1)) > 0).all() or name != 'S60', (name, key)
    assert want['rejoin'][:, :, n].sum() > 0 and want['ahead'][:, :, n].sum() > 0 and want['ahead'][:, :, n + 1].sum() > 0
    assert want['gap_behind'][:, :, B].sum() > want['rejoin'][:, :, n].sum()          # "no car behind" beside "retired"
    assert want['gap_ahead'][:, :, B].sum() > want['rejoin'][:, :, n].sum()           # "no car ahead" likewise
    assert all((want[k].sum(axis=2) == m).all() and want[k].shape[2] == width[k] for k in WR.ROWS)
    # ---- the device
    rc, got = WR.run_c(case, m, seed, windows=every)
    assert rc == 0, _err()
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_window_kernel'
    _equal(got, want, (name, 64))
    rc, one = WR.run_c(case, m, seed, windows=every[:1])
    assert rc == 0, _err()
    _equal(one, {k: (v if k == 'hist' else v[:, :1]) for k, v in want.items()}, (name, 1))
    hist, _, _ = product_run(case, m, seed)                            # the histogram is mcgp_run's
    assert np.array_equal(got['hist'], hist) and np.array_equal(one['hist'], hist)


@pytest.mark.parametrize('n', [1, 2, 32])
def test_synthetic_fields(require_gpu, n):
    case = RR.field_case(n)
    windows = WR.every_driver(n, [float(case['config']['pit_loss']), 0.0])
    rc, got = WR.run_c(case, 512, seed=3, windows=windows)
    assert rc == 0, _err()
    _equal(got, WR.window_counts(case, 512, seed=3, windows=windows), f'n={n}')
    if n == 1:
        assert (got['gap_ahead'][:, 0, B] == 512).all() and (got['gap_behind'][:, 0, B] == 512).all()


def test_one_edge_and_sixty_three_edges(require_gpu):
    """1 edge and 63: the narrowest and the widest rows the counting kernel takes (n + 2 = 22 and B + 1 = 65 values)."""
    fine = tuple(float(x) for x in np.concatenate([np.arange(1, 41) * 0.25, np.arange(1, 24) * 5.0 + 10.0]))
    assert len(fine) == 63
    windows = WR.every_driver(20, [21.0, 0.5])
    for edges in ((4.0,), fine):
        case, _, want = _reference('S60', 512, 7, windows, edges=edges)
        rc, got = WR.run_c(case, 512, seed=7, windows=windows, edges=edges)
        assert rc == 0, _err()
        _equal(got, want, len(edges))
    assert (want['gap_ahead'][29].sum(axis=0) > 0).sum() > 40          # the fine edges spread the gaps over the bins


def test_a_huge_loss_rejoins_last_with_nobody_behind(require_gpu):
    windows = WR.every_driver(20, [1e6])
    case, ref, want = _reference('S60', 512, 7, windows)
    assert (want['gap_behind'][:, :, B] == 512).all() and want['lost'][:, :, 19].sum() > 0
    running = (ref['trace']['dnf'][:, 59] == 0).sum(axis=1)
    # every runner rejoins behind all the others: position p is taken by the p + 1 runners of a simulation that has them
    assert np.array_equal(want['rejoin'][59, :, :20].sum(axis=0), np.bincount(running - 1, minlength=20) * np.arange(1, 21))
    rc, got = WR.run_c(case, 512, seed=7, windows=windows)
    assert rc == 0, _err()
    _equal(got, want, '1e6')


def test_window_counts_around_the_register_group(require_gpu):
    every = WR.every_driver(20, [21.0, 0.5, 11.0, 0.0])[:64]
    case, _, full = _reference('S60', 512, 7, every)
    for W in (GROUP - 1, GROUP, GROUP + 1, 2 * GROUP - 1, 2 * GROUP + 1, 63):
        rc, got = WR.run_c(case, 512, seed=7, windows=every[:W])
        assert rc == 0, _err()
        _equal(got, {k: (v if k == 'hist' else v[:, :W]) for k, v in full.items()}, W)


# ---------------------------------------------------------------- from a state
def test_oracle_states_continue_into_the_oracle_trace(require_gpu):
    """Oracle states after laps 1, L / 2, L - 1 and L continued as their own simulation into buffers pre-filled with a
    constant: rows k + 1 .. L equal the oracle trace's, earlier rows (all of them from lap L) stay as passed, the
    histogram is mcgp_run_from_state's."""
    total = 0
    for name in ('S60', 'EVT', 'N10', 'WET'):
        case, ref, slot = _traced(name, 6, 11, 500)
        L, seed, base = case['config']['total_laps'], 11, 500
        n = len(case['grid_probs'])
        windows = WR.every_driver(n, [float(case['config']['pit_loss']), 0.0])[:2 * GROUP + 1]
        vals = WR.values_from_times(ref['trace']['cum'], ref['trace']['dnf'], slot, windows)
        prob = RR.problem(case)
        for i in range(6):
            for k in (1, L // 2, L - 1, L):
                st = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k))
                want = WR.continued_counts(ref, [i], k, windows, vals=vals)
                into = {key: np.full_like(v, 9, dtype=np.uint64) for key, v in want.items()}
                rc, got = WR.run_c(case, 1, seed, sim_offset=base + i, windows=windows, state=st, prob=prob, into=into)
                assert rc == 0, _err()
                for key in WR.ROWS:
                    assert (got[key][:k] == 9).all(), (name, i, k, key)            # earlier laps: as the caller passed them
                _equal({key: v - 9 for key, v in got.items()}, want, (name, i, k))
                rc, hist, _ = RR.run_c(prob, [st], 1, [base + i], seed, orders=False)
                assert rc == 0 and np.array_equal(got['hist'] - 9, hist[0])
                total += 1
    assert total == 96


def test_one_state_continued_as_many_equals_the_restatement(require_gpu):
    case = O.load_case('S60')
    seed, k, m = 13, 31, 256
    ref = RR.traced_run(case, 3, seed)
    st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, seed, 2, k))
    windows = WR.every_driver(20, [21.0, 0.0, 11.0])
    want = WR.restated_counts(case, m, seed, sim_offset=1000, state=st, windows=windows)
    assert (want['rejoin'][k:].sum(axis=2) == m).all() and not want['rejoin'][:k].any()
    assert (want['rejoin'][-1, 0] > 0).sum() >= 8                      # the futures spread over the positions
    into = {key: np.full_like(v, 5, dtype=np.uint64) for key, v in want.items()}
    rc, got = WR.run_c(case, m, seed, sim_offset=1000, windows=windows, state=st, into=into)
    assert rc == 0, _err()
    for key in WR.ROWS:
        assert (got[key][:k] == 5).all(), key
    _equal({key: v - 5 for key, v in got.items()}, want, 'many from one')
    rc, hist, _ = RR.run_c(RR.problem(case), [st], m, [1000], seed, orders=False)
    assert rc == 0 and np.array_equal(got['hist'] - 5, hist[0])


# ---------------------------------------------------------------- invariance
def _sum(a, b):
    return {k: a[k] + b[k] for k in WR.KEYS}


def test_split_and_shards_equal_one_call_across_chunks(require_gpu):
    case = O.load_case('S60')
    windows = WR.every_driver(20, [21.0, 0.0, 11.0, 0.5])[:64]
    rc, _ = WR.run_c(case, 300000, seed=9, windows=windows[:1])        # a full launch: the device's round
    assert rc == 0, _err()
    chunk = WR.chunk_sims(60, 64, TR.device_round())
    assert WR.budget_sims(60, 64) == (1024 << 20) // (60 * 5 * 64) // 256 * 256 == 55808 and chunk <= 55808
    N_ = chunk + 7001                                  # one call crosses a chunk boundary, the halves do not
    rc, whole = WR.run_c(case, N_, seed=9, sim_offset=100, windows=windows)
    assert rc == 0, _err()
    h = N_ // 2
    rc1, a = WR.run_c(case, h, seed=9, sim_offset=100, windows=windows)
    rc2, b = WR.run_c(case, N_ - h, seed=9, sim_offset=100 + h, windows=windows)
    assert rc1 == rc2 == 0
    _equal(whole, _sum(a, b), 'split')
    assert all((whole[k].sum(axis=2) == N_).all() for k in WR.ROWS)
    # two-device-style shards through the simulator surface: device [0, 0] shards by offset
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    names = list(case['grid_probs'])
    named = [(names[d], x) for d, x in windows[:9]]
    one = RaceSimulator(RaceConfig(**case['config']), device=0, set_pop=RR.SET_POP).run_pit_windows(
        30001, *args, windows=named, seed=9, sim_offset=100)
    two = RaceSimulator(RaceConfig(**case['config']), device=[0, 0], set_pop=RR.SET_POP).run_pit_windows(
        30001, *args, windows=named, seed=9, sim_offset=100)
    rc, direct = WR.run_c(case, 30001, seed=9, sim_offset=100, windows=windows[:9])
    assert rc == 0
    for k in WR.KEYS:
        assert np.array_equal(getattr(one, k), getattr(two, k)) and np.array_equal(getattr(one, k), direct[k]), k
    probs = RaceSimulator(RaceConfig(**case['config']), device=0, set_pop=RR.SET_POP).run_monte_carlo(
        30001, *args, seed=9, sim_offset=100)
    assert one.position_probabilities() == probs and one.first_lap == 1


# ---------------------------------------------------------------- the fuzz inputs
@pytest.mark.parametrize('part', range(4))
def test_fuzz_inputs(require_gpu, part):
    """generic_cases' inputs (the 84 fuzz configurations among them, X_all_out_lap1 too: every window retired from lap
    1), 64 simulations each, every driver at the configured loss and at none."""
    done = 0
    for name, case, seed in G.run_input_slices(4)[part]:
        n = len(case['grid_probs'])
        windows = WR.every_driver(n, [float(case['config']['pit_loss']), 0.0])
        want = WR.window_counts(case, 64, seed, 3, windows)
        if name == 'X_all_out_lap1':
            assert (want['rejoin'][:, :, n] == 64).all() and (want['ahead'][:, :, n + 1] == 64).all()
        rc, got = WR.run_c(case, 64, seed, sim_offset=3, windows=windows)
        assert rc == 0, (name, _err())
        _equal(got, want, name)
        done += 1
    assert done >= 25


def test_no_noise_where_the_grid_slots_decide(require_gpu):
    """X_no_noise and X_all_attempt at no loss and at half a second: thousands of cells in which the rejoin time equals
    another car's and the slots decide."""
    for name in ('X_no_noise', 'X_all_attempt'):
        case, ref, _ = _traced(name, 64, 7)
        tr = ref['trace']
        n = len(case['grid_probs'])
        cells = {x: WR.tie_cells(tr['cum'], tr['dnf'], x) for x in (0.0, 0.5)}
        assert cells[0.0] > 0 and (name != 'X_no_noise' or min(cells.values()) > 1000), (name, cells)
        windows = WR.every_driver(n, [0.0, 0.5, float(case['config']['pit_loss'])])
        _, _, want = _reference(name, 64, 7, windows)
        rc, got = WR.run_c(case, 64, 7, windows=windows)
        assert rc == 0, _err()
        _equal(got, want, name)


# ---------------------------------------------------------------- the surface and the command
def _cli_case():
    inp = F1Predictor().simulator_inputs(cli.synthetic_fixture(), 'Bahrain')
    cfg = dataclasses.asdict(inp['config'])
    return dict(config=cfg, grid_probs=inp['grid_probs'], base_pace=inp['base_pace'], tire_deg=inp['tire_deg'],
                driver_variance=inp['driver_variance'], driver_dnf_rates=inp['driver_dnf_rates'],
                track_condition=inp['track_condition'])


def _result(case, counts, m, windows, first_lap=1):
    drivers = list(case['grid_probs'])
    return PitWindowResult(drivers=drivers, n_simulations=m, total_laps=case['config']['total_laps'],
                           edges=tuple(float(x) for x in WR.DEFAULT_EDGES), windows=[(drivers[d], x) for d, x in windows],
                           first_lap=first_lap, **counts)


def test_command_end_to_end_against_the_c_call(require_gpu, tmp_path, capsys):
    """python -m monte_carlo_gp_amd.pit_window on the offline fixture, from the grid and from a state: the JSON block is
    pit_window_keys of the C call's counts, which are the reference's."""
    command = importlib.import_module('monte_carlo_gp_amd.pit_window')
    case = _cli_case()
    drivers = list(case['grid_probs'])
    n, L = len(drivers), case['config']['total_laps']
    m, seed, d = 2000, 5, 3
    pit_loss, thr = float(case['config']['pit_loss']), float(case['config']['dirty_air_threshold'])
    windows = [(d, pit_loss), (d, 11.0)]
    prob = _Problem(RaceConfig(**case['config']), drivers, case['base_pace'], case['tire_deg'], case['driver_variance'],
                    case['driver_dnf_rates'], case['track_condition'], DEFAULT_SET_POP)
    ref_run = O.Problem(case, set_pop=DEFAULT_SET_POP).run(m, rng=O.RNG_PHILOX, seed=seed, want_orders=True,
                                                           want_grids=True, n_trace=m)
    rc, direct = WR.run_c(case, m, seed, windows=windows, prob=prob)
    assert rc == 0, _err()
    _equal(direct, WR.window_counts(case, m, seed, windows=windows, ref=ref_run), 'command case')
    out = tmp_path / 'window.json'
    assert command.main(['--race', 'Bahrain', '--season', '2024', '--offline', '--driver', drivers[d], '--loss', '11',
                         '--laps', '20-30', '--simulations', str(m), '--seed', str(seed), '--json', str(out)]) == 0
    text = capsys.readouterr().out
    want = P.pit_window_keys(_result(case, direct, m, windows), thr)
    saved = json.loads(out.read_text())
    assert saved['pit_window'] == json.loads(json.dumps(want))
    assert f'PIT WINDOW: {drivers[d]} losing {pit_loss:g} s' in text and f'PIT WINDOW: {drivers[d]} losing 11 s' in text
    assert f"{want['windows'][0]['free_stop'][24]:6.1%}" in text and '\n  20 ' in text and '\n  31 ' not in text
    # from a state: simulation 0's state after lap 30 continued as one simulation is the oracle's trace of simulation 0
    k = 30
    arrays, dd = RR.state_arrays(ref_run, 0, k), RR.drs_disabled_until(case, seed, 0, k)
    path, out2 = tmp_path / 'lap30.json', tmp_path / 'inrace.json'
    path.write_text(json.dumps(RR.race_state(arrays, k, dd, drivers).to_json()))
    assert command.main(['--race', 'Bahrain', '--season', '2024', '--offline', '--state', str(path), '--driver', drivers[d],
                         '--loss', '11', '--simulations', '1', '--seed', str(seed), '--json', str(out2)]) == 0
    text = capsys.readouterr().out
    rc, cont = WR.run_c(case, 1, seed, windows=windows, state=(arrays, k, dd), prob=prob)
    assert rc == 0, _err()
    _equal(cont, WR.continued_counts(ref_run, [0], k, windows), 'command state')
    want = P.pit_window_keys(_result(case, cont, 1, windows, first_lap=k + 1), thr)
    assert json.loads(out2.read_text())['pit_window'] == json.loads(json.dumps(want))
    assert 'after lap 30' in text and '\n  31 ' in text and '\n  30 ' not in text and want['first_lap'] == 31
    f = C.c_float()
    assert N.lib().mcgp_last_kernel_ms(0, C.byref(f)) == 0 and f.value > 0
