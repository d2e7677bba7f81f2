"""Races for the lap step's pit region (csrc/race_isa.hip.h step_commit*: the two pit writes and the fetch of the rule word
sit behind a branch the wave takes when none of its lanes stops), shared by tests/test_step_rare_host_build.py and
tests/test_gpu_step_rare.py: the configurations, and the oracle's results, computed once per process and read-only.

Field sizes: 4, 5, 6, 7 (a statement of four slots, then the tails of one, two and three), 20, 21 and 22 (the tails again
behind five statements of four; 5 and 6 keep the form without a branch, reg_step_plain(), so 21 and 22 are the one- and
two-slot tails of the form with it) and 12, a size of reg_step_by_selects()."""
import functools

import numpy as np

import oracle_py as O
import step_commit_cases as S
from test_gpu_parity import _field

SIZES = [4, 5, 6, 7, 12, 20, 21, 22]
CONFIGS = ['closed', 'always', 'always_retire', 's60', 'events']
N_SIMS = 2000
WAVE_SIMS = 64 * 9 + 1          # the last wave enters with 63 lanes off
SIM_OFFSET = 0x1_0000_0123      # simulation ids past 2^32, not a multiple of 64


def seed_of(n, config):
    return 7000 + 10 * n + CONFIGS.index(config)


def case_of(n, config):
    if config == 's60':
        # the clustered case: S60 as it is at 20 cars, its parameters on an n-car field otherwise
        if n == 20:
            return O.load_case('S60')
        case = _field(n)
        case['config'] = dict(case['config'], total_laps=O.load_case('S60')['config']['total_laps'])
        return case
    case = S.field(n)
    cfg = case['config']
    if config == 'closed':
        # remaining_laps > 5 never holds from lap 2 on: the region is never entered
        case['config'] = dict(cfg, total_laps=6)
        return case
    if config == 'events':
        # tyre ages drift apart between the lanes of a wave (a safety car and a VSC stop some races' clocks, not others'),
        # and a red flag changes compound in mid-stint
        case['config'] = dict(cfg, total_laps=30, sc_probability=0.5, vsc_probability=0.5, red_flag_probability=0.3)
        return case
    # 'always': optimal_laps = 1 for every compound, so every running car is past its threshold on every lap of the window;
    # 34 laps: remaining laps of 32 .. 6 pass through all four regimes of the pit rule (> 30, > 20, > 15, the rest), and a
    # car that has used one dry compound meets the two-compound rule at its second stop
    comp = {k: dict(v, optimal_laps=1) for k, v in cfg['tire_compounds'].items()}
    case['config'] = dict(cfg, total_laps=34, tire_compounds=comp)
    if config == 'always_retire':
        # ... with a retirement rate of 3 % per lap and car: most laps of a wave have a retirement while most cars still run, so
        # a slot has a stop in one lane and a retirement in another
        case['driver_dnf_rates'] = {d: 0.03 for d in case['grid_probs']}
    return case


def _events_seen(case, trace, config):
    """From the oracle's per-lap trace ([sim][lap - 1][driver], the state at the END of each lap): what the configuration
    is there for happens in the run."""
    age, dnf = trace['age'].astype(np.int64), trace['dnf'].astype(bool)
    L = case['config']['total_laps']
    stop = ~dnf[:, 1:] & (age[:, 1:] == 0)
    retire = dnf[:, 1:] & ~dnf[:, :-1]
    if config == 'closed':
        assert not stop.any(), 'a stop with the window closed'
    elif config in ('always', 'always_retire'):
        lap = np.arange(2, L + 1)
        window = L - lap > S.PIT_WINDOW
        # nearly every race has a stop on every lap of the window (a car whose threshold rounds to 0 stops on each lap it
        # runs, the others on every second one), and every wave of 64 races has one on each of them
        per_race = stop[:, window].any(axis=2)
        share = 0.9 if config == 'always' else 0.5          # (fewer once cars have retired)
        assert per_race.mean() > share, f'a stop on {per_race.mean():.2f} of the window laps only'
        assert per_race.reshape(-1, 64, per_race.shape[1]).any(axis=1).all(), 'a wave-lap of the window without a stop'
        if config == 'always_retire':
            assert (retire.any(axis=(0, 2))).mean() > 0.5, 'retirements on fewer than half of the laps'
            assert (retire.any(axis=2) & stop.any(axis=2)).any()
    else:
        assert stop.any() and retire.any()


@functools.lru_cache(maxsize=None)
def reference(n, config, rng=O.RNG_PHILOX, n_sims=N_SIMS, sim_offset=0):
    """(case, oracle orders, oracle histogram).  Read-only."""
    case = case_of(n, config)
    ref = O.Problem(case).run(n_sims, rng=rng, seed=seed_of(n, config), sim_offset=sim_offset, want_orders=True,
                              n_trace=min(n_sims, 256))
    _events_seen(case, ref['trace'], config)
    ref['orders'].setflags(write=False)
    ref['hist'].setflags(write=False)
    return case, ref['orders'], ref['hist']
