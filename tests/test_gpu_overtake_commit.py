"""The write-back chain of an overtake pass on the device (race_isa.hip.h ovt_commit*: the two additions of a successful
attempt issued under an execution mask narrowed to the lanes with a hit) against the CPU oracle: finishing orders and
histogram bit for bit, at both deviate widths.

4096 simulations are 64 waves: the lanes of a wave leave the pass loop at different passes, so the statements are entered
with part of the wave switched off.  The field sizes cover every form of the chain -- pairs go four to a statement, the
rest in a statement of one, two or three -- and every block shape; a few sizes keep the select form
(reg_commit_by_selects) and are here to show that both give the oracle's result."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
from helpers import product_run

pytestmark = pytest.mark.gpu

N_SIMS = 4096
WIDTHS = [(32, O.RNG_PHILOX), (53, O.RNG_PHILOX53)]


def _field(n, laps=20):
    """An n-car field with S60's parameters, paces 0.2 s apart and a grid drawn at random, so that faster cars start behind
    slower ones.  Below 20 cars overtake_delta is 0.05 s instead of S60's 0.6: neighbours 0.2 s apart never reach 0.6, and a
    small field would finish without one successful attempt (in a large one tyre ages and DRS spread the paces enough)."""
    rng = np.random.default_rng(1000 + n)
    base = O.load_case('S60')
    drivers = [f'D{i:02d}' for i in range(n)]
    case = dict(base)
    case['config'] = dict(base['config'], total_laps=laps, overtake_delta=base['config']['overtake_delta'] if n >= 20 else 0.05,
                          driver_teams={d: list(base['config']['dnf_rates'])[i % 10] for i, d in enumerate(drivers)})
    case['grid_probs'] = {d: [float(x) for x in rng.random(n)] for d in drivers}
    case['base_pace'] = {d: 90.0 + 0.2 * i for i, d in enumerate(drivers)}
    case['tire_deg'] = {d: 0.05 for d in drivers}
    case['driver_variance'] = {d: 0.2 for d in drivers}
    case['driver_dnf_rates'] = {d: 0.01 for d in drivers}
    return case


def _s60(laps=20):
    case = copy.deepcopy(O.load_case('S60'))
    case['config']['total_laps'] = laps
    return case


def _check(case, seed, kernel_prefix=None):
    from monte_carlo_gp_amd import _native as N
    for deviates, rng in WIDTHS:
        ref = O.Problem(case).run(N_SIMS, rng=rng, seed=seed, sim_offset=3, want_orders=True)
        hist, _, orders = product_run(case, N_SIMS, seed, sim_offset=3, orders=True, deviates=deviates)
        name = N.lib().mcgp_last_kernel_name(0).decode()
        if kernel_prefix is not None:
            assert name.startswith(kernel_prefix if deviates == 32 else 'mcgp::race_kernel_reg_wide<'), name
        bad = np.nonzero((orders != ref['orders']).any(axis=1))[0]
        assert bad.size == 0, f'deviates {deviates}: {bad.size} of {N_SIMS} finishing orders differ, first sims {bad[:5]}'
        assert np.array_equal(hist, ref['hist']), f'deviates {deviates}'


# pairs = n - 1:  2 -> a statement of one;  3, 4 -> of two, of three;  5 -> one full statement of four;  6, 7 -> a full one and a
# rest (6 keeps the select form);  21 -> five full ones, blocks of 11 waves;  32 -> seven full ones and three, 2 waves per SIMD
@pytest.mark.parametrize('n', [2, 3, 4, 5, 6, 7, 21, 32])
def test_field_sizes_match_the_oracle(require_gpu, n):
    case = _field(n)
    _check(case, seed=11 + n, kernel_prefix=f'mcgp::race_kernel_reg<{n}>')
    # ... and the chain had work to do: with no pair ever attempting, the same draws give another finishing order in
    # at least one race in ten (the oracle alone: 15 % at 2 cars, 41 % at 7, 99 % from 21 on)
    with_ovt = O.Problem(case).run(N_SIMS, rng=O.RNG_PHILOX, seed=11 + n, sim_offset=3, want_orders=True)['orders']
    never = dict(case, config=dict(case['config'], overtake_delta=1e9))
    without = O.Problem(never).run(N_SIMS, rng=O.RNG_PHILOX, seed=11 + n, sim_offset=3, want_orders=True)['orders']
    assert (with_ovt != without).any(axis=1).mean() >= 0.1


def test_twenty_cars_match_the_oracle(require_gpu):
    """S60's parameters over 20 laps: four full statements and one of three, blocks of 12 waves."""
    _check(_s60(), seed=42, kernel_prefix='mcgp::race_kernel_reg<20>')


def test_twenty_cars_in_blocks_of_four_waves(require_gpu):
    """The same problem on a device that offers half the LDS per block: the 4-wave instantiation.  A child process, because
    the limit is read when the device context is created.  (Default width only: the smallest block of the reference-width
    kernel needs 163 008 bytes at 20 cars, so under this limit its launch is refused with an error that names both sizes; its
    chain is the code test_twenty_cars_match_the_oracle runs.)"""
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, 'tests')\n"
        "import oracle_py as O\n"
        "from helpers import product_run\n"
        "from monte_carlo_gp_amd import _native as N\n"
        "case = O.load_case('S60')\n"
        "case['config']['total_laps'] = 20\n"
        "ref = O.Problem(case).run(4096, rng=O.RNG_PHILOX, seed=42, sim_offset=3, want_orders=True)\n"
        "hist, _, orders = product_run(case, 4096, 42, sim_offset=3, orders=True)\n"
        "assert np.array_equal(orders, ref['orders']) and np.array_equal(hist, ref['hist'])\n"
        "print(N.lib().mcgp_last_kernel_name(0).decode())\n")
    env = dict(os.environ, MCGP_LDS_PER_BLOCK='81920')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=O.ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'mcgp::race_kernel_reg<20, 4>', r.stdout


def test_verdicts_of_the_general_path_go_through_the_chain(require_gpu):
    """overtake_delta = 0: most passes have a lane with more than eight attempts, the wave decides them eight at a time and
    hands the chain its verdicts as (word 0, threshold 1) for a success, (0, 0) otherwise."""
    case = copy.deepcopy(O.load_case('S60'))
    case['config']['overtake_delta'] = 0.0
    _check(case, seed=5, kernel_prefix='mcgp::race_kernel_reg<20>')


def test_a_batch_launch_matches_the_oracle(require_gpu):
    """Six 20-car problems in one launch of the batch kernel."""
    from monte_carlo_gp_amd import RaceConfig, run_monte_carlo_batch, _native as N
    names = ['S60', 'S78', 'S50', 'EVT', 'DMP', 'WET']
    cases = [copy.deepcopy(O.load_case(k)) for k in names]
    for c in cases:
        c['config']['total_laps'] = 20
    problems = [dict(config=RaceConfig(**c['config']), grid_probs=c['grid_probs'], base_pace=c['base_pace'], tire_deg=c['tire_deg'],
                     driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'], seed=300 + i,
                     track_condition=c['track_condition'], sim_offset=5 * i) for i, c in enumerate(cases)]
    out = run_monte_carlo_batch(problems, N_SIMS, device=0, set_pop=O.load_cases()['set_pop'])
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_kernel_reg_batch<20>'
    for i, (k, c, (_, hist)) in enumerate(zip(names, cases, out)):
        ref = O.Problem(c).run(N_SIMS, rng=O.RNG_PHILOX, seed=300 + i, sim_offset=5 * i)['hist']
        assert np.array_equal(hist, ref), k
