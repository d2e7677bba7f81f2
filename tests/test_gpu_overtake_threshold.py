"""The threshold stage of an overtake pass on the device (race_isa.hip.h ovt_threshold_x: per adjacent pair the threshold
and the advance of the W-plane row written under an execution mask narrowed to the candidates' lanes, the pair's draw word
fetched inside the statement and waited for by the last pair's) against the CPU oracle: finishing orders and histogram bit
for bit, at both deviate widths.

4096 simulations are 64 waves: the lanes of a wave leave the pass loop at different passes, so the statements are entered
with part of the wave switched off.  The cases go for what the statement must keep: a threshold of exactly 0 for a pair that
is no candidate (the general path builds its candidate mask from it), the 2^31 clamp, NaN paces of retired cars, the words
of a stage in which no lane has a candidate (their registers die at the branch out of the pass) and of one whose words the
general path overwrites, every block shape, and the field sizes that keep the select form (reg_threshold_by_selects)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
import overtake_threshold_cases as T
from helpers import product_run

pytestmark = pytest.mark.gpu

N_SIMS = 4096


def _check(case, seed, kernel_prefix=None):
    from monte_carlo_gp_amd import _native as N
    for deviates, rng in T.WIDTHS:
        ref = O.Problem(case).run(N_SIMS, rng=rng, seed=seed, sim_offset=3, want_orders=True)
        hist, _, orders = product_run(case, N_SIMS, seed, sim_offset=3, orders=True, deviates=deviates)
        name = N.lib().mcgp_last_kernel_name(0).decode()
        if kernel_prefix is not None:
            assert name.startswith(kernel_prefix if deviates == 32 else 'mcgp::race_kernel_reg_wide<'), name
        bad = np.nonzero((orders != ref['orders']).any(axis=1))[0]
        assert bad.size == 0, f'deviates {deviates}: {bad.size} of {N_SIMS} finishing orders differ, first sims {bad[:5]}'
        assert np.array_equal(hist, ref['hist']), f'deviates {deviates}'


# one pair (its statement is the waiting one) .. 31 pairs; 21: blocks of 11 waves; 24, 32: 2 waves per SIMD; and every size
# that keeps the select form
@pytest.mark.parametrize('n', sorted({2, 3, 4, 5, 6, 7, 21, 24, 32} | set(T.select_form_sizes())))
def test_field_sizes_match_the_oracle(require_gpu, n):
    case = T.field(n)
    _check(case, seed=11 + n, kernel_prefix=f'mcgp::race_kernel_reg<{n}>')
    # ... and the stage had work to do: with no pair ever a candidate, the same draws give another finishing order in at
    # least one race in ten (the oracle alone: 15 % at 2 cars, 41 % at 7, 99 % from 21 on)
    assert T.overtakes_change(case, N_SIMS, 11 + n, sim_offset=3) >= 0.1


@pytest.mark.parametrize('n', [3, 5, 20])
def test_every_threshold_at_the_clamp(require_gpu, n):
    """Every candidate's pace delta is at least 1 s: its threshold is 2^31 by construction.  (The oracle alone: overtakes
    change 12.4 % of the races at 2 cars, 23.7 % at 3, 40.9 % at 5, 92.7 % at 20.)"""
    case = T.clamp_field(n)
    _check(case, seed=7, kernel_prefix=f'mcgp::race_kernel_reg<{n}>')
    assert T.overtakes_change(case, N_SIMS, 7, sim_offset=3) >= 0.1


def test_the_general_path_sees_zero_thresholds(require_gpu):
    """overtake_delta = 0 on S60: most passes have a lane with more than eight attempts and take the general path, which
    takes a pair for a candidate iff its threshold is not 0 and overwrites the words the stage fetched."""
    _check(T.s60(overtake_delta=0.0), seed=5, kernel_prefix='mcgp::race_kernel_reg<20>')


def test_no_candidate_anywhere(require_gpu):
    """overtake_delta = 1e9: every threshold is 0 and every wave leaves the pass loop at the first stage, with the words it
    fetched never read."""
    _check(T.s60(overtake_delta=1e9), seed=6, kernel_prefix='mcgp::race_kernel_reg<20>')


def test_many_retired_cars(require_gpu):
    """A retirement rate of 5 % per driver: many NaN paces, whose pairs must compare false."""
    case = T.field(20)
    case['driver_dnf_rates'] = {d: 0.05 for d in case['driver_dnf_rates']}
    _check(case, seed=8, kernel_prefix='mcgp::race_kernel_reg<20>')


def test_twenty_cars_in_blocks_of_four_waves(require_gpu):
    """S60 over 20 laps on a device that offers half the LDS per block: the 4-wave instantiation.  A child process, because
    the limit is read when the device context is created (default width only: the reference-width kernel has no block that
    small at 20 cars)."""
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


def test_a_batch_launch_matches_the_oracle(require_gpu):
    """Six 20-car problems in one launch of the batch kernel."""
    from monte_carlo_gp_amd import RaceConfig, run_monte_carlo_batch, _native as N
    names = ['S60', 'S78', 'S50', 'EVT', 'DMP', 'WET']
    cases = [copy.deepcopy(O.load_case(k)) for k in names]
    for c in cases:
        c['config']['total_laps'] = 20
    problems = [dict(config=RaceConfig(**c['config']), grid_probs=c['grid_probs'], base_pace=c['base_pace'], tire_deg=c['tire_deg'],
                     driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'], seed=400 + i,
                     track_condition=c['track_condition'], sim_offset=7 * i) for i, c in enumerate(cases)]
    out = run_monte_carlo_batch(problems, N_SIMS, device=0, set_pop=O.load_cases()['set_pop'])
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_kernel_reg_batch<20>'
    for i, (k, c, (_, hist)) in enumerate(zip(names, cases, out)):
        ref = O.Problem(c).run(N_SIMS, rng=O.RNG_PHILOX, seed=400 + i, sim_offset=7 * i)['hist']
        assert np.array_equal(hist, ref), k
