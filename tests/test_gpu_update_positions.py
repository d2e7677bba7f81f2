"""The position update under EXEC (csrc/race_isa.hip.h upd_commit1..4) and its select form (csrc/race_kernel_reg.hip.h
update_positions_reg, the path of a wave with two equal times) on the device, against the CPU oracle's Philox back-ends,
exactly: finishing orders and histograms of a close field and a spread one per size.  Before anything is compared the
oracle's own trace shows that the seeds enter every path (update_positions_cases.assert_paths_entered): a retired car in
front of the first running one, a retired car between two running ones, DRS on and off, gaps on both sides of the
dirty-air bound, two running cars on equal times.  Field sizes: every N mod 4 (the one- to four-slot statements, opening
the field and further down it), both sides of each occupancy step."""
import numpy as np
import pytest

import oracle_py as O
import update_positions_cases as U
from helpers import product_run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('kind', U.KINDS)
@pytest.mark.parametrize('n', U.SIZES)
def test_default_kernel(require_gpu, n, kind):
    case, orders, hist = U.reference(n, kind)
    got_hist, _, got = product_run(case, U.N_SIMS, U.seed_of(n), orders=True)
    bad = np.nonzero((got != orders).any(axis=1))[0]
    assert bad.size == 0, f'n = {n}, {kind}: {bad.size} finishing orders differ, first {bad[:5]}'
    assert np.array_equal(got_hist, hist)


@pytest.mark.parametrize('kind', U.KINDS)
@pytest.mark.parametrize('n', U.SIZES)
def test_reference_width_kernel(require_gpu, n, kind):
    case, orders, hist = U.reference(n, kind, O.RNG_PHILOX53)
    got_hist, _, got = product_run(case, U.N_SIMS, U.seed_of(n), orders=True, deviates=53)
    assert np.array_equal(got, orders) and np.array_equal(got_hist, hist)


def test_a_run_that_ends_inside_a_wave(require_gpu):
    """64 x 3 + 5 simulations: the last wave runs with 59 lanes that are off at every statement's entry."""
    case, orders, hist = U.reference(20, 'spread', O.RNG_PHILOX, U.TAIL_SIMS)
    got_hist, _, got = product_run(case, U.TAIL_SIMS, U.seed_of(20), orders=True)
    assert np.array_equal(got, orders) and np.array_equal(got_hist, hist)


def test_one_batch_call_with_three_field_sizes(require_gpu):
    """mcgp_run_batch: race_kernel_reg_batch<N> shares the position update; 3, 20 and 22 cars (a three-slot statement that
    opens the field, four-slot ones, a two-slot one at the end) in one call, both fields."""
    from monte_carlo_gp_amd import RaceConfig, run_monte_carlo_batch
    plan = [(3, 'spread'), (20, 'close'), (22, 'spread'), (20, 'spread')]

    def problem(n, kind):
        c = U.reference(n, kind)[0]
        return dict(config=RaceConfig(**c['config']), grid_probs=c['grid_probs'], base_pace=c['base_pace'],
                    tire_deg=c['tire_deg'], driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'],
                    seed=U.seed_of(n), track_condition=c['track_condition'], sim_offset=0)
    out = run_monte_carlo_batch([problem(n, kind) for n, kind in plan], U.N_SIMS, device=0, set_pop=O.load_cases()['set_pop'])
    for (n, kind), (probs, hist) in zip(plan, out):
        assert np.array_equal(hist, U.reference(n, kind)[2]), (n, kind)


def test_blocks_of_four_waves(require_gpu):
    """race_kernel_reg<N, 4>, the block shape of a device that offers less LDS per block (the mechanism of
    test_gpu_parity.test_a_device_with_less_lds_gets_small_blocks: the limit is read when the device context is created,
    hence the child process)."""
    import os
    import subprocess
    import sys
    code = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, 'tests')\n"
        "import update_positions_cases as U\n"
        "from helpers import product_run\n"
        "from monte_carlo_gp_amd import _native as N\n"
        "for n in (20, 21, 7):\n"
        "    for kind in U.KINDS:\n"
        "        case, orders, hist = U.reference(n, kind)\n"
        "        got_hist, _, got = product_run(case, U.N_SIMS, U.seed_of(n), orders=True)\n"
        "        assert np.array_equal(got, orders) and np.array_equal(got_hist, hist), (n, kind)\n"
        "    print(n, N.lib().mcgp_last_kernel_name(0).decode())\n")
    env = dict(os.environ, MCGP_LDS_PER_BLOCK='81920')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=O.ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names = dict(ln.split(' ', 1) for ln in r.stdout.strip().splitlines())
    assert names['20'] == 'mcgp::race_kernel_reg<20, 4>' and names['21'] == 'mcgp::race_kernel_reg<21, 4>', names
