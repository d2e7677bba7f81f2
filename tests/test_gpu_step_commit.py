"""The lap step's commits under EXEC (csrc/race_isa.hip.h step_commit1..4) on the device, against the CPU oracle's Philox
back-ends, exactly: finishing orders and histograms of fields in which most cars stop several times, several on the
same lap, cars retire in mid-race and the pit window opens and closes inside the run.  Before anything is compared
the oracle's own trace shows that the seeds enter every path (step_commit_cases.assert_paths_entered): a stop, two stops
in one lap, a retirement in a lap >= 2, a retirement on a lap with a stop, an age past its threshold outside the window.
Field sizes: every N mod 4 (the one- to four-slot statements), both sides of each occupancy step."""
import numpy as np
import pytest

import oracle_py as O
import step_commit_cases as S
from helpers import product_run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n', S.SIZES)
def test_default_kernel(require_gpu, n):
    case, orders, hist = S.reference(n)
    got_hist, _, got = product_run(case, S.N_SIMS, S.seed_of(n), orders=True)
    bad = np.nonzero((got != orders).any(axis=1))[0]
    assert bad.size == 0, f'n = {n}: {bad.size} finishing orders differ, first {bad[:5]}'
    assert np.array_equal(got_hist, hist)


@pytest.mark.parametrize('n', S.SIZES)
def test_reference_width_kernel(require_gpu, n):
    case, orders, hist = S.reference(n, O.RNG_PHILOX53)
    got_hist, _, got = product_run(case, S.N_SIMS, S.seed_of(n), orders=True, deviates=53)
    assert np.array_equal(got, orders) and np.array_equal(got_hist, hist)


def test_a_run_that_ends_inside_a_wave(require_gpu):
    """64 x 3 + 5 simulations: the last wave runs with 59 lanes that record nothing."""
    case, orders, hist = S.reference(20, O.RNG_PHILOX, S.TAIL_SIMS)
    got_hist, _, got = product_run(case, S.TAIL_SIMS, S.seed_of(20), orders=True)
    assert np.array_equal(got, orders) and np.array_equal(got_hist, hist)


def test_one_batch_call_with_three_field_sizes(require_gpu):
    """mcgp_run_batch: race_kernel_reg_batch<N> shares the lap step; 3, 20 and 22 cars (three, four and two slots in the
    last statement) in one call."""
    from monte_carlo_gp_amd import RaceConfig, run_monte_carlo_batch
    plan = [3, 20, 22, 20]

    def problem(n):
        c = S.reference(n)[0]
        return dict(config=RaceConfig(**c['config']), grid_probs=c['grid_probs'], base_pace=c['base_pace'],
                    tire_deg=c['tire_deg'], driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'],
                    seed=S.seed_of(n), track_condition=c['track_condition'], sim_offset=0)
    out = run_monte_carlo_batch([problem(n) for n in plan], S.N_SIMS, device=0, set_pop=O.load_cases()['set_pop'])
    for n, (probs, hist) in zip(plan, out):
        assert np.array_equal(hist, S.reference(n)[2]), n


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
        "import step_commit_cases as S\n"
        "from helpers import product_run\n"
        "from monte_carlo_gp_amd import _native as N\n"
        "for n in (20, 21, 7):\n"
        "    case, orders, hist = S.reference(n)\n"
        "    got_hist, _, got = product_run(case, S.N_SIMS, S.seed_of(n), orders=True)\n"
        "    assert np.array_equal(got, orders) and np.array_equal(got_hist, hist), n\n"
        "    print(n, N.lib().mcgp_last_kernel_name(0).decode())\n")
    env = dict(os.environ, MCGP_LDS_PER_BLOCK='81920')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=O.ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names = dict(ln.split(' ', 1) for ln in r.stdout.strip().splitlines())
    assert names['20'] == 'mcgp::race_kernel_reg<20, 4>' and names['21'] == 'mcgp::race_kernel_reg<21, 4>', names
