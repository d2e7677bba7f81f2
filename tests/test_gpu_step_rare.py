"""The lap step with its pit writes behind a branch (csrc/race_isa.hip.h step_commit*) on the device, against the CPU
oracle's Philox back-ends, exactly.  The configurations of tests/step_rare_cases.py -- the window never opens; a stop on every
lap of the window; the same with retirements on most laps; S60's parameters as they are; safety cars, VSCs and red flags in
most races -- through mcgp_run_device with the finishing orders written, at both deviate widths, and through one
mcgp_run_batch call that mixes field sizes on the form with the branch, on the form without it and on the select form.
Every run has 64 k + 1 simulations from a simulation id that is no multiple of 64: the last wave enters the statement with
63 lanes off, and the branch decision must not see them.  No run is sized like the benchmark."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import step_rare_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip(require_gpu):
    from monte_carlo_gp_amd import _native as N
    N.lib()
    with open('/proc/self/maps') as f:
        paths = sorted({line.split()[-1] for line in f if 'libamdhip64' in line})
    h = C.CDLL(paths[0])
    assert h.hipSetDevice(0) == 0
    return h


def run_device(hip, case, n_sims, seed, sim_offset, deviates=32):
    """(hist, orders) of mcgp_run_device into device buffers of the caller."""
    from monte_carlo_gp_amd import RaceConfig
    from monte_carlo_gp_amd import _native as N
    from monte_carlo_gp_amd.simulation import RaceSimulator, _Problem, _dptr

    def ok(rc):
        assert rc == 0, f'HIP error {rc}'
    drivers = list(case['grid_probs'])
    p = _Problem(RaceConfig(**case['config']), drivers, case['base_pace'], case['tire_deg'], case['driver_variance'],
                 case['driver_dnf_rates'], case['track_condition'], O.load_cases()['set_pop'], deviates)
    g = RaceSimulator._grid_matrix(case['grid_probs'], drivers)
    n = p.n
    d_hist, d_orders = C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(d_hist), C.c_size_t(n * n * 8)))
    ok(hip.hipMalloc(C.byref(d_orders), C.c_size_t(n_sims * n + 64)))
    try:
        ok(hip.hipMemset(d_hist, 0, C.c_size_t(n * n * 8)))
        ok(hip.hipMemset(d_orders, 0xEE, C.c_size_t(n_sims * n + 64)))
        N.check(N.lib().mcgp_run_device(C.byref(p.cfg), C.byref(p.drv), _dptr(g), n, n_sims, C.c_uint64(sim_offset),
                                        C.c_uint64(seed), 0, C.c_void_p(0), d_hist, d_orders))
        ok(hip.hipDeviceSynchronize())
        raw = np.zeros(n_sims * n + 64, np.uint8)
        hist = np.zeros((n, n), np.uint64)
        ok(hip.hipMemcpy(raw.ctypes.data_as(C.c_void_p), d_orders, C.c_size_t(raw.size), 2))
        ok(hip.hipMemcpy(hist.ctypes.data_as(C.c_void_p), d_hist, C.c_size_t(hist.nbytes), 2))
    finally:
        hip.hipFree(d_hist)
        hip.hipFree(d_orders)
    assert (raw[n_sims * n:] == 0xEE).all()          # nothing written for the 63 lanes past the end
    return hist.astype(np.int64), raw[:n_sims * n].reshape(n_sims, n)


@pytest.mark.parametrize('config', R.CONFIGS)
@pytest.mark.parametrize('n', R.SIZES)
def test_default_kernel(hip, n, config):
    case, orders, hist = R.reference(n, config, O.RNG_PHILOX, R.WAVE_SIMS, R.SIM_OFFSET)
    got_hist, got = run_device(hip, case, R.WAVE_SIMS, R.seed_of(n, config), R.SIM_OFFSET)
    bad = np.nonzero((got != orders).any(axis=1))[0]
    assert bad.size == 0, f'n = {n}, {config}: {bad.size} finishing orders differ, first {bad[:5]}'
    assert np.array_equal(got_hist, hist)


@pytest.mark.parametrize('config', R.CONFIGS)
@pytest.mark.parametrize('n', R.SIZES)
def test_reference_width_kernel(hip, n, config):
    case, orders, hist = R.reference(n, config, O.RNG_PHILOX53, R.WAVE_SIMS, R.SIM_OFFSET)
    got_hist, got = run_device(hip, case, R.WAVE_SIMS, R.seed_of(n, config), R.SIM_OFFSET, deviates=53)
    bad = np.nonzero((got != orders).any(axis=1))[0]
    assert bad.size == 0, f'n = {n}, {config}: {bad.size} finishing orders differ, first {bad[:5]}'
    assert np.array_equal(got_hist, hist)


def test_one_batch_call_mixing_the_forms(require_gpu):
    """mcgp_run_batch: race_kernel_reg_batch<N> shares the lap step.  20, 21 and 22 cars (the branch form; four, one and two
    slots in the last statement), 5 (the form without it) and 12 (the select form), every configuration, in one call."""
    from monte_carlo_gp_amd import RaceConfig, run_monte_carlo_batch
    plan = [(n, config) for config in R.CONFIGS for n in (20, 5, 12, 21, 22)]

    def problem(n, config):
        c = R.reference(n, config, O.RNG_PHILOX, R.WAVE_SIMS, R.SIM_OFFSET)[0]
        return dict(config=RaceConfig(**c['config']), grid_probs=c['grid_probs'], base_pace=c['base_pace'],
                    tire_deg=c['tire_deg'], driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'],
                    seed=R.seed_of(n, config), track_condition=c['track_condition'], sim_offset=R.SIM_OFFSET)
    out = run_monte_carlo_batch([problem(n, config) for n, config in plan], R.WAVE_SIMS, device=0, set_pop=O.load_cases()['set_pop'])
    for (n, config), (probs, hist) in zip(plan, out):
        assert np.array_equal(hist, R.reference(n, config, O.RNG_PHILOX, R.WAVE_SIMS, R.SIM_OFFSET)[2]), (n, config)


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
        "import oracle_py as O\n"
        "import step_rare_cases as R\n"
        "from helpers import product_run\n"
        "from monte_carlo_gp_amd import _native as N\n"
        "for n in (20, 21):\n"
        "    for config in R.CONFIGS:\n"
        "        case, orders, hist = R.reference(n, config, O.RNG_PHILOX, R.WAVE_SIMS, R.SIM_OFFSET)\n"
        "        got_hist, _, got = product_run(case, R.WAVE_SIMS, R.seed_of(n, config), sim_offset=R.SIM_OFFSET, orders=True)\n"
        "        assert np.array_equal(got, orders) and np.array_equal(got_hist, hist), (n, config)\n"
        "    print(n, N.lib().mcgp_last_kernel_name(0).decode())\n")
    env = dict(os.environ, MCGP_LDS_PER_BLOCK='81920')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=O.ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    names = dict(ln.split(' ', 1) for ln in r.stdout.strip().splitlines())
    assert names['20'] == 'mcgp::race_kernel_reg<20, 4>' and names['21'] == 'mcgp::race_kernel_reg<21, 4>', names
