"""The retirement draw of the register kernels on the device -- a per-launch table of survival thresholds built by the host
(params_build.h: build_retire_table) and a binary search in it per driver and race (race_kernel_reg.hip.h: retire_search4)
-- against the CPU oracle, which still walks the chain lap by lap: finishing orders row for row and the histogram, at both
deviate widths.

One field mixes drivers who never retire (p = 0: no row to search), who certainly do (p >= 1: S_2 = 0, out on lap 2), p = 0.3
(several retirements per race, several on one lap, lanes with more than two) and S60's 0.05 / 60.  Field sizes: 1, 3 (a group of
four mostly padding), 4, 5 (one full group and one car), 20, 21, 23, 32 -- blocks of 12, 11 and 8 waves, 2 and 3 waves per SIMD;
at the reference width 20 and 21 cars over 60 laps read the table, the others the chain in the block's LDS.  Laps: 1 (an empty
table, no search round), 2 (one entry), 3, 5, 60 (rows of 64 entries, six rounds).  4096 + 37 simulations are 65 wave-chunks, the
last one ragged, from a simulation offset that is not zero."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
from helpers import product_run

pytestmark = pytest.mark.gpu

N_SIMS = 4096 + 37
OFFSET = 1000003
WIDTHS = [(32, O.RNG_PHILOX), (53, O.RNG_PHILOX53)]
RATES = [0.3, 0.0, 1.0, 0.05 / 60, 0.3, 0.3]


def _field(n, laps, shift=0):
    """An n-car field with S60's parameters, paces 0.2 s apart, a grid drawn at random and per-lap retirement rates from RATES
    in turn (starting `shift` places in)."""
    rng = np.random.default_rng(2000 + n)
    base = O.load_case('S60')
    drivers = [f'D{i:02d}' for i in range(n)]
    case = dict(base)
    case['config'] = dict(base['config'], total_laps=laps, overtake_delta=base['config']['overtake_delta'] if n >= 20 else 0.05,
                          driver_teams={d: list(base['config']['dnf_rates'])[i % 10] for i, d in enumerate(drivers)})
    case['grid_probs'] = {d: [float(x) for x in rng.random(n)] for d in drivers}
    case['base_pace'] = {d: 90.0 + 0.2 * i for i, d in enumerate(drivers)}
    case['tire_deg'] = {d: 0.05 for d in drivers}
    case['driver_variance'] = {d: 0.2 for d in drivers}
    case['driver_dnf_rates'] = {d: RATES[(i + shift) % len(RATES)] for i, d in enumerate(drivers)}
    return case


@pytest.mark.parametrize('laps', [1, 2, 3, 5, 60])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 20, 21, 23, 32])
def test_orders_match_the_oracle(require_gpu, n, laps):
    from monte_carlo_gp_amd import _native as N
    case = _field(n, laps)
    seed = 100 * n + laps
    for deviates, rng in WIDTHS:
        ref = O.Problem(case).run(N_SIMS, rng=rng, seed=seed, sim_offset=OFFSET, want_orders=True)
        hist, _, orders = product_run(case, N_SIMS, seed, sim_offset=OFFSET, orders=True, deviates=deviates)
        name = N.lib().mcgp_last_kernel_name(0).decode()
        assert name == (f'mcgp::race_kernel_reg<{n}>' if deviates == 32 else f'mcgp::race_kernel_reg_wide<{n}>'), name
        bad = np.nonzero((orders != ref['orders']).any(axis=1))[0]
        assert bad.size == 0, f'deviates {deviates}: {bad.size} of {N_SIMS} finishing orders differ, first sims {bad[:5]}'
        assert np.array_equal(hist, ref['hist']), f'deviates {deviates}'


def test_a_batch_of_two_problems_with_their_own_tables(require_gpu):
    """mcgp_run_batch, two 20-car problems in one launch that differ in laps (rows of 64 and of 4 entries) and in rates: each
    block reads the table of the problem it is on."""
    from monte_carlo_gp_amd import RaceConfig, run_monte_carlo_batch, _native as N
    cases = [_field(20, 60), _field(20, 5, shift=2)]
    problems = [dict(config=RaceConfig(**c['config']), grid_probs=c['grid_probs'], base_pace=c['base_pace'], tire_deg=c['tire_deg'],
                     driver_variance=c['driver_variance'], driver_dnf_rates=c['driver_dnf_rates'], seed=700 + i,
                     track_condition=c['track_condition'], sim_offset=OFFSET + 5 * i) for i, c in enumerate(cases)]
    out = run_monte_carlo_batch(problems, N_SIMS, device=0, set_pop=O.load_cases()['set_pop'])
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_kernel_reg_batch<20>'
    for i, (c, (_, hist)) in enumerate(zip(cases, out)):
        ref = O.Problem(c).run(N_SIMS, rng=O.RNG_PHILOX, seed=700 + i, sim_offset=OFFSET + 5 * i)['hist']
        assert np.array_equal(hist, ref), i


def test_consecutive_calls_on_one_stream_with_other_rates(require_gpu):
    """Two mcgp_run_device calls back to back on one stream, the same problem but for the retirement rates (and then the
    first again): each launch reads the table of its own rates, none a table left by the call before it."""
    import torch
    from monte_carlo_gp_amd import RaceConfig, _native as N
    from monte_carlo_gp_amd.simulation import RaceSimulator, _Problem, _dptr
    dev = torch.device('cuda', 0)
    stream = torch.cuda.Stream(dev)
    cases = [_field(20, 60), _field(20, 60, shift=1), _field(20, 60)]
    runs = []
    torch.cuda.synchronize(dev)
    for c in cases:
        drivers = list(c['grid_probs'])
        p = _Problem(RaceConfig(**c['config']), drivers, c['base_pace'], c['tire_deg'], c['driver_variance'],
                     c['driver_dnf_rates'], c['track_condition'], O.load_cases()['set_pop'])
        g = RaceSimulator._grid_matrix(c['grid_probs'], drivers)
        d_hist = torch.zeros(p.n * p.n, dtype=torch.int64, device=dev)
        d_orders = torch.zeros(N_SIMS * p.n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        runs.append((p, g, d_hist, d_orders))
    for p, g, d_hist, d_orders in runs:                         # nothing between the launches but the next call
        N.check(N.lib().mcgp_run_device(C.byref(p.cfg), C.byref(p.drv), _dptr(g), p.n, N_SIMS, OFFSET, 9, 0,
                                        C.c_void_p(stream.cuda_stream), C.c_void_p(d_hist.data_ptr()),
                                        C.c_void_p(d_orders.data_ptr())))
    torch.cuda.synchronize(dev)
    refs = [O.Problem(c).run(N_SIMS, rng=O.RNG_PHILOX, seed=9, sim_offset=OFFSET, want_orders=True) for c in cases[:2]]
    assert (refs[0]['orders'] != refs[1]['orders']).any()       # (the rates matter)
    for i, (p, g, d_hist, d_orders) in enumerate(runs):
        ref = refs[i % 2]
        orders = d_orders.cpu().numpy().reshape(N_SIMS, p.n)
        bad = np.nonzero((orders != ref['orders']).any(axis=1))[0]
        assert bad.size == 0, f'call {i}: {bad.size} of {N_SIMS} finishing orders differ, first sims {bad[:5]}'
        assert np.array_equal(d_hist.cpu().numpy().reshape(p.n, p.n), ref['hist']), i
