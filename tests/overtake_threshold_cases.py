"""Fields for the tests of the overtake passes' threshold stage (csrc/race_isa.hip.h ovt_threshold_x: a pair's threshold and
row advance written under an execution mask narrowed to the candidates' lanes, the draw word fetched inside the statement;
ovt_threshold: the select form a few field sizes keep).  Shared by tests/test_gpu_overtake_threshold.py and its CPU twin."""
import copy
import os
import re

import numpy as np

import oracle_py as O

WIDTHS = [(32, O.RNG_PHILOX), (53, O.RNG_PHILOX53)]


def select_form_sizes():
    """The field sizes of reg_threshold_by_selects (csrc/race_kernel_reg.hip.h), read from the source."""
    src = open(os.path.join(O.ROOT, 'monte_carlo_gp_amd', 'csrc', 'race_kernel_reg.hip.h')).read()
    body = re.search(r'constexpr bool reg_threshold_by_selects\(int n\)\s*\{\s*return ([^;]*);', src).group(1)
    expr = body.replace('||', ' or ').replace('&&', ' and ')
    return [n for n in range(1, 33) if eval(expr, {'n': n})]


def field(n, laps=20):
    """tests/test_gpu_overtake_commit.py::_field with its seeds: an n-car field with S60's parameters, paces 0.2 s apart and
    a grid drawn at random, so that faster cars start behind slower ones.  Below 20 cars overtake_delta is 0.05 s instead of
    S60's 0.6 (neighbours 0.2 s apart never reach 0.6)."""
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


def clamp_field(n, laps=8):
    """Paces 1.2 s apart under a lap-time noise of 2 s: the noise shuffles the order, so attempts keep coming, and whenever
    a faster car sits behind a slower one their pace delta is at least 1 s -- the threshold of every candidate is the
    2^31 clamp, never the ceiling of a delta below it."""
    base = O.load_case('S60')
    drivers = [f'D{i:02d}' for i in range(n)]
    case = dict(base)
    case['config'] = dict(base['config'], total_laps=laps, overtake_delta=0.05,
                          driver_teams={d: list(base['config']['dnf_rates'])[i % 10] for i, d in enumerate(drivers)})
    case['grid_probs'] = {d: [float(x) for x in np.random.default_rng(2000 + n).random(n)] for d in drivers}
    case['base_pace'] = {d: 90.0 + 1.2 * i for i, d in enumerate(drivers)}
    case['tire_deg'] = {d: 0.05 for d in drivers}
    case['driver_variance'] = {d: 2.0 for d in drivers}
    case['driver_dnf_rates'] = {d: 0.01 for d in drivers}
    return case


def s60(laps=20, **config):
    case = copy.deepcopy(O.load_case('S60'))
    case['config']['total_laps'] = laps
    case['config'].update(config)
    return case


def overtakes_change(case, n_sims, seed, sim_offset=0):
    """Share of the races whose finishing order differs from the one the same draws give when no pair ever attempts."""
    with_ovt = O.Problem(case).run(n_sims, rng=O.RNG_PHILOX, seed=seed, sim_offset=sim_offset, want_orders=True)['orders']
    never = dict(case, config=dict(case['config'], overtake_delta=1e9))
    without = O.Problem(never).run(n_sims, rng=O.RNG_PHILOX, seed=seed, sim_offset=sim_offset, want_orders=True)['orders']
    return float((with_ovt != without).any(axis=1).mean())
