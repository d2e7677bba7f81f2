"""Inputs of the mcgp_run_batch tests (tests/test_gpu_batch.py, the batch part of tests/test_host.py): n-car fields that differ
from problem to problem, and a list of (case, seed, sim_offset, deviates) turned into run_monte_carlo_batch's problems, into
the arrays of the C call and into the CPU oracle's histograms.  Not a test module."""
import ctypes as C

import numpy as np

import oracle_py as O

RATES = [0.3, 0.0, 1.0, 0.05 / 60, 0.3, 0.3]


def field(n, laps, shift=0, pace=0.0, **config):
    """An n-car field with S60's parameters, paces 0.2 s apart (every other driver `pace` s slower, so that it changes the
    order of the field and not only its level), a grid matrix drawn at random from a generator that depends on n alone, and
    per-lap retirement rates from RATES in turn, starting `shift` places in: drivers who never retire, who are out on lap 2,
    who retire often and S60's 0.05 / 60.  overtake_delta is 0.05 below 20 cars; `config` overrides entries of the race
    configuration, and `track_condition` the condition of the track."""
    rng = np.random.default_rng(3000 + n)
    base = O.load_case('S60')
    drivers = [f'D{i:02d}' for i in range(n)]
    track = config.pop('track_condition', base['track_condition'])
    case = dict(base, track_condition=track)
    cfg = dict(base['config'], total_laps=laps, overtake_delta=base['config']['overtake_delta'] if n >= 20 else 0.05,
               driver_teams={d: list(base['config']['dnf_rates'])[i % 10] for i, d in enumerate(drivers)})
    cfg.update(config)
    case['config'] = cfg
    case['grid_probs'] = {d: [float(x) for x in rng.random(n)] for d in drivers}
    case['base_pace'] = {d: 90.0 + 0.2 * i + (pace if i % 2 else 0.0) for i, d in enumerate(drivers)}
    case['tire_deg'] = {d: 0.05 for d in drivers}
    case['driver_variance'] = {d: 0.2 for d in drivers}
    case['driver_dnf_rates'] = {d: RATES[(i + shift) % len(RATES)] for i, d in enumerate(drivers)}
    return case


def problem(case, seed, sim_offset=0, deviates=32):
    """One entry of run_monte_carlo_batch's list."""
    from monte_carlo_gp_amd import RaceConfig
    return dict(config=RaceConfig(**case['config']), grid_probs=case['grid_probs'], base_pace=case['base_pace'],
                tire_deg=case['tire_deg'], driver_variance=case['driver_variance'], driver_dnf_rates=case['driver_dnf_rates'],
                seed=seed, track_condition=case['track_condition'], sim_offset=sim_offset, deviates=deviates)


def reference(case, n_sims, seed, sim_offset=0, deviates=32):
    """The oracle's histogram of one problem, from the back-end of its deviate width."""
    rng = O.RNG_PHILOX53 if deviates == 53 else O.RNG_PHILOX
    return O.Problem(case).run(n_sims, rng=rng, seed=seed, sim_offset=sim_offset)['hist']


def problems_and_references(specs, n_sims):
    """specs: a list of (case, seed, sim_offset, deviates).  The problems for run_monte_carlo_batch and the oracle's
    histograms, in the same order."""
    return [problem(*s) for s in specs], [reference(s[0], n_sims, *s[1:]) for s in specs]


def run_batch(specs, n_sims):
    """The histograms run_monte_carlo_batch gives for `specs`, in their order."""
    from monte_carlo_gp_amd import run_monte_carlo_batch
    out = run_monte_carlo_batch([problem(*s) for s in specs], n_sims, device=0, set_pop=O.load_cases()['set_pop'])
    return [hist for _, hist in out]


class RawBatch:
    """The arguments of mcgp_run_batch for problems of one field size, as the Python wrapper builds them; the arrays
    they point to stay alive with the object.  `hist` is what the call adds into."""

    def __init__(self, specs, fill=0):
        from monte_carlo_gp_amd import RaceConfig, RaceSimulator, _native as N
        from monte_carlo_gp_amd.simulation import _Problem, _dptr
        set_pop = O.load_cases()['set_pop']
        self.k = k = len(specs)
        self.n = n = len(specs[0][0]['grid_probs'])
        self.problems, self.grids_np = [], []
        for case, _, _, deviates in specs:
            drivers = list(case['grid_probs'])
            assert len(drivers) == n
            self.problems.append(_Problem(RaceConfig(**case['config']), drivers, case['base_pace'], case['tire_deg'],
                                          case['driver_variance'], case['driver_dnf_rates'], case['track_condition'], set_pop,
                                          deviates))
            self.grids_np.append(RaceSimulator._grid_matrix(case['grid_probs'], drivers))
        self.cfgs = (N.McgpConfig * k)(*[p.cfg for p in self.problems])
        self.drvs = (N.McgpDrivers * k)(*[p.drv for p in self.problems])
        self.grids = (C.POINTER(C.c_double) * k)(*[_dptr(g) for g in self.grids_np])
        self.seeds = (C.c_uint64 * k)(*[s[1] for s in specs])
        self.offsets = (C.c_uint64 * k)(*[s[2] for s in specs])
        self.hist = np.full((k, n, n), fill, np.uint64)

    @property
    def hist_ptr(self):
        return self.hist.ctypes.data_as(C.POINTER(C.c_uint64))

    def call(self, n_sims, **replace):
        """mcgp_run_batch's return code with these arguments, those named in `replace` replaced (n_problems, cfgs, drvs,
        grids, n, offsets, seeds, hist_ptr)."""
        from monte_carlo_gp_amd import _native as N
        a = dict(n_problems=self.k, cfgs=self.cfgs, drvs=self.drvs, grids=self.grids, n=self.n, offsets=self.offsets,
                 seeds=self.seeds, hist_ptr=self.hist_ptr)
        a.update(replace)
        return N.lib().mcgp_run_batch(a['n_problems'], a['cfgs'], a['drvs'], a['grids'], a['n'], n_sims, a['offsets'],
                                      a['seeds'], 0, a['hist_ptr'])


def last_launch():
    """(kernel name, blocks, threads per block, LDS bytes) of the last launch on device 0."""
    from monte_carlo_gp_amd import _native as N
    g, b, l = C.c_uint32(), C.c_uint32(), C.c_uint32()
    N.check(N.lib().mcgp_last_launch_info(0, C.byref(g), C.byref(b), C.byref(l)))
    return N.lib().mcgp_last_kernel_name(0).decode(), g.value, b.value, l.value
