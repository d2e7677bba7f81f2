"""Fields that load the commit paths of the register kernel's lap step (csrc/race_isa.hip.h: step_commit*), shared by
tests/test_step_commit_host_build.py and tests/test_gpu_step_commit.py: the cases, the oracle's results (computed
once per process) and the proof from the oracle's own trace that the chosen seeds enter every path."""
import functools

import numpy as np

import oracle_py as O
from test_gpu_parity import _field

# every N mod 4 (the one- to four-slot statements), both sides of each occupancy step, and sizes that keep the select form
# (csrc/race_kernel_reg.hip.h reg_step_by_selects: 3, 12, 25) beside neighbours that do not
SIZES = [1, 2, 3, 4, 5, 7, 8, 12, 20, 21, 22, 23, 25, 32]
N_SIMS = 1500
TAIL_SIMS = 64 * 3 + 5          # three full waves and five lanes of a fourth
PIT_WINDOW = 5                  # reference :465: a stop needs remaining_laps > 5


def laps_of(n):
    return 12 + n % 9           # 12 .. 20: the pit window opens and closes inside the race


def seed_of(n):
    return 100 + n


def field(n):
    """test_gpu_parity._field(n) with 12-20 laps, tyres that last 3-5 laps (most cars stop several times, several on the
    same lap), a retirement rate of 1-2 % per lap, tyre-degradation rates on both sides of the rule's 0.85 / 1.1 scalings,
    and no race-interrupting events: a tyre age of 0 at the end of a lap is then a pit stop and nothing else."""
    case = _field(n)
    drivers = list(case['grid_probs'])
    comp = {k: dict(v) for k, v in case['config']['tire_compounds'].items()}
    for name, laps in (('SOFT', 3), ('MEDIUM', 4), ('HARD', 5)):
        comp[name]['optimal_laps'] = laps
    case['config'] = dict(case['config'], total_laps=laps_of(n), tire_compounds=comp, sc_probability=0.0,
                          vsc_probability=0.0, red_flag_probability=0.0)
    case['tire_deg'] = {d: (0.06, 0.05, 0.01)[i % 3] for i, d in enumerate(drivers)}
    case['driver_dnf_rates'] = {d: 0.01 + 0.01 * (i % 2) for i, d in enumerate(drivers)}
    return case


def _optimal_laps(case, comp, drivers):
    """The pit threshold of every (lap, driver) of a trace, reference :454-462."""
    cfg = case['config']
    by_id = np.zeros(max(O.COMPOUND_ID.values()) + 1, np.int64)
    for name, i in O.COMPOUND_ID.items():
        by_id[i] = int(cfg['tire_compounds'].get(name, {}).get('optimal_laps', 30))
    opt = by_id[comp]
    deg = np.array([case['tire_deg'][d] for d in drivers])
    return np.where(deg > 0.05, (opt * 0.85).astype(np.int64), np.where(deg < 0.02, (opt * 1.1).astype(np.int64), opt))


def assert_paths_entered(case, trace):
    """From the oracle's per-lap trace (state at the END of every lap, [sim][lap - 1][driver]): the run contains a pit stop,
    a lap with two stops in one simulation, a retirement in a lap >= 2, a retirement on a lap on which another car of the
    simulation stops, and a car whose tyre age meets its threshold outside the pit window.  (One car alone cannot show
    the two that need a second car.)"""
    drivers = list(case['grid_probs'])
    n, L = len(drivers), case['config']['total_laps']
    age, dnf, comp = trace['age'].astype(np.int64), trace['dnf'].astype(bool), trace['comp']
    running = ~dnf[:, 1:]
    stop = running & (age[:, 1:] == 0)                               # laps 2 .. L
    retire = dnf[:, 1:] & ~dnf[:, :-1]
    assert stop.any(), 'no pit stop'
    assert retire.any(), 'no retirement in a lap >= 2'
    # the age the pit rule saw on laps 2 .. L of a car that did not stop: last lap's + 1, against that lap's compound
    seen = age[:, :-1] + 1
    thr = _optimal_laps(case, comp[:, :-1], drivers)
    lap = np.arange(2, L + 1)[None, :, None]
    outside = running & ~stop & (seen > thr) & (L - lap <= PIT_WINDOW)
    assert outside.any(), 'no tyre age past its threshold outside the pit window'
    assert not (stop & (L - lap <= PIT_WINDOW)).any() and (stop <= (seen > thr)).all()      # (the reading of the trace holds)
    if n >= 2:
        assert (stop.sum(axis=2) >= 2).any(), 'no lap with two stops'
        assert (retire.any(axis=2) & stop.any(axis=2)).any(), 'no retirement on a lap with a stop'


@functools.lru_cache(maxsize=None)
def reference(n, rng=O.RNG_PHILOX, n_sims=N_SIMS):
    """(case, oracle orders, oracle histogram) of field(n), the paths asserted from the oracle's trace.  Read-only."""
    case = field(n)
    ref = O.Problem(case).run(n_sims, rng=rng, seed=seed_of(n), want_orders=True, n_trace=n_sims)
    assert_paths_entered(case, ref['trace'])
    ref['orders'].setflags(write=False)
    ref['hist'].setflags(write=False)
    return case, ref['orders'], ref['hist']
