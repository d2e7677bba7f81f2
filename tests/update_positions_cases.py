"""Fields that load the paths of the register kernel's position update (csrc/race_isa.hip.h: upd_commit*; csrc/
race_kernel_reg.hip.h: update_positions_distinct, update_positions_reg), shared by tests/test_update_positions_host_build.py
and tests/test_gpu_update_positions.py: the cases, the oracle's results (computed once per process) and the proof from the
oracle's own trace that the chosen seeds enter every path.

Two fields per size.  `close` is step_commit_cases.field(n): base paces 0.2 s apart, so the field stays within DRS and
dirty-air range and retired cars (their times stand still) collect in front of the first running car.  `spread` is the
same field with the base paces spread evenly over 12 s a lap: the field strings out, a car that retires in mid-field is
passed by the cars behind it one after another and sits between two running cars meanwhile (the `prev` path), and gaps
fall on both sides of both bounds.  Either field ends some laps with two running cars on equal times from 12 cars up."""
import functools

import numpy as np

import oracle_py as O
import step_commit_cases as S

# step_commit_cases.SIZES covers every N mod 4 (the one- to four-slot statements, opening the field and further down it)
# and both sides of each occupancy step; with them the sizes that keep the select form (csrc/race_kernel_reg.hip.h
# reg_update_by_selects: 1, 6, 9, 10, 11, 22, 28, 29), each beside a neighbour that does not (2, 5 and 7, 8 and 12, 21 and
# 23, 27)
SIZES = sorted(set(S.SIZES) | {6, 9, 10, 11, 27, 28, 29})
KINDS = ('close', 'spread')
N_SIMS = S.N_SIMS
TAIL_SIMS = S.TAIL_SIMS
seed_of = S.seed_of


def field(n, kind):
    case = S.field(n)
    if kind == 'spread':
        drivers = list(case['grid_probs'])
        case['base_pace'] = {d: 90.0 + 12.0 * i / max(n - 1, 1) for i, d in enumerate(drivers)}
    return case


def paths(case, trace):
    """Lap-ends (laps 2 .. L: the lap loop's calls) of the oracle's trace (state at the END of every lap, [sim][lap - 1][driver])
    that show each path of the position update, counted."""
    cum, tbl = trace['cum'][:, 1:], trace['tbl'][:, 1:]
    dnf, drs = trace['dnf'][:, 1:].astype(bool), trace['drs'][:, 1:].astype(bool)
    thr = case['config']['dirty_air_threshold']
    run = ~dnf
    big = np.finfo(np.float64).max
    lead = np.where(run, cum, big).min(axis=2, keepdims=True)           # the first running car's time
    last = np.where(run, cum, -big).max(axis=2, keepdims=True)          # the last running car's
    behind = run & (cum > lead)                                         # running cars that are not the leader
    order = np.sort(np.where(run, cum, big), axis=2)
    ties = (order[:, :, 1:] == order[:, :, :-1]) & (order[:, :, 1:] < big)
    return dict(
        retired_in_front=int((dnf & (cum < lead) & run.any(axis=2, keepdims=True)).any(axis=2).sum()),
        retired_between=int((dnf & (cum > lead) & (cum < last)).any(axis=2).sum()),
        drs_on=int((behind & drs).sum()), drs_off=int((behind & ~drs).sum()),
        dirty=int((behind & (tbl < thr)).sum()), clean=int((behind & ~(tbl < thr)).sum()),
        equal_times=int(ties.any(axis=2).sum()))


def assert_paths_entered(case, trace, kind):
    """What each field shows at each size (checked on the oracle at N_SIMS simulations, seeds seed_of(n)).  One car alone
    has no path to show, and two cars have none between them.
      close:   a retired car in front of the first running one, DRS on and off, both sides of the dirty-air bound at every
               n >= 2.
      spread:  a retired car between two running cars from n = 3 (n = 3: 48 lap-ends, n = 4: 157, n = 5: 230, n = 20: 715; the
               close field has none up to 20 cars); DRS on and off and both sides of the bound from n = 4.
      both:    two running cars on equal times, the select form's path, from n = 12 (spread: n = 12: 32 lap-ends, n = 20: 203)."""
    n = len(case['grid_probs'])
    got = paths(case, trace)
    want = []
    if kind == 'close' and n >= 2: want += ['retired_in_front', 'drs_on', 'drs_off', 'dirty', 'clean']
    if n >= 12: want += ['equal_times']
    if kind == 'spread' and n >= 3: want += ['retired_between']
    if kind == 'spread' and n >= 4: want += ['drs_on', 'drs_off', 'dirty', 'clean']
    missing = [k for k in want if got[k] == 0]
    assert not missing, f'n = {n}, {kind}: the run does not enter {missing} ({got})'


@functools.lru_cache(maxsize=None)
def reference(n, kind='close', rng=O.RNG_PHILOX, n_sims=N_SIMS):
    """(case, oracle orders, oracle histogram) of field(n, kind), the paths asserted from the oracle's trace.  Read-only."""
    case = field(n, kind)
    ref = O.Problem(case).run(n_sims, rng=rng, seed=seed_of(n), want_orders=True, n_trace=n_sims)
    if n_sims == N_SIMS: assert_paths_entered(case, ref['trace'], kind)
    ref['orders'].setflags(write=False)
    ref['hist'].setflags(write=False)
    return case, ref['orders'], ref['hist']
