"""Fuzz parity of mcgp_run_events on the device: the 100 inputs of generic_cases.run_inputs() under the generated override
sets of events_cases (seeded by the case's name; each set holds an override that contradicts a lap's draw and a planned
stop on a forced safety-car lap) at 8 simulations from the grid, and the 94 resume inputs from the state of simulation 0
after lap L // 2, against the Python restatement (events_ref): finishing orders, hist, delta and events_out.  The empty
scenario is mcgp_run (the product's own race) or mcgp_run_from_state.  The comparison from the grid also runs on the host
build (tests/test_events_host_build.py), so that a failure here splits into kernel text and device build."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch        # noqa: F401  (loaded before the library initialises HIP: afterwards it takes 10 s more)

import events_cases as EC
import events_ref as ER
import generic_cases as G
import oracle_py as O
import resume_ref as RR
import strategy_ref as SR
from helpers import product_run
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

SIMS, STATE_SIMS, OFFSET = 8, 8, 3
KERNEL = 'mcgp::race_events_kernel'


def _run(case, scen, m, seed, off=0, **kw):
    rc, h, dl, ev, o = ER.run_c(case, [pl for _, pl in scen], [ov for ov, _ in scen], m, seed, sim_offset=off, **kw)
    assert rc == 0, N.lib().mcgp_last_error().decode()
    assert N.lib().mcgp_last_kernel_name(0).decode() == KERNEL
    return h, dl, ev, o


@functools.lru_cache(maxsize=None)
def _traced():
    """The oracle's traced run of every run input, made once: [(name, case, seed, ref)]."""
    inputs = G.run_inputs()
    O.lib()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        refs = list(pool.map(lambda a: RR.traced_run(a[1], SIMS, a[2], OFFSET), inputs))
    return [(name, case, seed, ref) for (name, case, seed), ref in zip(inputs, refs)]


def _compare(name, case, scen, m, seed, off, got, **kw):
    n, L = len(case['grid_probs']), case['config']['total_laps']
    h, dl, ev, o = got
    seen = []
    for s, (ov, pl) in enumerate(scen):
        want, sn = ER.orders(case, m, seed, off, plans=pl, overrides=ov, **kw)
        bad = np.nonzero((o[s] != want).any(axis=1))[0]
        assert bad.size == 0, f'{name}, scenario {s}: {bad.size} finishing orders differ, first {bad[:5]}'
        seen.append(sn)
    assert np.array_equal(h, ER.hist_counts(o, n)) and np.array_equal(dl, SR.delta_counts(o, n)), name
    assert np.array_equal(ev, ER.event_counts(np.stack(seen), L)), name
    assert (ev.sum(axis=2) == m).all() and (dl[0, :, n - 1] == m).all(), name
    return o


def test_from_the_grid_on_every_input(require_gpu):
    done = contradicted = stops = moved = 0
    for name, case, seed, ref in _traced():
        scen, c = EC.scenarios(name, case, seed, OFFSET, 2)
        contradicted += c > 0
        stops += len(scen) > 1 and bool(scen[1][1])
        o = _compare(name, case, scen, SIMS, seed, OFFSET, _run(case, scen, SIMS, seed, OFFSET), grids=ref['grids'])
        hist, _, orders = product_run(case, SIMS, seed, sim_offset=OFFSET, orders=True)
        assert np.array_equal(o[0], orders) and np.array_equal(o[0], ref['orders']), name
        moved += any(not np.array_equal(o[s], o[0]) for s in range(1, len(scen)))
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and len(_traced()) == 100
    # every race of two laps or more holds a contradicted lap; most hold a stop under a forced safety car; the overrides
    # change finishing orders on most inputs (not where every car is out on lap 1, or a field of one)
    assert contradicted >= 97 and stops >= 90 and moved >= 80, (contradicted, stops, moved)


def test_from_a_state_on_every_input(require_gpu):
    """From the state of simulation 0 after lap L // 2, into buffers of fives; scenario 0 is mcgp_run_from_state."""
    resume = {name for name, _, _ in G.resume_inputs()}
    done = states = 0
    for name, case, seed, ref in _traced():
        if name not in resume:
            continue
        L = case['config']['total_laps']
        k = max(1, L // 2)
        prob, m = RR.problem(case), STATE_SIMS
        st = (RR.state_arrays(ref, 0, k), k, RR.drs_disabled_until(case, seed, OFFSET, k))
        scen, _ = EC.scenarios(name, case, seed, 0, k + 1)
        h, dl, ev, o = _run(case, scen, m, seed, 0, state=st, prob=prob, fill=5)
        o = _compare(name, case, scen, m, seed, 0, (h - 5, dl - 5, ev - 5, o), state=st)
        rc, hist, orders = RR.run_c(prob, [st], m, [0], seed)
        assert rc == 0 and np.array_equal(o[0], orders[0]) and np.array_equal(h[0] - 5, hist[0]), name
        states += 1
        done += name in G.fuzz_cases()
    assert done == G.N_FUZZ and states >= 94, (done, states)
