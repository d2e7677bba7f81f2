"""numpy restatement of mcgp_run_trace's counts (include/mcgp.h, csrc/trace.hip.h) from the CPU oracle's per-lap trace of
the same simulations (resume_ref.traced_run), and the C-ABI call for the tests.  The race events are restated from the
event draws, telling red flags from safety cars (resume_ref.lap_event lumps them together)."""
import ctypes as C

import numpy as np

import oracle_py as O
import resume_ref as RR
from monte_carlo_gp_amd import _native as N

RED, SC, VSC = 0, 1, 2


def lap_event_kind(case, seed, sim, lap):
    """RED, SC, VSC or None: the short-circuit chain of run_laps, counter {sim, lap, EVENT}."""
    cfg = case['config']
    e = O.philox([sim & 0xFFFFFFFF, sim >> 32, lap, RR.PURPOSE_EVENT], [seed & 0xFFFFFFFF, seed >> 32])
    if e[0] < RR.threshold(cfg['red_flag_probability']):
        return RED
    if e[1] < RR.threshold(cfg['sc_probability']):
        return SC
    if e[2] < RR.threshold(cfg['vsc_probability']):
        return VSC
    return None


def empty(n, L):
    return dict(hist=np.zeros((n, n), np.int64), lap_pos=np.zeros((L, n, n + 1), np.int64),
                laps_led=np.zeros((n, L + 1), np.int64), stops=np.zeros((n, L + 1), np.int64),
                fastest=np.zeros(n, np.int64), events=np.zeros((3, L + 1), np.int64))


def trace_counts(case, m, seed, sim_offset=0):
    """The five count arrays (and the histogram) of simulations sim_offset .. sim_offset + m - 1, from the oracle."""
    ref = RR.traced_run(case, m, seed, sim_offset)
    tr, grids = ref['trace'], ref['grids']
    n = grids.shape[1]
    L = case['config']['total_laps']
    out = empty(n, L)
    out['hist'] = ref['hist'].astype(np.int64)
    rows = np.arange(m)[:, None]
    slot = np.zeros((m, n), np.int64)
    slot[rows, grids] = np.arange(n)[None, :]
    led = np.zeros((m, n), np.int64)
    stops = np.zeros((m, n), np.int64)
    best_t = np.full(m, np.inf)
    best_d = np.full(m, -1)
    for k in range(L):                                     # after lap k + 1
        running = tr['dnf'][:, k, :] == 0
        order = np.lexsort((slot, tr['cum'][:, k, :]), axis=-1)        # (cumulative time, grid slot)
        run_sorted = running[rows, order]
        rank = np.cumsum(run_sorted, axis=1) - 1
        pos = np.empty((m, n), np.int64)
        pos[rows, order] = np.where(run_sorted, rank, n)
        for d in range(n):
            out['lap_pos'][k, d] += np.bincount(pos[:, d], minlength=n + 1)
        led += pos == 0
        if k >= 1:
            stops += running & (tr['age'][:, k, :] == 0)
            # fastest: smallest lap time, ties to the better running position (first in running order), then to the
            # earlier lap (strict <)
            t_sorted = np.where(run_sorted, tr['last'][:, k, :][rows, order], np.inf)
            j = np.argmin(t_sorted, axis=1)
            t = t_sorted[np.arange(m), j]
            better = t < best_t
            best_t = np.where(better, t, best_t)
            best_d = np.where(better, order[np.arange(m), j], best_d)
    for d in range(n):
        out['laps_led'][d] += np.bincount(led[:, d], minlength=L + 1)
        out['stops'][d] += np.bincount(stops[:, d], minlength=L + 1)
    out['fastest'] += np.bincount(best_d[best_d >= 0], minlength=n)
    for i in range(m):
        c = [0, 0, 0]
        for lap in range(2, L + 1):
            kind = lap_event_kind(case, seed, sim_offset + i, lap)
            if kind is not None:
                c[kind] += 1
        for kind in range(3):
            out['events'][kind, c[kind]] += 1
    return out


def run_c(case, n_sims, seed, sim_offset=0, device=0, optional=True, prob=None):
    """mcgp_run_trace on a case -> (rc, counts dict as trace_counts returns)."""
    prob = prob or RR.problem(case)
    g = np.ascontiguousarray(O.Problem(case).grid_probs)
    n, L = prob.n, case['config']['total_laps']
    out = {k: v.astype(np.uint64) for k, v in empty(n, L).items()}
    p = lambda k: out[k].ctypes.data_as(C.POINTER(C.c_uint64))
    opt = lambda k: p(k) if optional else None
    rc = N.lib().mcgp_run_trace(C.byref(prob.cfg), C.byref(prob.drv), g.ctypes.data_as(C.POINTER(C.c_double)), n,
                                int(n_sims), int(sim_offset), int(seed), device, p('hist'), p('lap_pos'), opt('laps_led'),
                                opt('stops'), opt('fastest'), opt('events'))
    return rc, {k: v.astype(np.int64) for k, v in out.items()}


def budget_sims(n, L, cap=0xFFFFFE00):
    """The staging budget of mcgp_run_trace: 512 MiB / (L n) simulations, at most the launch cap, in multiples of 256
    when it can."""
    c = min(cap, max(1, (512 << 20) // (L * n)))
    return c // 256 * 256 if c >= 256 else c


def chunk_sims(n, L, device_round):
    """The documented chunk rule of mcgp_run_trace: the budget, rounded down to whole rounds of the device
    (device_round = grid_blocks x block_threads of a full launch, mcgp_last_launch_info)."""
    c = budget_sims(n, L)
    return c // device_round * device_round if c >= device_round else c


def device_round(device=0):
    """grid_blocks x block_threads after a trace call on `device` (its first chunk's launch) that fills the device."""
    g, b, l = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert N.lib().mcgp_last_launch_info(device, C.byref(g), C.byref(b), C.byref(l)) == 0
    return g.value * b.value
