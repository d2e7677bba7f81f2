"""Host DEBUGGING build of csrc/penalties.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_scenario_kernel<false / true, kRulePenalties> and penalties_count on the CPU and decode the raw staging by the layout documented at
the top of penalties.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no
CPU path."""
import ctypes as C

import numpy as np

import kernel_host_build as KH
import penalties_ref as PR
import resume_ref as RR
import strategy_ref as SR

STAGE_FILL = 0xEE           # what the staging holds before the kernel runs (bit 7 of a staged byte stays 0)
PAD = 4096                  # bytes of fill kept behind the chunk


def lib():
    L = KH.generic_lib()
    L.emu_penalties_run.restype = C.c_int
    return L


def penalties_raw(case, plans, penalties, n_sims, seed, sim_offset=0, state=None, prob=None, grid_x=3, count=True):
    """race_scenario_kernel with penalties (and penalties_count, as grid_x x S blocks of one thread) on the host -> (hist [S][n][n],
    stage [S][n_sims][n], delta [S][n][2n-1], fate [S][n][4]; the last two without their derived centre bin and column
    0, as the device leaves them), after checking that nothing is written past the chunk."""
    p, g = prob or KH.generic_problem(case)
    n, S = p.n, len(penalties)
    plans = plans if plans is not None else [{}] * S
    counts, c_plans = SR.c_plans(plans)
    pcounts, c_pens = PR.c_penalties(penalties)
    cs = RR.c_state(*state) if state is not None else None
    used = S * n_sims * n
    hist, err = np.zeros((S, n, n), np.uint64), C.c_char_p()
    stage = np.full(used + PAD, STAGE_FILL, np.uint8)
    delta, fate = np.zeros((S, n, 2 * n - 1), np.uint64), np.zeros((S, n, 4), np.uint64)
    rc = lib().emu_penalties_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                                 C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint32(S), counts, c_plans,
                                 pcounts, c_pens, C.c_uint64(n_sims), C.c_uint64(sim_offset), C.c_uint64(seed),
                                 KH._vp(hist), KH._vp(stage), KH._vp(delta) if count else None,
                                 KH._vp(fate) if count else None, C.c_uint32(grid_x), C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (stage[used:] == STAGE_FILL).all()                       # nothing written past the chunk
    return hist.astype(np.int64), stage[:used].reshape(S, n_sims, n).copy(), delta.astype(np.int64), fate.astype(np.int64)


def decode(stage):
    """(orders [S][m][n], fates [S][m][n]) of staged bytes [S][m][n]: bits 0-4 the position, bits 5-6 the fate."""
    n = stage.shape[2]
    assert ((stage & 0x80) == 0).all()
    pos = stage & 31
    assert (np.sort(pos, axis=2) == np.arange(n, dtype=np.uint8)).all()            # every row a permutation
    return np.argsort(pos, axis=2).astype(np.uint8), (stage >> 5) & 3


def penalties(case, plans, pens, n_sims, seed, sim_offset=0, state=None, prob=None):
    """-> dict(hist, orders, fates, delta, fate): the emulated kernels' outputs with the host's derived bins filled in
    as the C ABI fills them."""
    hist, stage, delta, fate = penalties_raw(case, plans, pens, n_sims, seed, sim_offset, state, prob)
    orders, fates = decode(stage)
    n = stage.shape[2]
    assert (delta[:, :, n - 1] == 0).all() and (fate[:, :, 0] == 0).all()
    delta[:, :, n - 1] = n_sims - delta.sum(axis=2)
    fate[:, :, 0] = n_sims - fate.sum(axis=2)
    return dict(hist=hist, orders=orders, fates=fates, delta=delta, fate=fate)
