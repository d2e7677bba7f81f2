"""Host DEBUGGING build of csrc/moves.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_moves_kernel<false / true> on the CPU and decode its raw staging by the layout documented at the top of
moves.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no CPU path."""
import ctypes as C

import numpy as np

import kernel_host_build as KH
import moves_ref as MR
import resume_ref as RR

FILL = 0x7F                         # what the staging holds before the kernel runs (no position, no slot: n <= 32)
PIT, POS_MASK = KH.TRACE_PIT, KH.TRACE_POS_MASK


def lib():
    L = KH.generic_lib()
    L.emu_moves_run.restype = C.c_int
    return L


def moves_raw(case, n_sims, seed, sim_offset=0, state=None, prob=None):
    """race_moves_kernel on the host -> (hist [n][n], laps [L][n][n_sims] u8, slot [n][n_sims] u8, pos [n][n_sims] u8),
    after checking that nothing is written past the chunk or, from a state, before the baseline row.  state = (arrays,
    lap, drs_disabled_until) or None (from the grid)."""
    p, g = prob or KH.generic_problem(case)
    n, L = p.n, int(case['config']['total_laps'])
    stride = (n_sims + 255) // 256 * 256
    hist, err = np.zeros((n, n), np.uint64), C.c_char_p()
    stage = np.full(((L + 2) * n, stride), FILL, np.uint8)
    cs = RR.c_state(*state) if state is not None else None
    rc = lib().emu_moves_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                             C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint64(n_sims),
                             C.c_uint64(sim_offset), C.c_uint64(seed), KH._vp(hist), KH._vp(stage), C.c_uint64(stride),
                             C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (stage[:, n_sims:] == FILL).all()                                     # nothing written past the chunk
    lap0 = 1 if state is None else int(state[1])
    assert (stage[:(lap0 - 1) * n] == FILL).all()                                # nothing before the baseline row
    assert (stage[(lap0 - 1) * n:, :n_sims] != FILL).all()                       # every later row written
    laps = stage[:L * n, :n_sims].reshape(L, n, n_sims)
    return hist.astype(np.int64), laps.copy(), stage[L * n:(L + 1) * n, :n_sims].copy(), stage[(L + 1) * n:, :n_sims].copy()


def counts_from_staging(laps, slot, pos, lap0, from_grid):
    """Every output but hist from the raw staging, in numpy: the bytes are decoded by the documented layout and handed
    to moves_ref's pair-by-pair counting as a field whose "time" is the staged position."""
    L, n, m = laps.shape
    p = (laps & POS_MASK).astype(np.int64).transpose(2, 0, 1)                    # [m][L][n]
    pit = (laps & PIT) != 0
    live = slice(lap0 - 1, L)
    assert p[:, live].max(initial=0) <= n and not (laps[live] & ~np.uint8(PIT | POS_MASK)).any()
    run = p < n
    # the running positions of a lap are 0 .. r - 1, each once
    srt = np.sort(np.where(run, p, n), axis=2)[:, live]
    assert (srt == np.where(np.arange(n)[None, None, :] < run[:, live].sum(axis=2)[..., None], np.arange(n), n)).all()
    assert not (pit.transpose(2, 0, 1) & ~run)[:, live].any() and not pit[0].any()
    slot, pos = slot.T.astype(np.int64), pos.T.astype(np.int64)
    assert (np.sort(slot, axis=1) == np.arange(n)).all() and (np.sort(pos, axis=1) == np.arange(n)).all()
    # moves_ref orders by (time, slot): the staged position as the time; a retired car's is never read
    age = np.where(pit.transpose(2, 0, 1), 0, 1)
    t = MR.tallies(p.astype(np.float64), (~run).astype(np.int64), age, slot, lap0)
    return MR.counts_from_tallies(t, slot, pos, L, from_grid), t


def moves(case, n_sims, seed, sim_offset=0, state=None, prob=None):
    """race_moves_kernel on the host -> the dict moves_ref.move_counts returns."""
    hist, laps, slot, pos = moves_raw(case, n_sims, seed, sim_offset, state, prob)
    out, _ = counts_from_staging(laps, slot, pos, 1 if state is None else int(state[1]), state is None)
    out['hist'] = hist
    return out
