"""Host DEBUGGING build of csrc/pit_window.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_window_kernel<false / true> on the CPU and decode its raw staging by the layout documented at the top of
pit_window.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no CPU path."""
import ctypes as C

import numpy as np

import kernel_host_build as KH
import resume_ref as RR
import window_ref as WR

FILL = 0xEE             # what the staging holds before the kernel runs (no staged value: at most 64)


def values_from_staging(stage, m, n, L, n_edges, W, lap0=0):
    """[m][L - lap0][W][5] from race_window_kernel's raw staging: stage[((lap - lap0 - 1) W + w) 5 + row][simulation];
    rows: rejoin, lost, ahead, gap_ahead, gap_behind."""
    b = stage[:(L - lap0) * W * 5, :m].reshape(L - lap0, W, 5, m).astype(np.int64)
    for r, width in enumerate(WR.widths(n, n_edges)[k] for k in WR.ROWS):
        assert b[:, :, r].max(initial=0) < width, (r, width)
    return b.transpose(3, 0, 1, 2)


def window_values(case, n_sims, seed, sim_offset=0, windows=(), edges=WR.DEFAULT_EDGES, state=None, prob=None):
    """race_window_kernel on the host -> (hist [n][n], values [n_sims][recorded laps][W][5]).  windows = [(driver index,
    loss)]; state = (arrays, lap, drs_disabled_until) or None (from the grid)."""
    p, g = prob or KH.generic_problem(case)
    n, L = p.n, int(p.cfg.total_laps)
    lap0 = 0 if state is None else int(state[1])
    e = np.ascontiguousarray(edges, np.float64)
    wd = np.ascontiguousarray([w[0] for w in windows], np.uint8)
    wl = np.ascontiguousarray([w[1] for w in windows], np.float64)
    W = len(wd)
    stride = (n_sims + 255) // 256 * 256
    hist, err = np.zeros((n, n), np.uint64), C.c_char_p()
    stage = np.full((max((L - lap0) * W * 5, 1), stride), FILL, np.uint8)
    cs = RR.c_state(*state) if state is not None else None
    lib = KH.generic_lib()
    lib.emu_window_run.restype = C.c_int
    rc = lib.emu_window_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                            C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint32(len(e)), KH._vp(e),
                            C.c_uint32(W), KH._vp(wd), KH._vp(wl), C.c_uint64(n_sims), C.c_uint64(sim_offset),
                            C.c_uint64(seed), KH._vp(hist), KH._vp(stage), C.c_uint64(stride), C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (stage[:, n_sims:] == FILL).all()                  # nothing written past the chunk
    if L == lap0:
        assert (stage == FILL).all()                          # ... and nothing at all when no lap is left
    return hist.astype(np.int64), values_from_staging(stage, n_sims, n, L, len(e), W, lap0)


def windows_run(case, n_sims, seed, sim_offset=0, windows=(), edges=WR.DEFAULT_EDGES, state=None, prob=None):
    """race_window_kernel on the host -> the dict window_ref.window_counts returns."""
    hist, vals = window_values(case, n_sims, seed, sim_offset, windows, edges, state, prob)
    n, L = hist.shape[0], int(case['config']['total_laps'])
    lap0 = L - vals.shape[1]
    full = np.zeros((n_sims, L) + vals.shape[2:], np.int64)
    full[:, lap0:] = vals
    out = WR.counts_from_values(full, n, len(edges), lap0)
    out['hist'] = hist
    return out
