"""Host DEBUGGING build of csrc/conditions.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_conditions_kernel<false / true> and conditions_count on the CPU and decode the raw staging by the layout documented
at the top of conditions.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has
no CPU path."""
import ctypes as C

import numpy as np

import conditions_ref as CR
import kernel_host_build as KH
import resume_ref as RR

FILL = 0xEE             # what the staging holds before the kernel runs (no driver index: n <= 32)


def staged(case, conds, n_sims, seed, sim_offset=0, state=None, prob=None, count=True, cond_hist=True, grid_x=3,
           table=None):
    """race_conditions_kernel on the host -> dict(hist [n][n], orders [n_sims][n], masks [n_sims] u64) from the raw staging
    (rows p < n: the driver classified p-th, [stride] bytes each; then [stride] u64 masks), and -- count -- conditions_count's
    count [C] and cond_hist [C][n][n] (or None) over grid_x x ceil(C / 8) blocks of one thread.  state = (arrays, lap,
    drs_disabled_until) or None (from the grid).  table: CR.c_conditions(conds), where a caller has it already."""
    p, g = prob or KH.generic_problem(case)
    n, K = p.n, len(conds)
    stride = (n_sims + 255) // 256 * 256
    hist, err = np.zeros((n, n), np.uint64), C.c_char_p()
    stage = np.full((n + 8) * stride, FILL, np.uint8)
    cnt = np.zeros(K, np.uint64) if count else None
    ch = np.zeros((K, n, n), np.uint64) if count and cond_hist else None
    cs = RR.c_state(*state) if state is not None else None
    table = table if table is not None else CR.c_conditions(conds)
    fn = KH.generic_lib().emu_conditions_run
    fn.restype = C.c_int
    rc = fn(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None, C.byref(cs) if cs is not None else None,
            C.c_uint32(n), C.c_uint32(K), table, C.c_uint64(n_sims), C.c_uint64(sim_offset),
            C.c_uint64(seed), KH._vp(hist), KH._vp(stage), C.c_uint64(stride), KH._vp(cnt), KH._vp(ch), C.c_uint32(grid_x),
            C.byref(err))
    assert rc == 0, (rc, err.value)
    rows = stage[:n * stride].reshape(n, stride)
    words = stage[n * stride:].view(np.uint64)
    assert (rows[:, n_sims:] == FILL).all()                                   # nothing written past the chunk
    assert (words[n_sims:] == np.uint64(0xEEEEEEEEEEEEEEEE)).all()
    orders = np.ascontiguousarray(rows[:, :n_sims].T)
    assert (np.sort(orders, axis=1) == np.arange(n, dtype=np.uint8)).all()    # every staged order a permutation
    return dict(hist=hist.astype(np.int64), orders=orders, masks=words[:n_sims].copy(),
                count=None if cnt is None else cnt.astype(np.int64), cond_hist=None if ch is None else ch.astype(np.int64))
