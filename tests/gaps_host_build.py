"""Host DEBUGGING build of csrc/gaps.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_gaps_kernel<false / true> on the CPU and decode its raw staging by the layout documented at the top of gaps.hip.h.
Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no CPU path."""
import ctypes as C

import numpy as np

import gaps_ref as GR
import kernel_host_build as KH
import resume_ref as RR

FILL = 0xEE             # what the staging holds before the kernel runs (no staged value: 2B <= 128)


def values_from_staging(stage, m, n, L, n_edges, n_pairs, lap0=0):
    """[m][L - lap0][n + 1 + n_pairs] from race_gaps_kernel's raw staging: stage[(lap - lap0 - 1) R + row][simulation], R =
    n + 1 + n_pairs; rows d < n: the driver's bin or B; row n: the lead's bin or B; row n + 1 + p: pair p's column."""
    B, R = n_edges + 1, n + 1 + n_pairs
    b = stage[:(L - lap0) * R, :m].reshape(L - lap0, R, m).astype(np.int64)
    assert b[:, :n + 1].max(initial=0) <= B and b[:, n + 1:].max(initial=0) <= 2 * B
    return b.transpose(2, 0, 1)


def gaps_values(case, n_sims, seed, sim_offset=0, edges=GR.DEFAULT_EDGES, pairs=(), state=None, prob=None):
    """race_gaps_kernel on the host -> (hist [n][n], values [n_sims][recorded laps][n + 1 + P]).  state = (arrays, lap,
    drs_disabled_until) or None (from the grid)."""
    p, g = prob or KH.generic_problem(case)
    n, L = p.n, int(p.cfg.total_laps)
    lap0 = 0 if state is None else int(state[1])
    e, pr = np.ascontiguousarray(edges, np.float64), GR.c_pairs(pairs)
    R = n + 1 + len(pr)
    stride = (n_sims + 255) // 256 * 256
    hist, err = np.zeros((n, n), np.uint64), C.c_char_p()
    stage = np.full((max((L - lap0) * R, 1), stride), FILL, np.uint8)
    cs = RR.c_state(*state) if state is not None else None
    rc = KH.generic_lib().emu_gaps_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                                 C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint32(len(e)), KH._vp(e),
                                 C.c_uint32(len(pr)), KH._vp(pr) if len(pr) else None, C.c_uint64(n_sims),
                                 C.c_uint64(sim_offset), C.c_uint64(seed), KH._vp(hist), KH._vp(stage), C.c_uint64(stride),
                                 C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (stage[:, n_sims:] == FILL).all()                  # nothing written past the chunk
    if L == lap0:
        assert (stage == FILL).all()                          # ... and nothing at all when no lap is left
    return hist.astype(np.int64), values_from_staging(stage, n_sims, n, L, len(e), len(pr), lap0)


def gaps(case, n_sims, seed, sim_offset=0, edges=GR.DEFAULT_EDGES, pairs=(), state=None, prob=None):
    """race_gaps_kernel on the host -> the dict gaps_ref.gap_counts returns."""
    hist, vals = gaps_values(case, n_sims, seed, sim_offset, edges, pairs, state, prob)
    n, L = hist.shape[0], int(case['config']['total_laps'])
    lap0 = L - vals.shape[1]
    full = np.zeros((n_sims, L, vals.shape[2]), np.int64)
    full[:, lap0:] = vals
    out = GR.counts_from_values(full, n, len(edges), len(pairs), lap0)
    out['hist'] = hist
    return out
