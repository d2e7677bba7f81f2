"""Host DEBUGGING build of csrc/stints.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_stints_kernel<false / true> on the CPU and decode its raw staging by the layout documented at the top of
stints.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no CPU path."""
import ctypes as C

import numpy as np

import kernel_host_build as KH
import resume_ref as RR
import stints_ref as SR

REC_FILL = 0xEEEEEEEEEEEEEEEE       # what the staging holds before the kernel runs (bits 60 .. 63 of a record stay 0)
POS_FILL = 0xEE                     # (no position: n <= 32)


def lib():
    L = KH.generic_lib()
    L.emu_stints_run.restype = C.c_int
    return L


def decode(rec):
    """The fields of records (any shape, uint64) by the documented layout: dict(stints 1 .. 15, comps [..., 4], stops
    0 .. 15, laps [..., 4])."""
    r = np.asarray(rec, np.uint64)
    f = lambda shift, bits: ((r >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    return dict(stints=f(0, 4), comps=np.stack([f(4 + 3 * j, 3) for j in range(4)], axis=-1), stops=f(16, 4),
                laps=np.stack([f(20 + 10 * k, 10) for k in range(4)], axis=-1), spare=f(60, 4))


def stints_raw(case, n_sims, seed, sim_offset=0, state=None, prob=None):
    """race_stints_kernel on the host -> (hist [n][n], rec [n][n_sims] u64, pos [n][n_sims] u8), after checking that
    nothing is written past the chunk.  state = (arrays, lap, drs_disabled_until) or None (from the grid)."""
    p, g = prob or KH.generic_problem(case)
    n = p.n
    stride = (n_sims + 255) // 256 * 256
    hist, err = np.zeros((n, n), np.uint64), C.c_char_p()
    rec, pos = np.full((n, stride), REC_FILL, np.uint64), np.full((n, stride), POS_FILL, np.uint8)
    cs = RR.c_state(*state) if state is not None else None
    rc = lib().emu_stints_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                              C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint64(n_sims),
                              C.c_uint64(sim_offset), C.c_uint64(seed), KH._vp(hist), KH._vp(rec), KH._vp(pos),
                              C.c_uint64(stride), C.byref(err))
    assert rc == 0, (rc, err.value)
    assert (rec[:, n_sims:] == REC_FILL).all() and (pos[:, n_sims:] == POS_FILL).all()   # nothing written past the chunk
    return hist.astype(np.int64), rec[:, :n_sims].copy(), pos[:, :n_sims].copy()


def counts_from_staging(rec, pos, L):
    """stop_lap, stops_pos and seq from the raw staging, in numpy."""
    n, m = rec.shape
    f = decode(rec)
    assert (f['spare'] == 0).all() and (f['stints'] >= 1).all() and f['comps'].max(initial=0) <= 4
    assert pos.max(initial=0) < n and (np.sort(pos, axis=0) == np.arange(n, dtype=np.uint8)[:, None]).all()
    kept = np.arange(4)[None, None, :]
    # fields past the stops and stints a record counts stay zero
    assert (np.where(kept < np.minimum(f['stops'], 4)[..., None], 0, f['laps']) == 0).all()
    assert (np.where(kept < np.minimum(f['stints'], 4)[..., None], 0, f['comps']) == 0).all()
    code = sum(np.where(j < f['stints'], (f['comps'][..., j] + 1) * 6 ** j, 0) for j in range(4))
    t = dict(stops=f['stops'].T, code=np.where(f['stints'] > 4, 0, code).T, laps=f['laps'].transpose(1, 0, 2))
    return SR.counts_from_tallies(t, pos.T.astype(np.int64), L)


def stints(case, n_sims, seed, sim_offset=0, state=None, prob=None):
    """race_stints_kernel on the host -> the dict stints_ref.stint_counts returns."""
    hist, rec, pos = stints_raw(case, n_sims, seed, sim_offset, state, prob)
    out = counts_from_staging(rec, pos, int(case['config']['total_laps']))
    out['hist'] = hist
    return out
