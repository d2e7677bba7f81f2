"""Host DEBUGGING build of csrc/priors.hip.h (tools/emu/emu_generic.cpp, kernel_host_build.generic_lib): run
race_scenario_kernel<false / true, kRulePriors> and priors_count on the CPU and decode the raw staging by the layout
documented at the top of priors.hip.h.  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and
has no CPU path."""
import ctypes as C

import numpy as np

import kernel_host_build as KH
import priors_ref as QR
import resume_ref as RR
import strategy_ref as SR

STAGE_FILL = 0xEE           # what the byte stagings hold before the kernel runs (no position or bin is 0xEE)
OFF_FILL = np.float32(-77.25)   # ... and the staged offsets (no sigma <= 10 draws it: |z| < 7)
PAD = 4096                  # items of fill kept around each chunk


def lib():
    L = KH.generic_lib()
    L.emu_priors_run.restype = C.c_int
    return L


def priors_raw(case, plans, scenarios, edges, n_sims, seed, sim_offset=0, state=None, prob=None, grid_x=3, count=True,
               want_offsets=True, fill=0):
    """race_scenario_kernel with priors (and priors_count, as grid_x x S x (1 + n) blocks of one thread) on the host ->
    (hist [S][n][n], stage [S][n_sims][n], bins [S][n_sims][n], offsets [S][n_sims][n] float32 or None, delta
    [S][n][2n-1] without its derived centre bin, draws [S][n][B][n]), after checking that nothing is written before or
    past any of the three stagings.  fill: what hist, delta and draws hold before the call (they are accumulated into; it is
    taken off again here)."""
    p, g = prob or KH.generic_problem(case)
    n, S, B = p.n, len(scenarios), len(edges) + 1
    plans = plans if plans is not None else [{}] * S
    counts, c_plans = SR.c_plans(plans)
    pcounts, c_items = QR.c_priors(scenarios)
    keep, e = QR.c_edges(edges)
    cs = RR.c_state(*state) if state is not None else None
    used = S * n_sims * n
    hist, err = np.full((S, n, n), fill, np.uint64), C.c_char_p()
    stage = np.full(PAD + used + PAD, STAGE_FILL, np.uint8)
    bins = np.full(PAD + used + PAD, STAGE_FILL, np.uint8)
    offs = np.full(PAD + used + PAD, OFF_FILL, np.float32)
    delta, draws = np.full((S, n, 2 * n - 1), fill, np.uint64), np.full((S, n, B, n), fill, np.uint64)
    rc = lib().emu_priors_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g) if state is None else None,
                              C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint32(S), counts, c_plans,
                              pcounts, c_items, C.c_uint32(len(edges)), e, C.c_uint64(n_sims), C.c_uint64(sim_offset),
                              C.c_uint64(seed), KH._vp(hist), KH._vp(stage[PAD:]), KH._vp(bins[PAD:]),
                              KH._vp(offs[PAD:]) if want_offsets else None, KH._vp(delta) if count else None,
                              KH._vp(draws) if count else None, C.c_uint32(grid_x), C.byref(err))
    assert rc == 0, (rc, err.value)
    for a, guard in ((stage, STAGE_FILL), (bins, STAGE_FILL), (offs, OFF_FILL)):      # nothing outside the chunk
        assert (a[:PAD] == guard).all() and (a[PAD + used:] == guard).all()
    if not want_offsets:
        assert (offs == OFF_FILL).all()
    cut = lambda a: a[PAD:PAD + used].reshape(S, n_sims, n).copy()
    b = cut(bins)
    assert (b < B).all()
    return (hist.astype(np.int64) - fill, cut(stage), b, cut(offs) if want_offsets else None, delta.astype(np.int64) - fill,
            draws.astype(np.int64) - fill)


def priors(case, plans, scenarios, edges, n_sims, seed, sim_offset=0, state=None, prob=None, **kw):
    """-> dict(hist, orders, bins, offsets, delta, draws): the emulated kernels' outputs with the host's derived centre
    bin filled in as the C ABI fills it."""
    hist, stage, bins, offs, delta, draws = priors_raw(case, plans, scenarios, edges, n_sims, seed, sim_offset, state, prob, **kw)
    n = stage.shape[2]
    assert (np.sort(stage, axis=2) == np.arange(n, dtype=np.uint8)).all()          # every row a permutation
    assert (delta[:, :, n - 1] == 0).all()
    delta[:, :, n - 1] = n_sims - delta.sum(axis=2)
    return dict(hist=hist, orders=np.argsort(stage, axis=2).astype(np.uint8), bins=bins, offsets=offs, delta=delta,
                draws=draws)
