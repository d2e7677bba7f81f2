"""Reference for the tests of mcgp_run_priors (include/mcgp.h) that is not a restatement of its kernel: the drawn offsets
x_d(i) are computed here from the CPU oracle's Philox and inverse-normal (oracle_py.philox, orc_normal_from_u32) in the
header's arithmetic, with numpy's float32 for the one rounding; simulation i of a scenario must then finish as the pinned
C oracle does under base_pace[d] + float(x_d(i)) (the case's base_pace.get(d, 90.0) default resolved before the
addition) and, from a state, as paces_ref's restatement does with a LAPS offset [k + 1, L] of x_d(i) on every driver.

A scenario's items: [('driver', d, sigma), ('group', [d, ...], sigma), ...] by driver index."""
import ctypes as C

import numpy as np

import oracle_py as O
import paces_ref as PR
import resume_ref as RR
import strategy_ref as SR

PURPOSE_PRIOR = 5 << 16
GROUP_BLOCK = 8
DRIVER, GROUP = 0, 1                                               # MCGP_PRIOR_*


def driver(d, sigma):
    return ('driver', int(d), float(sigma))


def group(members, sigma):
    return ('group', [int(d) for d in members], float(sigma))


def deviate(seed, sim, word):
    """z of word `word & 3` of block `word >> 2` of simulation `sim`: a Python float holding a binary32 value."""
    w = O.philox([sim & 0xFFFFFFFF, sim >> 32, 0, PURPOSE_PRIOR | (word >> 2)], [seed & 0xFFFFFFFF, seed >> 32])[word & 3]
    return SR._normal(w)


def offsets_of(items, n, seed, sim):
    """x_d of simulation `sim` under `items`: np.float32 [n]."""
    own, grp = {}, {}
    for it in items:
        if it[0] == 'driver':
            assert it[1] not in own
            own[it[1]] = it[2]
        else:
            for d in it[1]:
                assert d not in grp
                grp[d] = (min(it[1]), it[2])
    x = np.zeros(n, np.float32)
    for d in range(n):
        t = 0.0
        if d in own:
            t = own[d] * deviate(seed, sim, d)
        if d in grp:
            g, sigma = grp[d]
            t = t + sigma * deviate(seed, sim, 4 * GROUP_BLOCK + g)
        x[d] = np.float32(t)
    return x


def offsets(items, n, m, seed, sim_offset=0):
    """[m][n] float32: x of simulations sim_offset .. sim_offset + m - 1."""
    return np.stack([offsets_of(items, n, seed, sim_offset + i) for i in range(m)]) if m else np.zeros((0, n), np.float32)


def with_drawn_pace(case, x):
    """The case under base_pace[d] + float(x_d), the default resolved first."""
    names = list(case['grid_probs'])
    return dict(case, base_pace={nm: case['base_pace'].get(nm, 90.0) + float(x[i]) for i, nm in enumerate(names)})


def orders(case, items, m, seed, sim_offset=0, state=None, x=None):
    """Finishing orders [m][n] of simulations sim_offset .. + m - 1 under `items`: from the grid the pinned C oracle's,
    one simulation at a time under its own base pace; from state = (arrays, lap, drs_disabled_until) paces_ref's."""
    n, L = len(case['grid_probs']), case['config']['total_laps']
    out = np.zeros((m, n), np.uint8)
    for i in range(m):
        xi = x[i] if x is not None else offsets_of(items, n, seed, sim_offset + i)
        if state is None:
            out[i] = O.Problem(with_drawn_pace(case, xi)).run(1, rng=O.RNG_PHILOX, seed=seed, sim_offset=sim_offset + i,
                                                               want_orders=True)['orders'][0]
        else:
            k = state[1]
            offs = [PR.laps(d, k + 1, L, float(xi[d])) for d in range(n)] if k < L else []
            out[i] = PR.orders(case, 1, seed, sim_offset=sim_offset + i, offsets=offs, state=state)[0][0]
    return out


def bins_of(x, edges):
    """searchsorted(edges, x, side='right') in binary64."""
    return np.searchsorted(np.asarray(edges, np.float64), np.asarray(x, np.float64), side='right')


def draw_counts(orders_, x, edges):
    """draws_out [S][n][B][n] of orders [S][m][n] and offsets [S][m][n]."""
    S, m, n = orders_.shape
    B = len(edges) + 1
    out = np.zeros((S, n, B, n), np.int64)
    pos = np.argsort(orders_, axis=2)
    b = bins_of(x, edges)
    for s in range(S):
        for d in range(n):
            np.add.at(out[s, d], (b[s, :, d], pos[s, :, d]), 1)
    return out


def sweep_items(n):
    """The sweep's scenario: own sigma 0.15 on everyone, pair groups (2t, 2t + 1) of sigma 0.2."""
    return [driver(d, 0.15) for d in range(n)] + [group([d for d in (2 * t, 2 * t + 1) if d < n], 0.2)
                                                  for t in range((n + 1) // 2)]


SWEEP_EDGES = (-0.3, -0.1, 0.0, 0.1, 0.3)
SWEEP_SIMS = 8
SWEEP_OFFSET = 1000
_sweep = None


def sweep():
    """[(name, case, seed, items, x [8][n], the oracle's undrawn orders [8][n], its orders under the draws [8][n])] of the
    100 inputs of generic_cases.run_inputs(), computed once and shared (nobody writes into it), after asserting from
    the oracle alone that the sweep is not empty: the draws move an order on at least 80 inputs and a winner on at least
    60, and hit all six bins on at least 85."""
    global _sweep
    if _sweep is None:
        import generic_cases as GC
        out, moved, winner, all_bins = [], 0, 0, 0
        inputs = GC.run_inputs()
        assert len(inputs) == 100
        for name, case, seed in inputs:
            n = len(case['grid_probs'])
            items = sweep_items(n)
            x = offsets(items, n, SWEEP_SIMS, seed, SWEEP_OFFSET)
            base = O.Problem(case).run(SWEEP_SIMS, rng=O.RNG_PHILOX, seed=seed, sim_offset=SWEEP_OFFSET, want_orders=True)['orders']
            want = orders(case, items, SWEEP_SIMS, seed, SWEEP_OFFSET, x=x)
            moved += not np.array_equal(base, want)
            winner += not np.array_equal(base[:, 0], want[:, 0])
            all_bins += len(np.unique(bins_of(x, SWEEP_EDGES))) == len(SWEEP_EDGES) + 1
            out.append((name, case, seed, items, x, base, want))
        print(f'priors sweep: an order moved on {moved} inputs, a winner on {winner}, all six bins hit on {all_bins}')
        assert moved >= 80 and winner >= 60 and all_bins >= 85, (moved, winner, all_bins)
        _sweep = out
    return _sweep


def check_sweep(run):
    """run(case, seed, [[], items]) -> dict(orders, offsets, hist, delta, draws) of SWEEP_SIMS simulations from
    SWEEP_OFFSET under SWEEP_EDGES, compared on every input of sweep()."""
    for name, case, seed, items, x, base, want in sweep():
        n = len(case['grid_probs'])
        got = run(case, seed, [[], items])
        both = np.stack([base, want])
        xs = np.stack([np.zeros_like(x), x])
        assert np.array_equal(got['offsets'].view(np.uint32), xs.view(np.uint32)), name
        assert np.array_equal(got['orders'], both), name
        assert np.array_equal(got['hist'], PR.hist_counts(both, n)), name
        assert np.array_equal(got['delta'], SR.delta_counts(both, n)), name
        assert np.array_equal(got['draws'], draw_counts(both, xs, SWEEP_EDGES)), name


# ---------------------------------------------------------------- the C-ABI call for the tests
def c_priors(scenarios):
    """[[item, ...], ...] -> (prior_count array, mcgp_pace_prior array)."""
    from monte_carlo_gp_amd import _native as N
    flat = []
    for sc in scenarios:
        for it in sc:
            if it[0] == 'driver':
                flat.append(N.McgpPacePrior(kind=DRIVER, driver=it[1], members=0, pad=0, sigma=it[2]))
            else:
                flat.append(N.McgpPacePrior(kind=GROUP, driver=0, members=sum(1 << d for d in it[1]), pad=0, sigma=it[2]))
    counts = [len(sc) for sc in scenarios]
    return (C.c_uint32 * max(len(counts), 1))(*counts), (N.McgpPacePrior * max(len(flat), 1))(*flat)


def c_edges(edges):
    e = np.ascontiguousarray(list(edges) + [0.0], np.float64)
    return e, e.ctypes.data_as(C.POINTER(C.c_double))


def run_c(case, plans, scenarios, edges, n_sims, seed, sim_offset=0, state=None, orders=True, delta=True, draws=True,
          offsets=True, prob=None, device=0, fill=0):
    """mcgp_run_priors on a case -> dict(rc, hist, delta, draws, offsets, orders).  fill: what the count outputs hold
    before the call (they are accumulated into)."""
    from monte_carlo_gp_amd import _native as N
    prob = prob or RR.problem(case)
    n, S, B = prob.n, len(scenarios), len(edges) + 1
    plans = plans if plans is not None else [{}] * S
    counts, c_plans = SR.c_plans(plans)
    pcounts, c_items = c_priors(scenarios)
    keep, e = c_edges(edges)
    g = np.ascontiguousarray(O.Problem(case).grid_probs, np.float64) if state is None else None
    cs = RR.c_state(*state) if state is not None else None
    h = np.full((S, n, n), fill, np.uint64)
    dl = np.full((S, n, 2 * n - 1), fill, np.uint64)
    dr = np.full((S, n, B, n), fill, np.uint64)
    xo = np.full((S, n_sims, n), np.nan, np.float32) if offsets else None
    o = np.full((S, n_sims, n), 0xEE, np.uint8) if orders else None
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_priors(C.byref(prob.cfg), C.byref(prob.drv),
                                 g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None,
                                 C.byref(cs) if cs is not None else None, n, S, counts, c_plans, pcounts, c_items,
                                 len(edges), e, int(n_sims), int(sim_offset), int(seed), device, u64(h),
                                 u64(dl) if delta else None, u64(dr) if draws else None,
                                 xo.ctypes.data_as(C.POINTER(C.c_float)) if offsets else None,
                                 o.ctypes.data_as(C.POINTER(C.c_uint8)) if orders else None)
    return dict(rc=rc, hist=h.astype(np.int64), delta=dl.astype(np.int64), draws=dr.astype(np.int64), offsets=xo, orders=o)
