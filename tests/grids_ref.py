"""Independent Python restatement of one race under edits of the starting grid (include/mcgp.h: mcgp_run_grids), for the
tests of RaceSimulator.run_grids.  It is strategy_ref's race with its own start: the slots of the oracle's drawn grid are
reassigned as the header states it, written with sorted() -- the pit-lane drivers on the last slots in their drawn order,
the pinned drivers on their slots, everybody else by (drawn slot + drop, drawn slot) on the slots left --, the cars are
set up by the new slot, and lap 1 runs on the new grid with the pit-lane seconds added.  Without edits it must give
strategy_ref's finishing orders (tests/test_grids_host_build.py checks that first), which is what makes it a reference for
the edits.

edits: {driver index: (kind, value, seconds)}, kind DROP / PIN / PIT_LANE, value the places or the 1-based slot.
plans: strategy_ref's."""
import ctypes as C

import numpy as np

import oracle_py as O
import resume_ref as RR
import strategy_ref as SR

DROP, PIN, PIT_LANE = 0, 1, 2


def edited_grid(grid, edits):
    """The drivers in the order of their new slots, from the drawn order `grid` (driver on slot 0, 1, ...)."""
    n = len(grid)
    s = {int(d): pos for pos, d in enumerate(grid)}
    pit = sorted((d for d, e in edits.items() if e[0] == PIT_LANE), key=lambda d: s[d])
    pins = {e[1] - 1: d for d, e in edits.items() if e[0] == PIN}
    assert len(pins) == sum(1 for e in edits.values() if e[0] == PIN) and all(p < n - len(pit) for p in pins)
    drop = lambda d: edits[d][1] if d in edits and edits[d][0] == DROP else 0
    rest = sorted((d for d in s if d not in pit and d not in pins.values()), key=lambda d: (s[d] + drop(d), s[d]))
    new = [None] * n
    for k, d in enumerate(pit):
        new[n - len(pit) + k] = d
    for slot, d in pins.items():
        new[slot] = d
    free = [p for p in range(n) if new[p] is None]
    for p, d in zip(free, rest):
        new[p] = d
    assert sorted(new) == list(range(n))
    return new


class _Race(SR._Race):
    def start_grid(self, grid, plans, edits):
        """-> (first lap to run, drs_disabled_until, start compounds by driver)."""
        M = self.M
        new = edited_grid(grid, edits)
        for pos, d in enumerate(new):
            if M.track == 2:
                comp, age = 4, 0
            elif M.track == 1:
                comp, age = 3, 0
            else:
                comp, age = (0, 4) if pos < 10 else (1, 0)
            if d in plans and plans[d][0] >= 0:
                comp, age = plans[d][0], plans[d][1]
            self.comp[d], self.age[d], self.used[d], self.gpos[d] = comp, age, 1 << comp, pos
            self.ord[pos] = d
        start_comp = list(self.comp)
        for pos in range(M.n):                                  # lap 1, on the new grid
            d = self.ord[pos]
            w = self.draw(1, SR.PURPOSE_CAR | d)
            if w[0] < M.t_dnf1[d]:
                self.dnf[d] = 1
                continue
            comp, age = self.comp[d], self.age[d]
            tire = age * (M.cdeg[comp] * M.factor[d])
            noise = 0.0 + M.var[d] * SR._normal(w[1])
            base_lap = M.base[d] + tire - (110.0 - 110.0) * 0.03 + M.cdelta[comp] - 0.0 + noise
            pf = 0.5 + (pos + 1) * 0.1
            if not pf < 1.5:
                pf = 1.5
            sd = 0.0 + pf * SR._normal(w[2])
            if pos + 1 <= 3 and 1.0 < sd:
                sd = 1.0
            t = 0.0 + (base_lap - sd * 0.5)
            if d in edits and edits[d][0] == PIT_LANE:
                t = t + float(edits[d][2])
            self.cum[d] = t
            self.age[d] = age + 1
        self.sort()
        self.update_positions(False)
        self.retirements()
        return 2, 0, start_comp


def orders(case, m, seed, sim_offset=0, plans=None, edits=None, grids=None, want_marks=False):
    """(finishing orders [m][n], start slots by driver [m][n]) of simulations sim_offset .. sim_offset + m - 1 under
    `plans` and `edits`, on the oracle's sampled grids (or `grids`).  want_marks: also every simulation's start compounds
    by driver [m][n]."""
    M = SR.Model(case)
    plans, edits = plans or {}, edits or {}
    if grids is None:
        grids = RR.traced_run(case, m, seed, sim_offset)['grids']
    out, slots, comps = np.zeros((m, M.n), np.uint8), np.zeros((m, M.n), np.int64), np.zeros((m, M.n), np.int64)
    for i in range(m):
        r = _Race(M, seed, sim_offset + i)
        first, dd, comps[i] = r.start_grid(grids[i], plans, edits)
        slots[i] = r.gpos
        r.laps(first, dd, plans)
        out[i] = r.classify()
    return (out, slots, comps) if want_marks else (out, slots)


def hist_counts(orders_, n):
    """hist_out [S][n][n] of orders [S][N][n]."""
    return np.stack([RR.counts(orders_[s], n) for s in range(orders_.shape[0])])


def start_counts(slots, n):
    """start_out [S][n][n] of start slots [S][N][n]."""
    S = slots.shape[0]
    out = np.zeros((S, n, n), np.int64)
    for s in range(S):
        for d in range(n):
            out[s, d] = np.bincount(slots[s][:, d], minlength=n)
    return out


def gain_counts(slots, orders_, n):
    """gain_out [S][n][2n - 1] of start slots [S][N][n] and finishing orders [S][N][n]."""
    S = slots.shape[0]
    pos = np.argsort(orders_, axis=2)                   # pos[s, i, d] = classified position of driver d
    out = np.zeros((S, n, 2 * n - 1), np.int64)
    for s in range(S):
        diff = slots[s] - pos[s] + n - 1
        for d in range(n):
            out[s, d] = np.bincount(diff[:, d], minlength=2 * n - 1)
    return out


# ---------------------------------------------------------------- the C-ABI call for the tests
def c_edits(scenarios):
    """[{driver: (kind, value, seconds)}, ...] -> (edit_count array, mcgp_grid_edit array)."""
    from monte_carlo_gp_amd import _native as N
    flat = [N.McgpGridEdit(driver=int(d), kind=int(k), value=int(v), seconds=float(sec))
            for sc in scenarios for d, (k, v, sec) in sc.items()]
    counts = [len(sc) for sc in scenarios]
    return (C.c_uint32 * max(len(counts), 1))(*counts), (N.McgpGridEdit * max(len(flat), 1))(*flat)


def run_c(case, plans, edits, n_sims, seed, sim_offset=0, orders=True, delta=True, start=True, gain=True, prob=None,
          grid=None, device=0, fill=0):
    """mcgp_run_grids on a case -> (rc, hist [S][n][n], delta [S][n][2n-1], start [S][n][n], gain [S][n][2n-1], orders
    [S][N][n] or None).  plans / edits: one entry per scenario (plans None: none anywhere).  fill: what the counts hold
    before the call (they are accumulated into)."""
    from monte_carlo_gp_amd import _native as N
    prob = prob or RR.problem(case)
    n, S = prob.n, len(edits)
    plans = plans if plans is not None else [{}] * S
    assert len(plans) == S
    counts, c_pl = SR.c_plans(plans)
    ecounts, c_ed = c_edits(edits)
    g = np.ascontiguousarray(grid if grid is not None else O.Problem(case).grid_probs, np.float64)
    h = np.full((S, n, n), fill, np.uint64)
    dl = np.full((S, n, 2 * n - 1), fill, np.uint64)
    st = np.full((S, n, n), fill, np.uint64)
    gn = np.full((S, n, 2 * n - 1), fill, np.uint64)
    o = np.zeros((S, n_sims, n), np.uint8) if orders else None
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_grids(C.byref(prob.cfg), C.byref(prob.drv), g.ctypes.data_as(C.POINTER(C.c_double)), n, S, counts,
                                c_pl, ecounts, c_ed, int(n_sims), int(sim_offset), int(seed), device, u64(h),
                                u64(dl) if delta else None, u64(st) if start else None, u64(gn) if gain else None,
                                o.ctypes.data_as(C.POINTER(C.c_uint8)) if orders else None)
    return rc, h.astype(np.int64), dl.astype(np.int64), st.astype(np.int64), gn.astype(np.int64), o
