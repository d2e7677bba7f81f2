"""Independent Python restatement of one race with planned pit stops and lap-time offsets (include/mcgp.h:
mcgp_run_paces), for the tests of RaceSimulator.run_paces.  It is built on strategy_ref's pieces -- the CPU oracle's
Philox (oracle_py.philox) and inverse-normal, resume_ref's grids, states and retirement chains, strategy_ref's Model and
_Race (sort, update_positions, start_state, classify) -- with its own lap 1 and its own lap loop, in which the car's base
pace is the header's: b = base_pace[d]; + the seconds of the LAPS offset that covers the lap; + the seconds of the car's
active UNTIL_STOP offset (from its first_lap until the pit step of the car's first stop on a lap >= first_lap; that lap's
lap time still carries it, its overtakes do not).  b stands where the model reads base_pace[d]: lap 1's base_lap, the lap
time of laps >= 2 and the pace of the three overtake passes; nothing else moves.  Without offsets it must give
strategy_ref's finishing orders (tests/test_paces_host_build.py asserts that first).

plans: as strategy_ref takes them.  offsets: [(driver, kind, first_lap, last_lap, seconds)], kind LAPS / UNTIL_STOP
(last_lap 0)."""
import ctypes as C

import numpy as np

import oracle_py as O
import resume_ref as RR
import strategy_ref as SR

LAPS, UNTIL_STOP = 0, 1                                             # MCGP_PACE_*
FATE_NONE, FATE_STOP, FATE_FLAG, FATE_RETIRED = range(4)            # how a driver's UNTIL_STOP offset ended
PURPOSE_EVENT, PURPOSE_CAR, PURPOSE_OVT = SR.PURPOSE_EVENT, SR.PURPOSE_CAR, SR.PURPOSE_OVT


def laps(driver, first_lap, last_lap, seconds):
    return (driver, LAPS, first_lap, last_lap, seconds)


def until_stop(driver, first_lap, seconds):
    return (driver, UNTIL_STOP, first_lap, 0, seconds)


class _Race(SR._Race):
    """strategy_ref's race with lap 1 and the lap loop restated around the replaced base pace; `carried` = {driver: laps
    whose lap time carried its UNTIL_STOP offset}."""

    def set_offsets(self, offsets):
        self.by_lap, self.until, self.active, self.carried, self.fate = {}, {}, set(), {}, {}
        for d, kind, a, b, sec in offsets:
            if kind == LAPS:
                for lap in range(a, b + 1):
                    assert (lap, d) not in self.by_lap, f'driver {d} has two LAPS offsets on lap {lap}'
                    self.by_lap[lap, d] = sec
            else:
                assert d not in self.until, f'driver {d} has two UNTIL_STOP offsets'
                self.until[d] = (a, sec)
                self.active.add(d)

    def base(self, lap, d):
        b = self.M.base[d]
        if (lap, d) in self.by_lap:
            b = b + self.by_lap[lap, d]
        if d in self.active and lap >= self.until[d][0]:
            b = b + self.until[d][1]
        return b

    def start_grid(self, grid, plans):
        M = self.M
        for pos, d in enumerate(grid):
            d = int(d)
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
        for pos in range(M.n):                                  # lap 1
            d = self.ord[pos]
            w = self.draw(1, PURPOSE_CAR | d)
            if w[0] < M.t_dnf1[d]:
                self.dnf[d] = 1
                continue
            comp, age = self.comp[d], self.age[d]
            tire = age * (M.cdeg[comp] * M.factor[d])
            noise = 0.0 + M.var[d] * SR._normal(w[1])
            base_lap = self.base(1, d) + tire - (110.0 - 110.0) * 0.03 + M.cdelta[comp] - 0.0 + noise
            pf = 0.5 + (pos + 1) * 0.1
            if not pf < 1.5:
                pf = 1.5
            sd = 0.0 + pf * SR._normal(w[2])
            if pos + 1 <= 3 and 1.0 < sd:
                sd = 1.0
            self.cum[d] = 0.0 + (base_lap - sd * 0.5)
            self.age[d] = age + 1
        self.sort()
        self.update_positions(False)
        self.retirements()
        return 2, 0

    def laps(self, first_lap, dd, plans):
        M = self.M
        stops = {d: dict(p[2]) for d, p in plans.items()}
        for lap in range(first_lap, M.L + 1):
            remaining = M.L - lap
            e = self.draw(lap, PURPOSE_EVENT)
            red = e[0] < M.t_red
            sc = not red and e[1] < M.t_sc
            vsc = not red and not sc and e[2] < M.t_vsc
            if red or sc or vsc:
                dec_age = sc or (vsc and e[3] < M.t_vsc_tire)
                newc = SR._stint(M.track, remaining)
                k, leader, prev_nt, tie = 0, 0.0, -1.0, False
                for d in self.ord:
                    if self.dnf[d]:
                        continue
                    t = self.cum[d]
                    if k == 0:
                        leader = t
                    nt = leader + k * 0.1 if red else leader + k * 0.5 if sc else leader + (t - leader) * 0.8
                    tie |= nt == prev_nt
                    prev_nt = nt
                    self.dirty[d] = 0 < nt - leader < M.dirty_thr
                    if red:                                     # a free tyre change, not a stop: no offset is cleared
                        self.age[d], self.comp[d] = 0, newc
                        self.used[d] |= 1 << newc
                    elif dec_age:
                        self.age[d] = max(self.age[d] - 1, 0)
                    self.cum[d] = nt
                    k += 1
                dd = lap + (1 if vsc else 2)
                if tie:
                    self.sort()
            fuel = 110.0 - 1.5 * (lap - 1)
            if not fuel > 0:
                fuel = 0.0
            fuel_effect = (110.0 - fuel) * 0.03
            carry = 0.0
            for i, d in enumerate(list(self.ord)):
                if self.dnf[d]:
                    continue
                ahead_last, carry = carry, self.last[d]
                if self.out[d] == lap:
                    self.dnf[d] = lap
                    continue
                w = self.draw(lap, PURPOSE_CAR | (i >> 2))[i & 3]
                comp, age = self.comp[d], self.age[d]
                tire = age * (M.cdeg[comp] * M.factor[d])
                drs_gain = M.drs_delta if self.drs[d] else 0.0
                noise = 0.0 + M.var[d] * SR._normal(w)
                clean = self.base(lap, d) + tire - fuel_effect + M.cdelta[comp] - drs_gain + noise
                lap_time = clean
                if self.dirty[d] and ahead_last > 0:
                    dirty_time = clean + M.dirty_pen
                    lap_time = ahead_last if ahead_last > dirty_time else dirty_time
                t = self.cum[d] + lap_time
                age += 1
                if d in plans:
                    stop, newc = lap in stops[d], stops[d].get(lap)
                else:
                    stop, newc = age > M.opt[d][comp] and remaining > 5, None
                    if stop:
                        newc = SR._stint(M.track, remaining)
                        used_dry = self.used[d] & 7
                        if M.track == 0 and bin(used_dry).count('1') == 1 and (used_dry >> newc) & 1:
                            avail = 7 & ~used_dry
                            popped = M.pop_sh if avail == 5 else M.pop_mh if avail == 6 else 0
                            if remaining > 20:
                                newc = 1 if avail & 2 else popped
                            else:
                                newc = 0 if avail & 1 else popped
                if stop:
                    t = t + M.pit_loss
                    comp = newc
                    self.used[d] |= 1 << comp
                    age = 0
                    if d in self.active and lap >= self.until[d][0]:        # the stop clears the offset
                        self.active.discard(d)
                        self.carried[d], self.fate[d] = lap - self.until[d][0] + 1, FATE_STOP
                self.cum[d], self.last[d], self.comp[d], self.age[d] = t, lap_time, comp, age
            for pas in range(3):
                self.sort()
                o = self.ord
                pace = lambda d: self.base(lap, d) + (self.dnf[d] if self.dnf[d] else self.age[d]) * M.deg[d]
                cand = []
                for i in range(1, M.n):
                    a, b = o[i - 1], o[i]
                    delta = pace(a) - pace(b)
                    if self.drs[b]:
                        delta += M.drs_delta
                    if not self.dnf[a] and not self.dnf[b] and delta > M.overtake_delta:
                        cand.append(i)
                if not cand:
                    break
                success, words = False, None
                for k, i in enumerate(cand):
                    if k % 4 == 0:
                        words = self.draw(lap, PURPOSE_OVT | (8 * pas + (k >> 2)))
                    db, da = o[i], o[i - 1]
                    delta = pace(da) - pace(db)
                    if self.drs[db]:
                        delta += M.drs_delta
                    prob = delta / 2.0
                    if not prob < 0.5:
                        prob = 0.5
                    if words[k & 3] * (1.0 / 4294967296.0) < prob:
                        nb = self.cum[da] - 0.1
                        if not nb > 0.1:
                            nb = 0.1
                        self.cum[db], self.cum[da] = nb, nb + 0.3
                        success = True
                if not success:
                    break
            self.sort()
            self.update_positions(lap > 2 and lap > dd)
        # the offsets no stop cleared: carried up to the car's retirement, or to the flag
        for d in self.active:
            p = self.until[d][0]
            self.carried[d] = max(self.dnf[d] - p, 0) if self.dnf[d] else M.L - p + 1
            self.fate[d] = FATE_RETIRED if self.dnf[d] else FATE_FLAG


def orders(case, m, seed, sim_offset=0, plans=None, offsets=(), state=None, grids=None, want_fates=False):
    """(finishing orders [m][n], laps carried [m][n]: 0 for a driver without an UNTIL_STOP offset) of simulations
    sim_offset .. sim_offset + m - 1 under `plans` and `offsets`, from the grid (the oracle's sampled grids, or `grids`) or
    from state = (mcgp_race_state arrays, lap, drs_disabled_until).  want_fates: also FATE_* [m][n], how each driver's
    UNTIL_STOP offset ended."""
    M = SR.Model(case)
    plans = plans or {}
    if state is None and grids is None:
        grids = RR.traced_run(case, m, seed, sim_offset)['grids']
    out, carried, fates = np.zeros((m, M.n), np.uint8), np.zeros((m, M.n), np.int64), np.zeros((m, M.n), np.int64)
    for i in range(m):
        r = _Race(M, seed, sim_offset + i)
        r.set_offsets(offsets)
        first, dd = r.start_grid(grids[i], plans) if state is None else r.start_state(*state)
        r.laps(first, dd, plans)
        out[i] = r.classify()
        for d, c in r.carried.items():
            carried[i, d], fates[i, d] = c, r.fate[d]
    return (out, carried, fates) if want_fates else (out, carried)


def carried_counts(carried, L):
    """carried_out [S][n][L + 1] of laps carried [S][N][n]."""
    S, _, n = carried.shape
    out = np.zeros((S, n, L + 1), np.int64)
    for s in range(S):
        for d in range(n):
            out[s, d] = np.bincount(carried[s][:, d], minlength=L + 1)
    return out


def hist_counts(orders_, n):
    """hist_out [S][n][n] of orders [S][N][n]."""
    return np.stack([RR.counts(orders_[s], n) for s in range(orders_.shape[0])])


def with_base_pace(case, add):
    """The case under base_pace[d] + add[d] (add: by driver index, in the order of the case's grid_probs), the sum
    formed here in binary64."""
    names = list(case['grid_probs'])
    return dict(case, base_pace={nm: case['base_pace'][nm] + add[i] for i, nm in enumerate(names)})


# ---------------------------------------------------------------- the C-ABI call for the tests
def c_paces(scenarios):
    """[[(driver, kind, first_lap, last_lap, seconds), ...], ...] -> (pace_count array, mcgp_pace_offset array)."""
    from monte_carlo_gp_amd import _native as N
    flat = [N.McgpPaceOffset(driver=int(d), kind=int(k), first_lap=int(a), last_lap=int(b), seconds=float(s))
            for sc in scenarios for d, k, a, b, s in sc]
    counts = [len(sc) for sc in scenarios]
    return (C.c_uint32 * max(len(counts), 1))(*counts), (N.McgpPaceOffset * max(len(flat), 1))(*flat)


def run_c(case, plans, offsets, n_sims, seed, sim_offset=0, state=None, orders=True, delta=True, carried=True, prob=None,
          grid=None, device=0, fill=0):
    """mcgp_run_paces on a case -> (rc, hist [S][n][n], delta [S][n][2n-1], carried [S][n][L+1], orders [S][N][n] or
    None).  plans / offsets: one entry per scenario (plans None: none anywhere).  state as strategy_ref.run_c's.
    fill: what hist, delta and carried hold before the call (they are accumulated into)."""
    from monte_carlo_gp_amd import _native as N
    prob = prob or RR.problem(case)
    n, S, L = prob.n, len(offsets), int(prob.cfg.total_laps)
    plans = plans if plans is not None else [{}] * S
    assert len(plans) == S
    counts, c_plans = SR.c_plans(plans)
    pcounts, c_offs = c_paces(offsets)
    g = None
    if state is None:
        g = np.ascontiguousarray(grid if grid is not None else O.Problem(case).grid_probs, np.float64)
    cs = RR.c_state(*state) if state is not None else None
    h = np.full((S, n, n), fill, np.uint64)
    dl = np.full((S, n, 2 * n - 1), fill, np.uint64)
    ca = np.full((S, n, L + 1), fill, np.uint64)
    o = np.zeros((S, n_sims, n), np.uint8) if orders else None
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_paces(C.byref(prob.cfg), C.byref(prob.drv),
                                g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None,
                                C.byref(cs) if cs is not None else None, n, S, counts, c_plans, pcounts, c_offs,
                                int(n_sims), int(sim_offset), int(seed), device, u64(h), u64(dl) if delta else None,
                                u64(ca) if carried else None, o.ctypes.data_as(C.POINTER(C.c_uint8)) if orders else None)
    return rc, h.astype(np.int64), dl.astype(np.int64), ca.astype(np.int64), o


def scenarios(first, L, n):
    """The tests' mixed scenarios for a run whose first lap an offset may name is `first`: [(offsets, plans)].  None;
    single-lap ranges at `first`, at L and in between; two ranges of one driver; LAPS plus UNTIL_STOP on one driver on the
    same laps (the order of the two additions); UNTIL_STOP from the lap of a planned stop (c = 1); UNTIL_STOP on a driver
    under the rule (cleared by a rule stop where it stops); UNTIL_STOP on a planned driver whose plan has no stop (carried
    to the flag); drivers 0 and n - 1."""
    mid = (first + L) // 2
    a, z = 0, n - 1
    stop = min(max(mid, 2), L)                  # a lap a plan may stop on
    out = [
        ([], {}),
        ([laps(a, first, first, 0.7), laps(z, L, L, -0.45), laps(a, mid, mid, 1.3)] if mid not in (first, L)
         else [laps(a, first, first, 0.7)] + ([laps(z, L, L, -0.45)] if L > first else []), {}),
        ([laps(a, first, mid, 0.35)] + ([laps(a, mid + 1, L, -0.6)] if mid < L else []) + [laps(z, first, L, 0.21)], {}),
        ([laps(a, first, L, 0.3), until_stop(a, first, 0.1), laps(z, first, L, 0.1), until_stop(z, first, 0.3)], {}),
        ([until_stop(z, first, 0.8), until_stop(a, first, -0.37)], {}),
    ]
    if first <= stop:
        out.append(([until_stop(a, stop, 0.9)], {a: (-1, 0, [(stop, 2)])}))
    out.append(([until_stop(z, first, 0.55), laps(a, first, L, -0.2)], {z: (-1, 0, [])}))
    return out
