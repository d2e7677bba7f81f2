"""Independent Python restatement of one race with planned pit stops and race events set on chosen laps (include/mcgp.h:
mcgp_run_events), for the tests of RaceSimulator.run_events.  It is built on strategy_ref's pieces -- the CPU oracle's
Philox (oracle_py.philox) and inverse-normal, resume_ref's grids, states and retirement chains, strategy_ref's Model and
_Race (start, sort, update_positions, classify) -- with its own lap loop, whose event step is the header's: on a lap an
override covers, the outcome of the short-circuit chain is replaced by the override's kind whatever the lap's event words
say; a forced VSC still takes its tyre decrement from word 3; nothing else moves.  Without overrides it must give
strategy_ref's finishing orders (tests/test_events_host_build.py asserts that first).

plans: as strategy_ref takes them.  overrides: [(first_lap, last_lap, kind)], kind NONE / RED / SC / VSC."""
import ctypes as C

import numpy as np

import oracle_py as O
import resume_ref as RR
import strategy_ref as SR

NONE, RED, SC, VSC = 0, 1, 2, 3                                     # MCGP_EVT_*
PURPOSE_EVENT, PURPOSE_CAR, PURPOSE_OVT = SR.PURPOSE_EVENT, SR.PURPOSE_CAR, SR.PURPOSE_OVT


def by_lap(overrides):
    """{lap: kind} of [(first_lap, last_lap, kind)]; overlapping overrides are the caller's mistake."""
    out = {}
    for a, b, kind in overrides:
        for lap in range(a, b + 1):
            assert lap not in out, f'lap {lap} has two overrides'
            out[lap] = kind
    return out


class _Race(SR._Race):
    """strategy_ref's race with the lap loop restated around the replaced event step; `seen` counts the events."""

    def laps(self, first_lap, dd, plans, overrides=()):
        M = self.M
        stops = {d: dict(p[2]) for d, p in plans.items()}
        forced = by_lap(overrides)
        self.seen = [0, 0, 0]                               # red flags, safety cars, VSCs
        for lap in range(first_lap, M.L + 1):
            remaining = M.L - lap
            e = self.draw(lap, PURPOSE_EVENT)
            if lap in forced:
                red, sc, vsc = forced[lap] == RED, forced[lap] == SC, forced[lap] == VSC
            else:
                red = e[0] < M.t_red
                sc = not red and e[1] < M.t_sc
                vsc = not red and not sc and e[2] < M.t_vsc
            if red or sc or vsc:
                self.seen[0 if red else 1 if sc else 2] += 1
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
                    if red:
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
                clean = M.base[d] + tire - fuel_effect + M.cdelta[comp] - drs_gain + noise
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
                self.cum[d], self.last[d], self.comp[d], self.age[d] = t, lap_time, comp, age
            for pas in range(3):
                self.sort()
                o = self.ord
                pace = lambda d: M.base[d] + (self.dnf[d] if self.dnf[d] else self.age[d]) * M.deg[d]
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


def orders(case, m, seed, sim_offset=0, plans=None, overrides=(), state=None, grids=None):
    """(finishing orders [m][n], event laps [m][3]: red flags, safety cars, VSCs) of simulations sim_offset ..
    sim_offset + m - 1 under `plans` and `overrides`, from the grid (the oracle's sampled grids, or `grids`) or from
    state = (mcgp_race_state arrays, lap, drs_disabled_until)."""
    M = SR.Model(case)
    plans = plans or {}
    if state is None and grids is None:
        grids = RR.traced_run(case, m, seed, sim_offset)['grids']
    out, seen = np.zeros((m, M.n), np.uint8), np.zeros((m, 3), np.int64)
    for i in range(m):
        r = _Race(M, seed, sim_offset + i)
        first, dd = r.start_grid(grids[i], plans) if state is None else r.start_state(*state)
        r.laps(first, dd, plans, overrides)
        out[i], seen[i] = r.classify(), r.seen
    return out, seen


def drawn_event(case, seed, sim, lap):
    """(kind, e3 < t_vsc_tire) of the lap's own draw under the case's probabilities: the oracle's short-circuit chain."""
    cfg = case['config']
    e = O.philox([sim & 0xFFFFFFFF, sim >> 32, lap, PURPOSE_EVENT], [seed & 0xFFFFFFFF, seed >> 32])
    dec = e[3] < RR.threshold(0.3)
    if e[0] < RR.threshold(cfg['red_flag_probability']):
        return RED, dec
    if e[1] < RR.threshold(cfg['sc_probability']):
        return SC, dec
    if e[2] < RR.threshold(cfg['vsc_probability']):
        return VSC, dec
    return NONE, dec


def event_counts(seen, L):
    """events_out [S][3][L + 1] of event laps [S][N][3]."""
    S = seen.shape[0]
    out = np.zeros((S, 3, L + 1), np.int64)
    for s in range(S):
        for k in range(3):
            out[s, k] = np.bincount(seen[s][:, k], minlength=L + 1)
    return out


def hist_counts(orders_, n):
    """hist_out [S][n][n] of orders [S][N][n]."""
    return np.stack([RR.counts(orders_[s], n) for s in range(orders_.shape[0])])


def with_probabilities(case, red, sc, vsc):
    """The case under other event probabilities."""
    return dict(case, config=dict(case['config'], red_flag_probability=red, sc_probability=sc, vsc_probability=vsc))


# ---------------------------------------------------------------- the C-ABI call for the tests
def c_events(scenarios):
    """[[(first_lap, last_lap, kind), ...], ...] -> (event_count array, mcgp_lap_event array)."""
    from monte_carlo_gp_amd import _native as N
    flat = [N.McgpLapEvent(first_lap=int(a), last_lap=int(b), kind=int(k)) for sc in scenarios for a, b, k in sc]
    counts = [len(sc) for sc in scenarios]
    return (C.c_uint32 * max(len(counts), 1))(*counts), (N.McgpLapEvent * max(len(flat), 1))(*flat)


def run_c(case, plans, overrides, n_sims, seed, sim_offset=0, state=None, orders=True, delta=True, events=True, prob=None,
          grid=None, device=0, fill=0):
    """mcgp_run_events on a case -> (rc, hist [S][n][n], delta [S][n][2n-1], events [S][3][L+1], orders [S][N][n] or
    None).  plans / overrides: one entry per scenario (plans None: none anywhere).  state as strategy_ref.run_c's.
    fill: what hist, delta and events hold before the call (they are accumulated into)."""
    from monte_carlo_gp_amd import _native as N
    prob = prob or RR.problem(case)
    n, S, L = prob.n, len(overrides), int(prob.cfg.total_laps)
    plans = plans if plans is not None else [{}] * S
    assert len(plans) == S
    counts, c_plans = SR.c_plans(plans)
    ecounts, c_evs = c_events(overrides)
    g = None
    if state is None:
        g = np.ascontiguousarray(grid if grid is not None else O.Problem(case).grid_probs, np.float64)
    cs = RR.c_state(*state) if state is not None else None
    h = np.full((S, n, n), fill, np.uint64)
    dl = np.full((S, n, 2 * n - 1), fill, np.uint64)
    ev = np.full((S, 3, L + 1), fill, np.uint64)
    o = np.zeros((S, n_sims, n), np.uint8) if orders else None
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = N.lib().mcgp_run_events(C.byref(prob.cfg), C.byref(prob.drv),
                                 g.ctypes.data_as(C.POINTER(C.c_double)) if g is not None else None,
                                 C.byref(cs) if cs is not None else None, n, S, counts, c_plans, ecounts, c_evs,
                                 int(n_sims), int(sim_offset), int(seed), device, u64(h), u64(dl) if delta else None,
                                 u64(ev) if events else None, o.ctypes.data_as(C.POINTER(C.c_uint8)) if orders else None)
    return rc, h.astype(np.int64), dl.astype(np.int64), ev.astype(np.int64), o


def scenarios(first, L, n):
    """The tests' mixed scenarios for a run whose first lap with an event step is `first`: [(overrides, plans)].  None;
    each kind on a single lap (`first`, L and in between); a range of safety cars; no event anywhere (contradicts every
    drawn event); a VSC on every lap (contradicts every other draw); a safety car on the lap a plan stops on; a red flag
    on `first` and one on L."""
    mid = (first + L) // 2
    a = 0
    out = [
        ([], {}),
        ([(first, first, SC)], {}),
        ([(L, L, VSC)], {}),
        ([(mid, mid, RED)], {}),
        ([(first, L, NONE)], {}),
        ([(first, L, VSC)], {}),
        ([(mid, mid, SC)], {a: (-1, 0, [(mid, 2)])}),
        ([(first, first, RED)] + ([(L, L, RED)] if L > first else []), {}),
    ]
    if L - first >= 3:
        out.append(([(first, mid - 1, NONE), (mid, min(mid + 2, L), SC)] + ([(mid + 3, L, NONE)] if mid + 3 <= L else []),
                    {n - 1: (-1, 0, [(mid, 1)])}))
    return out
