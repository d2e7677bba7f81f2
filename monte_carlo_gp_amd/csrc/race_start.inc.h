// race_start.inc.h -- the start of one lane's race: grid, cars, lap 1 and the once-per-race retirement draws.
//
// Not a header: a run of statements, included in the bodies of race_kernel (race_kernel.hip.h) and race_trace_kernel
// (trace.hip.h), so that both kernels run one text.  It is text rather than a function because race_kernel must compile
// to the same instructions as before the trace kernel existed, and a function boundary here changes them (LLVM
// simplifies the callee on its own before it inlines it).
// In scope where it is included: `s` (Rows), `e` (LapEnv), `P`, `n`, `L`, `track`, `c0`, `c1`, `seed_lo`, `seed_hi`,
// `fixed_grid` (NULL: the grid is sampled from grid_probs).  Leaves the rows after update_positions of lap 1 and every
// driver's retirement lap (laps >= 2) in `out`.  MCGP_START_OVERRIDE(driver, comp, age) may replace a car's starting
// tyres (race_strategy_kernel, strategy.hip.h); race_kernel.hip.h defines it to expand to nothing.

        // ================= _sample_grid, reference :102-145 =================
        // probs / cdf scratch lives in the `last` rows (not needed until lap 2).
        {
            uint32_t remaining = (n >= 32) ? 0xffffffffu : ((1u << n) - 1u);
            int n_remaining = n;
            uint32_t g0 = 0, g1 = 0, g2 = 0, g3 = 0;
            for (int pos = 0; pos < n; ++pos) {
                uint32_t sel;
                if (fixed_grid) {
                    sel = fixed_grid[pos];
                } else {
                    if ((pos & 3) == 0)
                        philox4x32_10(c0, c1, 0u, kPurposeGrid | (uint32_t)(pos >> 2), seed_lo, seed_hi, g0, g1, g2, g3);
                    const uint32_t gw = (pos & 3) == 0 ? g0 : (pos & 3) == 1 ? g1 : (pos & 3) == 2 ? g2 : g3;
                    const double u = u32_to_unit(gw);
                    double total = 0.0;                                   // :119-123
                    for (int d = 0; d < n; ++d) {
                        const double p = ((remaining >> d) & 1u) ? P->grid_probs[d * n + pos] : 0.0;
                        total = total + p;
                    }
                    double prob_sum = 0.0;                                // :125-133
                    for (int d = 0; d < n; ++d) {
                        const bool rem = (remaining >> d) & 1u;
                        double p;
                        if (total > 0) p = (rem ? P->grid_probs[d * n + pos] : 0.0) / total;
                        else p = rem ? 1.0 / (double)n_remaining : 0.0;
                        s.Last(d) = p;
                        prob_sum = prob_sum + p;
                    }
                    const bool renorm = prob_sum > 0 && fabs(prob_sum - 1.0) > 1e-9;   // :134-135
                    // np.random.choice: cdf = cumsum(p); cdf /= cdf[-1]; searchsorted(u, 'right')
                    double acc = 0.0;
                    for (int d = 0; d < n; ++d) {
                        double p = s.Last(d);
                        if (renorm) p = p / prob_sum;
                        acc = (d == 0) ? p : acc + p;
                        s.Last(d) = acc;
                    }
                    const double cdf_last = acc;
                    sel = 0;
                    for (int d = 0; d < n; ++d)
                        if (s.Last(d) / cdf_last <= u) sel = (uint32_t)d + 1u;
                    if (sel >= (uint32_t)n) sel = (uint32_t)n - 1u;       // unreachable: cdf[-1] == 1 > u
                }
                if ((remaining >> sel) & 1u) { remaining &= ~(1u << sel); --n_remaining; }
                // _initialize_cars, reference :244-273
                uint32_t comp, age;
                if (track == 2) { comp = 4u; age = 0u; }
                else if (track == 1) { comp = 3u; age = 0u; }
                else { comp = pos < 10 ? 0u : 1u; age = pos < 10 ? 4u : 0u; }
                MCGP_START_OVERRIDE(sel, comp, age);
                s.Pk(sel) = age | (comp << kCompShift) | ((1u << comp) << kUsedShift) | ((uint32_t)pos << kGposShift);
                s.Cum(sel) = 0.0;
                s.Ord(pos) = (uint8_t)sel;
            }
            for (int d = 0; d < n; ++d) s.Last(d) = 0.0;
        }

        // ================= _simulate_lap_1, reference :275-311 =================
        for (int pos = 0; pos < n; ++pos) {
            const uint32_t d = s.Ord(pos);
            uint32_t pk = s.Pk(d);
            uint32_t w0, w1, w2, w3;
            philox4x32_10(c0, c1, 1u, kPurposeCar | d, seed_lo, seed_hi, w0, w1, w2, w3);
            if ((uint64_t)w0 < e.dnf1[d]) {
                s.Pk(d) = (pk & ~kAgeMask) | kDnf | 1u;
                continue;
            }
            const uint32_t comp = (pk >> kCompShift) & 7u;
            const uint32_t age = pk & kAgeMask;
            const double eff = e.cdeg[comp] * e.factor[d];
            const double tire = (double)age * eff;
            const double fuel_effect = (110.0 - 110.0) * 0.03;
            const double noise = 0.0 + e.var[d] * (double)normal_from_u32(w1, e.norm);
            const double base_lap = e.base[d] + tire - fuel_effect + e.cdelta[comp] - 0.0 + noise;
            double pf = 0.5 + (double)(pos + 1) * 0.1;
            if (!(pf < 1.5)) pf = 1.5;
            double sd = 0.0 + pf * (double)normal_from_u32(w2, e.norm);
            if (pos + 1 <= 3 && 1.0 < sd) sd = 1.0;
            const double lap_time = base_lap - sd * 0.5;
            s.Cum(d) = 0.0 + lap_time;
            s.Pk(d) = (pk & ~kAgeMask) | (age + 1u);
        }
        sort_by_time(s, n);
        update_positions(s, n, false, e.dirty_thr);

        // ================= retirements of laps 2..L (:190-197), drawn once per race: race_common.hip.h =================
        {
            uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
            for (int d = 0; d < n; ++d) {
                if ((d & 3) == 0)
                    philox4x32_10(c0, c1, 0u, kPurposeRetire | (uint32_t)(d >> 2), seed_lo, seed_hi, r0, r1, r2, r3);
                const uint32_t rw = (d & 3) == 0 ? r0 : (d & 3) == 1 ? r1 : (d & 3) == 2 ? r2 : r3;
                s.Out(d) = (uint16_t)draw_retirement_lap(rw, e.dnf[d], L);
            }
        }
