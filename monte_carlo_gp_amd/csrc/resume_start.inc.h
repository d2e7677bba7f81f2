// resume_start.inc.h -- the start of one lane's race from a mid-race state: the rows, the field order, the DRS and
// dirty-air flags after lap k, and the retirement laps after k.
//
// Not a header: a run of statements, included in the bodies of race_resume_kernel (resume.hip.h) and
// race_strategy_kernel (strategy.hip.h), as race_start.inc.h is, so that race_resume_kernel's instructions stay what
// they were when the text lived in its body.
// In scope where it is included: `s` (Rows), `e` (LapEnv), `n`, `L`, `st` (ResumeState), `k` (st.lap),
// `drs_disabled_until`, `c0`, `c1`, `seed_lo`, `seed_hi`.

        // ================= the state after lap k, as race_kernel leaves it =================
        for (int d = 0; d < n; ++d) {
            s.Cum(d) = st.cum[d];
            s.Last(d) = st.last[d];
            s.Pk(d) = st.pk[d];
            s.Ord(d) = (uint8_t)d;
        }
        sort_by_time(s, n);
        update_positions(s, n, k > 2 && k > drs_disabled_until, e.dirty_thr);

        // ================= retirements after lap k: race_kernel's draw, redrawn where the state contradicts it =================
        {
            uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
            for (int d = 0; d < n; ++d) {
                if ((d & 3) == 0)
                    philox4x32_10(c0, c1, 0u, kPurposeRetire | (uint32_t)(d >> 2), seed_lo, seed_hi, r0, r1, r2, r3);
                const uint32_t rw = (d & 3) == 0 ? r0 : (d & 3) == 1 ? r1 : (d & 3) == 2 ? r2 : r3;
                uint32_t out = draw_retirement_lap(rw, e.dnf[d], L);
                if (out != 0u && (int)out <= k && !(s.Pk(d) & kDnf)) {
                    uint32_t v0, v1, v2, v3;
                    philox4x32_10(c0, c1, 0u, kPurposeRetire | (8u + (uint32_t)(d >> 2)), seed_lo, seed_hi, v0, v1, v2, v3);
                    const uint32_t vw = (d & 3) == 0 ? v0 : (d & 3) == 1 ? v1 : (d & 3) == 2 ? v2 : v3;
                    out = draw_retirement_lap_after(vw, e.dnf[d], k, L);
                }
                s.Out(d) = (uint16_t)out;
            }
        }
