#!/usr/bin/env python3
"""Emit tools/cmpx_bodies.inc for tools/cmpx_bench.hip: the loop bodies of the comparator microbenchmark on fixed registers
(slot i: time in v[10 + 2 i : 11 + 2 i], payload in v(50 + i)).  Not product code."""
def t(i): return f'v[{10 + 2 * i}:{11 + 2 * i}]'
def lo(i): return f'v{10 + 2 * i}'
def hi(i): return f'v{11 + 2 * i}'
def p(i): return f'v{50 + i}'

def comparator(form, a, b):
    if form == 'A':      # the kernel's form
        return [f'v_cmp_gt_f64 vcc, {t(a)}, {t(b)}', f'v_min_f64 v[72:73], {t(a)}, {t(b)}', f'v_max_f64 {t(b)}, {t(a)}, {t(b)}',
                f'v_cndmask_b32 v74, {p(a)}, {p(b)}, vcc', f'v_cndmask_b32 {p(b)}, {p(b)}, {p(a)}, vcc',
                # (the product writes the minimum in place; here two moves stand in for the renaming the compiler does for free:
                #  they are counted out below by the variant A0, which has them without the comparator)
                f'v_mov_b32 {lo(a)}, v72', f'v_mov_b32 {hi(a)}, v73', f'v_mov_b32 {p(a)}, v74']
    if form == 'A0':
        return [f'v_mov_b32 {lo(a)}, v72', f'v_mov_b32 {hi(a)}, v73', f'v_mov_b32 {p(a)}, v74']
    if form == 'B':
        return [f'v_cmpx_gt_f64 vcc, {t(a)}, {t(b)}', f'v_swap_b32 {lo(a)}, {lo(b)}', f'v_swap_b32 {hi(a)}, {hi(b)}',
                f'v_swap_b32 {p(a)}, {p(b)}', 's_mov_b64 exec, s[20:21]']
    if form == 'C':
        return [f'v_cmp_gt_f64 vcc, {t(a)}, {t(b)}', 's_and_b64 exec, s[20:21], vcc', f'v_swap_b32 {lo(a)}, {lo(b)}',
                f'v_swap_b32 {hi(a)}, {hi(b)}', f'v_swap_b32 {p(a)}, {p(b)}', 's_mov_b64 exec, s[20:21]']
    if form == 'D':      # compare + min/max under the full mask, payload by swap under EXEC
        return [f'v_cmpx_gt_f64 vcc, {t(a)}, {t(b)}', f'v_swap_b32 {p(a)}, {p(b)}', 's_mov_b64 exec, s[20:21]',
                f'v_min_f64 v[72:73], {t(a)}, {t(b)}', f'v_max_f64 {t(b)}, {t(a)}, {t(b)}', f'v_mov_b32 {lo(a)}, v72', f'v_mov_b32 {hi(a)}, v73']
    # the write-back chain of an overtake pass (race_isa.hip.h ovt_commit*): a = the car ahead, b = the car behind, the draw
    # word in the payload register of b, its threshold in v(80 + b); -0.1 in s[24:25], 0.3 in s[26:27], the hit lanes in s[28:29]
    if form == 'S':      # by selects: both new times for every lane, four selects under the success mask
        return [f'v_cmp_lt_u32 vcc, {p(b)}, v{80 + b}', f'v_add_f64 v[72:73], {t(a)}, s[24:25]', 'v_add_f64 v[76:77], v[72:73], s[26:27]',
                f'v_cndmask_b32 {lo(b)}, {lo(b)}, v72, vcc', f'v_cndmask_b32 {hi(b)}, {hi(b)}, v73, vcc',
                f'v_cndmask_b32 {lo(a)}, {lo(a)}, v76, vcc', f'v_cndmask_b32 {hi(a)}, {hi(a)}, v77, vcc', 's_or_b64 s[28:29], s[28:29], vcc']
    if form == 'E':      # under EXEC: the two additions in place on the lanes with a hit
        return [f'v_cmpx_lt_u32 vcc, {p(b)}, v{80 + b}', f'v_add_f64 {t(b)}, {t(a)}, s[24:25]', f'v_add_f64 {t(a)}, {t(b)}, s[26:27]',
                's_or_b64 s[28:29], s[28:29], vcc', 's_mov_b64 exec, s[20:21]']
    raise ValueError(form)

# The lap step's commit of one slot (race_kernel_reg.hip.h, "every running car's lap"; race_isa.hip.h step_commit*): slot i has its
# time in t(i) and its pk word in p(i); LAST in v[100 + 2 i], the clean lap time in v[116 + 2 i] (in: clean, out: lap time), the
# age field in v(124 + i), the pit word in v(128 + i), the word a stop leaves in v(132 + i); the retirement word in v136, the
# carry (last lap of the running car ahead) in v[138:139]; pit_loss s[24:25], the dirty-air penalty s[26:27], the pit window
# s[30:31], the two field masks s32 / s33; {0.0, pit_loss} at LDS address 0 for the select form.
def last(i): return f'v[{100 + 2 * i}:{101 + 2 * i}]'
def lt(i): return f'v[{116 + 2 * i}:{117 + 2 * i}]'
def step_select(i):    # today's form: every lane computes everything, the results are merged by selects
    return [f'v_and_b32 v140, 0x200, {p(i)}', 'v_cmp_eq_u32 s[34:35], 0, v140', f'v_cmp_gt_i64 s[36:37], 0, {last(i)}',
            's_andn2_b64 s[38:39], s[34:35], s[36:37]',
            f'v_lshlrev_b32 v148, 18, {p(i)}', 'v_ashrrev_i32 v148, 31, v148', 'v_and_b32 v142, s26, v148', 'v_and_b32 v143, s27, v148',
            'v_and_b32 v144, v138, v148', 'v_and_b32 v145, v139, v148',
            f'v_cndmask_b32_e64 v138, v138, v{100 + 2 * i}, s[34:35]', f'v_cndmask_b32_e64 v139, v139, v{101 + 2 * i}, s[34:35]',
            f'v_add_f64 {lt(i)}, {lt(i)}, v[142:143]', f'v_max_f64 {lt(i)}, |v[144:145]|, {lt(i)}',
            f'v_cmp_ge_u32 s[40:41], v{124 + i}, v{128 + i}', 's_and_b64 s[40:41], s[40:41], s[38:39]', 's_and_b64 s[40:41], s[40:41], s[30:31]',
            f'v_and_or_b32 v140, {p(i)}, s32, v{132 + i}', f'v_add_u32 v141, 0x10000, {p(i)}', 'v_cndmask_b32_e64 v140, v141, v140, s[40:41]',
            f'v_and_or_b32 v141, {p(i)}, s33, v136', 'v_cndmask_b32_e64 v140, v140, v141, s[36:37]',
            f'v_cndmask_b32_e64 {p(i)}, {p(i)}, v140, s[34:35]',
            f'v_cndmask_b32_e64 v146, 0, v{116 + 2 * i}, s[38:39]', f'v_cndmask_b32_e64 v147, 0, v{117 + 2 * i}, s[38:39]',
            'v_cndmask_b32_e64 v141, 0, 8, s[40:41]', f'ds_read_b64 v[{150 + 2 * i}:{151 + 2 * i}], v141',
            f'v_add_f64 {t(i)}, {t(i)}, v[146:147]']
def step_select_tail(i): return [f'v_add_f64 {t(i)}, {t(i)}, v[{150 + 2 * i}:{151 + 2 * i}]']
def step_test(i, g):   # under EXEC, the compares of slot i into the SGPR pairs of group g (step_commit*: MCGP_STEP_TEST)
    a, d, c, y = (f's[{g + 2 * k}:{g + 2 * k + 1}]' for k in range(4))
    return ['s_mov_b64 exec, s[20:21]', f'v_and_b32 v140, 0x200, {p(i)}', f'v_cmp_eq_u32 {a}, 0, v140', f'v_cmp_gt_i32 {d}, 0, v{101 + 2 * i}',
            f'v_and_b32 v140, 0x2000, {p(i)}', f'v_cmp_ge_u32 {c}, v{124 + i}, v{128 + i}', f'v_cmp_ne_u32 {y}, 0, v140']
def step_write(i, g):  # ... and its writes, each under EXEC = saved & mask (MCGP_STEP_WRITE)
    a, d, c, y = (f's[{g + 2 * k}:{g + 2 * k + 1}]' for k in range(4))
    return [f's_and_b64 exec, s[20:21], {y}', f'v_add_f64 {lt(i)}, {lt(i)}, s[26:27]', f'v_max_f64 {lt(i)}, |v[138:139]|, {lt(i)}',
            f's_and_b64 exec, s[20:21], {a}', f'v_mov_b64 v[138:139], {last(i)}',
            f's_and_b64 {d}, {a}, {d}', f's_xor_b64 {a}, {a}, {d}', f's_and_b64 {c}, {c}, {a}', f's_and_b64 {c}, {c}, s[30:31]',
            f's_and_b64 exec, s[20:21], {a}', f'v_add_f64 {t(i)}, {t(i)}, {lt(i)}', f's_xor_b64 {a}, {a}, {c}',
            f's_and_b64 exec, s[20:21], {c}', f'v_add_f64 {t(i)}, {t(i)}, s[24:25]', f'v_and_or_b32 {p(i)}, {p(i)}, s32, v{132 + i}',
            f's_and_b64 exec, s[20:21], {a}', f'v_add_u32 {p(i)}, 0x10000, {p(i)}',
            f's_and_b64 exec, s[20:21], {d}', f'v_and_or_b32 {p(i)}, {p(i)}, s33, v136']
def step_body(form):
    # both forms: the carry starts at 0, the clean lap time and the age field of every slot are worked out afresh
    ins = ['v_mov_b32 v138, 0', 'v_mov_b32 v139, 0']
    for i in range(4):
        ins += [f'v_add_f64 {lt(i)}, v[{108 + 2 * i}:{109 + 2 * i}], 0.5', f'v_and_b32 v{124 + i}, 0x7ff0000, {p(i)}']
    if form == 'LS':
        for i in range(4): ins += step_select(i)
        ins += ['s_waitcnt lgkmcnt(0)']
        for i in range(4): ins += step_select_tail(i)
    else:              # the order of step_commit4: the compares of slot i + 1 ahead of the writes of slot i
        ins += step_test(0, 34) + step_test(1, 42) + step_write(0, 34) + step_test(2, 34) + step_write(1, 42) + step_test(3, 42)
        ins += step_write(2, 34) + step_write(3, 42) + ['s_mov_b64 exec, s[20:21]']
    # (the carry and the last slot's lap time go into the check value)
    return ins + [f'v_add_f64 {t(12)}, {t(12)}, v[138:139]', f'v_add_f64 {t(12)}, {t(12)}, {lt(3)}']
def step_setup():
    ins = ['v_mov_b32 v136, 0x70200', 's_mov_b32 s24, 0', 's_mov_b32 s25, 0x40340000', 's_mov_b32 s26, 0', 's_mov_b32 s27, 0x3fe00000',
           's_mov_b64 s[30:31], -1', 's_mov_b32 s32, 0xf800e3f8', 's_mov_b32 s33, 0xf800ffff',
           'v_mov_b32 v140, 0', 'v_mov_b32 v142, 0', 'v_mov_b32 v143, 0', 'ds_write_b64 v140, v[142:143]', 'v_mov_b32 v143, 0x40340000',
           'ds_write_b64 v140, v[142:143] offset:8', 's_waitcnt lgkmcnt(0)']
    for i in range(4):   # dirty flag by lane and slot, pit words 3 .. 9 laps, one slot whose car retires in a sixteenth of the lanes
        ins += [f'v_lshrrev_b32 v140, {i}, v70', 'v_and_b32 v140, 1, v140', 'v_lshlrev_b32 v140, 13, v140', f'v_or_b32 {p(i)}, {i << 4}, v140',
                'v_and_b32 v140, 3, v70', f'v_add_u32 v140, {3 + i}, v140', f'v_lshlrev_b32 v{128 + i}, 16, v140',
                f'v_mov_b32 v{132 + i}, 0x{(1 + i % 3) << 10 | 1:x}', f'v_mov_b32 v140, {90 + i}', f'v_cvt_f64_u32 {last(i)}, v140',
                f'v_mov_b32 v140, {88 + i}', f'v_cvt_f64_u32 v[{108 + 2 * i}:{109 + 2 * i}], v140']
    ins += ['v_and_b32 v140, 15, v70', 'v_cmp_eq_u32 vcc, 5, v140', 'v_mov_b32 v141, 0x80000000', 's_nop 1', 'v_cndmask_b32 v141, 0, v141, vcc',
            'v_or_b32 v105, v105, v141']
    return ins

# The lap step's rare writes behind a branch (race_isa.hip.h step_commit*): a chain of the four slots of LE in which stops and
# retirements come as they do in a race -- on few iterations, clustered by iteration, in lanes that change.  The word a stop leaves
# is fetched from an eight-entry rule row (LDS address 64, its base in s23, indexed by the used-set bits of the old pk word) as
# the kernel's load_slot does.  All forms read the same inputs and leave the same check value:
#   LF   today's sequence: the fetch for every slot ahead of the statement, both pit writes under the c mask, the retirement
#        write under the d mask, whether or not a lane of the wave has either
#   LFS  per slot: s_and_b64 c, c, win sets SCC, s_cbranch_scc0 jumps over the pit region (address, fetch, wait, both writes)
#   LFB  per batch: the four c masks (in pairs of their own, s[50:57]) OR-ed, one branch over the four pit regions, which sit at
#        the end of the statement (a stopping lane is in no other write of its slot after the lap time's addition)
#   LFR  per slot: s_and_b64 exec, ex, d sets SCC, s_cbranch_scc0 jumps over the retirement write;  LFSR / LFBR: with S / B
# Rates (the share of slot visits with a stopping lane): r0 the window is closed; r13 every lane stops each 23rd iteration, in three
# groups of lanes an iteration apart (3 / 23); r100 every fourth iteration, in four groups (every iteration has a stop in a
# quarter of the lanes).  Retirements: on every 16th iteration slots 1..3 retire in a sixteenth of the lanes (3 / 64 = 4.7 % of
# slot visits); the DNF bit is cleared at the end of the iteration so that they can retire again.  The lanes that retire never
# stop (their pit word is the largest age), so that a retirement does not shift the phase of a stop.
# Registers beyond step_setup's: rule-row addresses v[142:145], the sign-free high words of LAST v146..v148 (slots 1..3), this
# iteration's sign bit for the retiring lanes v149, their lanes' 0x80000000 in v141 (kept: the F forms do not use v141), s58 scratch.
def stepf_addr(i, dst): return [f'v_lshlrev_b32 {dst}, 2, {p(i)}', f'v_and_or_b32 {dst}, {dst}, 28, s23']
def stepf_pit(i, c, fetch):    # the pit region of slot i under its c mask
    ins = [f's_and_b64 exec, s[20:21], {c}']
    if fetch: ins += stepf_addr(i, 'v140') + [f'ds_read_b32 v{132 + i}, v140']
    ins += [f'v_add_f64 {t(i)}, {t(i)}, s[24:25]']
    if fetch: ins += ['s_waitcnt lgkmcnt(0)']
    return ins + [f'v_and_or_b32 {p(i)}, {p(i)}, s32, v{132 + i}']
def stepf_write(i, g, form):
    a, d, c, y = (f's[{g + 2 * k}:{g + 2 * k + 1}]' for k in range(4))
    S, B, R = 'S' in form, 'B' in form, 'R' in form
    if B: c = f's[{50 + 2 * i}:{51 + 2 * i}]'
    ins = [f's_and_b64 exec, s[20:21], {y}', f'v_add_f64 {lt(i)}, {lt(i)}, s[26:27]', f'v_max_f64 {lt(i)}, |v[138:139]|, {lt(i)}',
           f's_and_b64 exec, s[20:21], {a}', f'v_mov_b64 v[138:139], {last(i)}',
           f's_and_b64 {d}, {a}, {d}', f's_xor_b64 {a}, {a}, {d}']
    if not (S or B):     # today's order (MCGP_STEP_WRITE of the parent)
        ins += [f's_and_b64 {c}, {c}, {a}', f's_and_b64 {c}, {c}, s[30:31]', f's_and_b64 exec, s[20:21], {a}', f'v_add_f64 {t(i)}, {t(i)}, {lt(i)}',
                f's_xor_b64 {a}, {a}, {c}'] + stepf_pit(i, c, False)
    else:                # the mask's last AND directly ahead of the branch: every scalar instruction in between would set SCC anew
        ins += [f's_and_b64 exec, s[20:21], {a}', f'v_add_f64 {t(i)}, {t(i)}, {lt(i)}', f's_and_b64 {c}, {c}, {a}', f's_and_b64 {c}, {c}, s[30:31]']
        if S: ins += ['s_cbranch_scc0 2f', f's_xor_b64 {a}, {a}, {c}'] + stepf_pit(i, c, True) + ['2:']
        else: ins += [f's_xor_b64 {a}, {a}, {c}']
    ins += [f's_and_b64 exec, s[20:21], {a}', f'v_add_u32 {p(i)}, 0x10000, {p(i)}', f's_and_b64 exec, s[20:21], {d}']
    if R: ins += ['s_cbranch_scc0 3f']
    ins += [f'v_and_or_b32 {p(i)}, {p(i)}, s33, v136']
    if R: ins += ['3:']
    return ins
def stepf_test(i, g, form):
    ins = step_test(i, g)
    if 'B' in form: ins[5] = f'v_cmp_ge_u32 s[{50 + 2 * i}:{51 + 2 * i}], v{124 + i}, v{128 + i}'
    return ins
def stepf_body(form):
    # this iteration's retirements: the sign of LAST in slots 1..3, in the retiring lanes, on every 16th iteration
    ins = ['s_and_b32 s58, s22, 15', 's_cmp_eq_u32 s58, 7', 's_cselect_b32 s58, -1, 0', 'v_and_b32 v149, s58, v141']
    for i in range(1, 4): ins += [f'v_or_b32 v{101 + 2 * i}, v{145 + i}, v149']
    ins += ['v_mov_b32 v138, 0', 'v_mov_b32 v139, 0']
    if not ('S' in form or 'B' in form):
        for i in range(4): ins += stepf_addr(i, f'v{142 + i}') + [f'ds_read_b32 v{132 + i}, v{142 + i}']
    for i in range(4):
        ins += [f'v_add_f64 {lt(i)}, v[{108 + 2 * i}:{109 + 2 * i}], 0.5', f'v_and_b32 v{124 + i}, 0x7ff0000, {p(i)}']
    if not ('S' in form or 'B' in form): ins += ['s_waitcnt lgkmcnt(0)']
    ins += stepf_test(0, 34, form) + stepf_test(1, 42, form) + stepf_write(0, 34, form) + stepf_test(2, 34, form) + stepf_write(1, 42, form)
    ins += stepf_test(3, 42, form) + stepf_write(2, 34, form) + stepf_write(3, 42, form)
    if 'B' in form:
        ins += ['s_or_b64 s[34:35], s[50:51], s[52:53]', 's_or_b64 s[36:37], s[54:55], s[56:57]', 's_or_b64 s[34:35], s[34:35], s[36:37]',
                's_cbranch_scc0 2f']
        for i in range(4): ins += stepf_pit(i, f's[{50 + 2 * i}:{51 + 2 * i}]', True)
        ins += ['2:']
    ins += ['s_mov_b64 exec, s[20:21]']
    for i in range(4): ins += [f'v_and_b32 {p(i)}, 0xfffffdff, {p(i)}']
    return ins + [f'v_add_f64 {t(12)}, {t(12)}, v[138:139]', f'v_add_f64 {t(12)}, {t(12)}, {lt(3)}']
def stepf_setup(rate):
    period, groups = {'r0': (23, 3), 'r13': (23, 3), 'r100': (4, 4)}[rate]
    ins = ['v_mov_b32 v136, 0x70200', 's_mov_b32 s24, 0', 's_mov_b32 s25, 0x40340000', 's_mov_b32 s26, 0', 's_mov_b32 s27, 0x3fe00000',
           f's_mov_b64 s[30:31], {0 if rate == "r0" else -1}', 's_mov_b32 s32, 0xf800e3f8', 's_mov_b32 s33, 0xf800ffff', 's_mov_b32 s23, 64',
           'v_mov_b32 v140, 0']
    for j in range(8):   # the rule row: a compound by entry, the entry's own used set with one more bit
        ins += [f'v_mov_b32 v142, 0x{(1 + j % 3) << 10 | j | 1 << j % 3:x}', f'ds_write_b32 v140, v142 offset:{64 + 4 * j}']
    ins += ['s_waitcnt lgkmcnt(0)',
            # the retiring lanes: lane & 15 == 5
            'v_and_b32 v140, 15, v70', 'v_cmp_eq_u32 vcc, 5, v140', 'v_mov_b32 v141, 0x80000000', 'v_mov_b32 v143, 0x7ff0000', 's_nop 1',
            'v_cndmask_b32 v141, 0, v141, vcc',
            # the lane's group: its age at the start, so that the groups stop an iteration apart
            f'v_mov_b32 v140, 0x{(1 << 32) // groups + 1:x}', 'v_mul_hi_u32 v142, v70, v140', f'v_mul_u32_u24 v142, {groups}, v142',
            'v_sub_u32 v142, v70, v142', 'v_lshlrev_b32 v142, 16, v142']
    for i in range(4):   # dirty flag by lane and slot, the start age, the pit word (the largest age in the retiring lanes)
        ins += [f'v_lshrrev_b32 v140, {i}, v70', 'v_and_b32 v140, 1, v140', 'v_lshlrev_b32 v140, 13, v140', f'v_or_b32 {p(i)}, {i << 4}, v140',
                f'v_or_b32 {p(i)}, {p(i)}, v142', f'v_mov_b32 v140, 0x{(period - 1) << 16:x}', f'v_cndmask_b32 v{128 + i}, v140, v143, vcc',
                f'v_mov_b32 v140, {90 + i}', f'v_cvt_f64_u32 {last(i)}, v140',
                f'v_mov_b32 v140, {88 + i}', f'v_cvt_f64_u32 v[{108 + 2 * i}:{109 + 2 * i}], v140']
    for i in range(1, 4): ins += [f'v_mov_b32 v{145 + i}, v{101 + 2 * i}']
    return ins

# The position update of one slot (race_kernel_reg.hip.h update_positions_reg<N, true>; race_isa.hip.h upd_commit*): slot i has
# its time in t(i) and its pk word in p(i); leader in v[100:101], prev in v[102:103], the two gaps in v[104:107]; the lanes that
# have not met a running car in s[24:25], the dirty-air threshold in s[26:27] (v[114:115] for the select form's VOPC compare), the
# lanes with DRS enabled in s[28:29], the running tests of the four slots in s[34:41], saved & DRS lanes in s[42:43].
def upd_select(i):     # today's form as compiled: leader, prev and the two flag bits merged by six selects, the running test twice
    return [f'v_and_b32 v108, 0x200, {p(i)}', f'v_and_b32 v112, 0x200, {p(i)}', f'v_and_b32 v113, 0xffffdff7, {p(i)}',
            'v_cmp_eq_u32 vcc, 0, v108', 's_and_b64 vcc, vcc, s[24:25]',
            f'v_cndmask_b32 v101, v101, {hi(i)}, vcc', f'v_cndmask_b32 v100, v100, {lo(i)}, vcc',
            f'v_add_f64 v[104:105], {t(i)}, -v[100:101]', 'v_cmp_nlt_f64 vcc, v[104:105], v[114:115]',
            f'v_add_f64 v[106:107], {t(i)}, -v[102:103]', 's_andn2_b64 s[36:37], s[28:29], s[24:25]',
            'v_cmp_gt_f64 s[38:39], 1.0, v[106:107]', 's_and_b64 s[38:39], s[36:37], s[38:39]',
            'v_cndmask_b32_e64 v110, 0, 8, s[38:39]', 's_or_b64 s[40:41], s[24:25], vcc', 'v_cndmask_b32_e64 v109, v111, 0, s[40:41]',
            f'v_or3_b32 {p(i)}, v110, v113, v109', 'v_cmp_ne_u32 vcc, 0, v112',
            f'v_cndmask_b32 v103, {hi(i)}, v103, vcc', f'v_cndmask_b32 v102, {lo(i)}, v102, vcc', 's_and_b64 s[24:25], s[24:25], vcc']
def A(i): return f's[{34 + 2 * i}:{35 + 2 * i}]'
def upd_head(n):       # under the saved mask: the running test of every slot of the statement into an SGPR pair, the two flags cleared
    ins = ['s_and_b64 s[42:43], s[20:21], s[28:29]']
    for i in range(n): ins += [f'v_and_b32 v108, 0x200, {p(i)}', f'v_and_b32 {p(i)}, 0xffffdff7, {p(i)}', f'v_cmp_eq_u32 {A(i)}, 0, v108']
    return ins
def upd_slot(i, first=False):   # one slot under EXEC (MCGP_UPD_SLOT; first: MCGP_UPD_SLOT_FIRST, slot 0 of the field)
    if first: return [f'v_mov_b64 v[100:101], {t(i)}', f'v_mov_b64 v[102:103], {t(i)}', f's_andn2_b64 s[24:25], s[20:21], {A(i)}']
    return ['s_and_b64 exec, s[20:21], s[24:25]', f'v_mov_b64 v[100:101], {t(i)}', 's_andn2_b64 exec, s[20:21], s[24:25]',
            f'v_add_f64 v[104:105], {t(i)}, -v[100:101]', f'v_add_f64 v[106:107], {t(i)}, -v[102:103]',
            'v_cmpx_gt_f64 vcc, s[26:27], v[104:105]', f'v_or_b32 {p(i)}, 0x2000, {p(i)}', 's_andn2_b64 exec, s[42:43], s[24:25]',
            'v_cmpx_gt_f64 vcc, 1.0, v[106:107]', f'v_or_b32 {p(i)}, 8, {p(i)}',
            f's_and_b64 exec, s[20:21], {A(i)}', f'v_mov_b64 v[102:103], {t(i)}', f's_andn2_b64 s[24:25], s[24:25], {A(i)}']
def upd_body(form):
    # all forms: no running car met yet, leader and prev start at 0
    ins = ['s_mov_b64 s[24:25], s[20:21]', 'v_mov_b32 v100, 0', 'v_mov_b32 v101, 0', 'v_mov_b32 v102, 0', 'v_mov_b32 v103, 0']
    if form == 'US':
        for i in range(4): ins += upd_select(i)
    else:              # UE: upd_commit4<.., false>, a statement further down the field; UF: upd_commit4<.., true>, the one that opens it
        ins += upd_head(4)
        for i in range(4): ins += upd_slot(i, first=form == 'UF' and i == 0)
        ins += ['s_mov_b64 exec, s[20:21]']
    # (leader and prev go into the check value; the times move on, so the lanes of the masks change from one iteration to the next)
    return ins + [f'v_add_f64 {t(12)}, {t(12)}, v[100:101]', f'v_add_f64 {t(12)}, {t(12)}, v[102:103]',
                  f'v_add_f64 {t(1)}, {t(1)}, 0.5', f'v_add_f64 {t(2)}, {t(2)}, 1.0', f'v_add_f64 {t(3)}, {t(3)}, 2.0']
def upd_setup():
    # threshold 6.0; DRS off in a quarter of the lanes; slot 0 retired in a quarter of the lanes (a retired car in front of the first
    # running one), slot 1 in an eighth (all of them behind a retired slot 0: two in front), slot 2 in half (a retired car between two running ones)
    ins = ['s_mov_b32 s26, 0', 's_mov_b32 s27, 0x40180000', 's_mov_b32 s28, 0x77777777', 's_mov_b32 s29, 0x77777777', 'v_mov_b32 v111, 0x2000',
           'v_mov_b32 v114, 0', 'v_mov_b32 v115, 0x40180000']
    for i, (mask, want) in enumerate(((3, 1), (7, 5), (4, 4), (0, 1))):
        ins += [f'v_and_b32 v108, {mask}, v70', f'v_cmp_eq_u32 vcc, {want}, v108', 'v_mov_b32 v109, 0x200', 's_nop 1',
                'v_cndmask_b32 v109, 0, v109, vcc', f'v_or_b32 {p(i)}, {i << 4}, v109']
    return ins

# The threshold stage of an overtake pass (race_kernel_reg.hip.h, "overtakes: draw words"; race_isa.hip.h ovt_threshold /
# ovt_threshold_x): a chain of 19 adjacent pairs.  Pair i has its pace delta in v[10 + 2 i : 11 + 2 i], its threshold in v(50 + i),
# its draw word in v(80 + i); the W-plane row address runs in v100 (v101: the advanced one of the select form), the ceiling in
# v[102:103]; overtake_delta in s[24:25].  The plane (21 rows of 256 words at LDS address 0) holds a word per (lane, row).
# The deltas are lane * 5 + pair * 11 mod 32, plus a half, against a bound of 26.5: 5 pairs in 32 are candidates, in
# different pairs from lane to lane.
T_PAIRS = 19
def dl(i): return f'v[{10 + 2 * i}:{11 + 2 * i}]'
def thr_select(i):     # today's form: threshold and advanced row for every lane, two selects; the word read from the row before
    return [f'v_cmp_lt_f64 vcc, s[24:25], {dl(i)}', f'v_ceil_f64 v[102:103], {dl(i)}', f'v_cvt_u32_f64 v{50 + i}, v[102:103]',
            f'v_min_u32 v{50 + i}, 0x80000000, v{50 + i}', 'v_add_u32 v101, 0x400, v100', f'v_cndmask_b32 v{50 + i}, 0, v{50 + i}, vcc',
            f'ds_read_b32 v{80 + i}, v100', 'v_cndmask_b32 v100, v100, v101, vcc']
def thr_exec(i, zero=True):   # under EXEC: zero, fetch, narrow, then threshold and row advance in place on the candidates' lanes
    return ([f'v_mov_b32 v{50 + i}, 0'] if zero else []) + [
            f'ds_read_b32 v{80 + i}, v100', f'v_cmpx_lt_f64 vcc, s[24:25], {dl(i)}', f'v_ceil_f64 v[102:103], {dl(i)}',
            f'v_cvt_u32_f64 v{50 + i}, v[102:103]', f'v_min_u32 v{50 + i}, 0x80000000, v{50 + i}', 'v_add_u32 v100, 0x400, v100',
            's_mov_b64 exec, s[26:27]']
def thr_body(form):
    ins = ['v_lshlrev_b32 v100, 2, v70']
    if form == 'TS':
        for i in range(T_PAIRS): ins += thr_select(i)
    else:
        per = 1 if form == 'TE' else 4        # pairs to a statement: EXEC is saved once per statement
        for i in range(T_PAIRS):
            if i % per == 0: ins += ['s_mov_b64 s[26:27], exec']
            if form == 'TE4Z':                # thresholds zeroed two at a time (the thresholds of two pairs in an aligned register pair)
                if i % 2 == 0 and i + 1 < T_PAIRS: ins += [f'v_mov_b64 v[{50 + i}:{51 + i}], 0']
                ins += thr_exec(i, zero=i % 2 == 0 and i + 1 == T_PAIRS)
            else:
                ins += thr_exec(i)
    return ins + ['s_waitcnt lgkmcnt(0)']
def thr_kernel(form):
    ins = ['v_mbcnt_lo_u32_b32 v70, -1, 0', 'v_mbcnt_hi_u32_b32 v70, -1, v70', 'v_lshlrev_b32 v72, 2, v70', 'v_mov_b32 v73, 0x9e3779b1',
           'v_mul_lo_u32 v73, v73, v70']
    for k in range(T_PAIRS + 2):
        ins += [f'v_add_u32 v74, 0x{k * 0x61c88647 & 0xffffffff:x}, v73', f'ds_write_b32 v72, v74 offset:{k * 0x400}']
    for i in range(T_PAIRS):
        ins += ['v_mul_u32_u24 v71, 5, v70', f'v_add_u32 v71, {i * 11 % 32}, v71', 'v_and_b32 v71, 31, v71', f'v_cvt_f64_u32 {dl(i)}, v71',
                f'v_add_f64 {dl(i)}, {dl(i)}, 0.5']
    ins += ['s_mov_b32 s24, 0', 's_mov_b32 s25, 0x403a8000', 's_waitcnt lgkmcnt(0)', 's_mov_b64 s[20:21], exec', 's_mov_b32 s22, %0', '1:']
    ins += thr_body(form)
    ins += ['s_sub_u32 s22, s22, 1', 's_cmp_lg_u32 s22, 0', 's_cbranch_scc1 1b']
    # (the check value: the last iteration's thresholds, words and final row)
    ins += ['v_mov_b32 v75, v100']
    for i in range(T_PAIRS): ins += [f'v_mad_u32_u24 v75, v75, 31, v{50 + i}', f'v_xor_b32 v75, v75, v{80 + i}']
    ins += ['v_lshrrev_b32 v75, 8, v75', 'v_cvt_f64_u32 v[72:73], v75', 'v_lshlrev_b32 v70, 3, v70', 'global_store_dwordx2 v70, v[72:73], %1',
            's_waitcnt vmcnt(0)']
    print(f'__global__ void __launch_bounds__(256) k_{form}_chain(uint32_t iters, double *out)\n{{\n    asm volatile(')
    for x in ins:
        print(f'        "{x}\\n\\t"')
    tclob = ','.join(f'"v{i}"' for i in list(range(10, 48)) + list(range(50, 69)) + list(range(70, 76)) + list(range(80, 104)))
    print(f'        : : "s"(iters), "s"(out) : {tclob},"vcc","s20","s21","s22","s24","s25","s26","s27","memory");\n}}')

clob = ','.join(f'"v{i}"' for i in list(range(10, 42)) + list(range(50, 66)) + list(range(70, 76))) + ',"vcc","s20","s21","s22","memory"'
step_clob = ','.join(f'"v{i}"' for i in range(76, 160)) + ',' + ','.join(f'"s{i}"' for i in range(23, 50)) + ','
stepf_clob = step_clob + ','.join(f'"s{i}"' for i in range(50, 60)) + ','
# `tools/cmpx_bench_gen.py step` emits the LF.. forms alone, for tools/cmpx_step_bodies.inc (generated where the benchmark is
# built, not kept in the repository: eighteen kernels of some 350 lines)
import sys
STEPF = tuple((f, r) for f in ('LF', 'LFS', 'LFB', 'LFR', 'LFSR', 'LFBR') for r in ('r0', 'r13', 'r100'))
STEP_ONLY = sys.argv[1:] == ['step']
commit_clob = ','.join(f'"v{i}"' for i in (76, 77) + tuple(range(80, 96))) + ',"s24","s25","s26","s27","s28","s29",'
for form in STEPF if STEP_ONLY else ('A', 'A0', 'B', 'C', 'D', 'S', 'E', 'LS', 'LE', 'US', 'UE', 'UF'):
    form, rate = form if isinstance(form, tuple) else (form, None)
    commit = form in 'SE'
    upd = form[0] == 'U'
    step = form in ('LS', 'LE') or upd or rate is not None      # (a body of its own on the step forms' registers)
    for shape in ('chain',) if commit or step else ('layer', 'chain'):
        ins = ['v_mbcnt_lo_u32_b32 v70, -1, 0', 'v_mbcnt_hi_u32_b32 v70, -1, v70', 'v_mov_b32 v72, 0', 'v_mov_b32 v73, 0', 'v_mov_b32 v74, 0']
        for i in range(16):
            ins += [f'v_mul_u32_u24 v71, 13, v70', f'v_add_u32 v71, {i * 7 % 64}, v71', 'v_and_b32 v71, 31, v71', f'v_cvt_f64_u32 {t(i)}, v71', f'v_mov_b32 {p(i)}, {i}']
        if commit:       # words that differ by lane and slot, thresholds that let a quarter of the attempts succeed
            ins += ['v_mov_b32 v71, 0x9e3779b1', 'v_mul_lo_u32 v71, v71, v70']
            for i in range(16):
                ins += [f'v_add_u32 {p(i)}, 0x{i * 0x61c88647 & 0xffffffff:x}, v71', f'v_mov_b32 v{80 + i}, 0x40000000']
            ins += ['s_mov_b32 s24, 0x9999999a', 's_mov_b32 s25, 0xbfb99999', 's_mov_b32 s26, 0x33333333', 's_mov_b32 s27, 0x3fd33333',
                    's_mov_b64 s[28:29], 0']
        if upd: ins += upd_setup()
        elif rate: ins += stepf_setup(rate)
        elif step: ins += step_setup()
        ins += ['s_mov_b64 s[20:21], exec', 's_mov_b32 s22, %0', '1:']
        pairs = [(i, i + 1) for i in range(15)] if shape == 'chain' else [(i, i + 8) for i in range(8)] + [(2 * i, 2 * i + 1) for i in range(8)]
        if upd: ins += upd_body(form)
        elif rate: ins += stepf_body(form)
        elif step: ins += step_body(form)
        for a, b in [] if step else pairs:
            ins += comparator(form, a, b)
        if commit:       # (two of the words move on, so the lanes with a hit change from one iteration to the next)
            ins += [f'v_add_u32 {p(3)}, 0x9e3779b9, {p(3)}', f'v_add_u32 {p(11)}, 0x7f4a7c15, {p(11)}']
        ins += [f'v_add_f64 {t(0)}, {t(0)}, 4.0', f'v_add_f64 {t(9)}, {t(9)}, -2.0', 's_sub_u32 s22, s22, 1', 's_cmp_lg_u32 s22, 0', 's_cbranch_scc1 1b']
        if commit:       # (the hit lanes go into the check value)
            ins += ['v_cndmask_b32_e64 v74, 0, 1, s[28:29]', f'v_add_u32 {p(0)}, {p(0)}, v74']
        ins += ['v_mov_b32 v75, v50'] + [f'v_mad_u32_u24 v75, v75, 31, {p(i)}' for i in range(1, 16)]
        ins += ['v_cvt_f64_u32 v[72:73], v75', f'v_add_f64 v[72:73], v[72:73], {t(3)}', f'v_add_f64 v[72:73], v[72:73], {t(12)}',
                'v_lshlrev_b32 v70, 3, v70', 'global_store_dwordx2 v70, v[72:73], %1', 's_waitcnt vmcnt(0)']
        print(f'__global__ void __launch_bounds__(256) k_{form}{"_" + rate if rate else ""}_{shape}(uint32_t iters, double *out)\n{{\n    asm volatile(')
        for x in ins:
            print(f'        "{x}\\n\\t"')
        print(f'        : : "s"(iters), "s"(out) : {commit_clob if commit else stepf_clob if rate else step_clob if step else ""}{clob});\n}}')
for form in () if STEP_ONLY else ('TS', 'TE', 'TE4', 'TE4Z'):
    thr_kernel(form)
