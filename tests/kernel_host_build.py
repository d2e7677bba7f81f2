"""Host DEBUGGING build of the kernel sources (tools/emu): compile, load, run.  Test infrastructure only --
the product (monte_carlo_gp_amd/) never imports this and has no CPU path."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(ROOT, 'tools', 'emu')
LIB = os.path.join(EMU_DIR, 'libmcgp_emu.so')
CSRC = os.path.join(ROOT, 'monte_carlo_gp_amd', 'csrc')

_libs = {}

# named diagnostic variants of the host build: extra -D flags of csrc/race_kernel_reg.hip.h
VARIANTS = {
    None: [],
    'grid_exact': ['-DMCGP_GRID_EXACT=1'],      # _sample_grid takes the exact (dividing) path for every draw
    # the reference-width build decides every event draw and overtake pass with its exact 53-bit code (the path of a draw
    # word equal to the leading word of its threshold, one in 2^32), and reads every deviate's row from device memory
    'wide_exact': ['-DMCGP_WIDE_EXACT=1'],
    # ... a draw word within 2^27 of the leading word of its threshold counts as a tie: a few per cent of the draws
    'wide_near_ties': ['-DMCGP_WIDE_TIE_SHIFT=27'],
}


def build(variant=None):
    LIB = os.path.join(EMU_DIR, 'libmcgp_emu.so' if variant is None else f'libmcgp_emu_{variant}.so')
    tag = '' if variant is None else '_' + variant
    srcs = [os.path.join(EMU_DIR, f) for f in ('emu_kernel.cpp', 'race_isa_host.h', 'hip/hip_runtime.h')]
    srcs += [os.path.join(CSRC, f) for f in ('race_kernel_reg.hip.h', 'race_common.hip.h', 'params_build.h', 'normal_table.h', 'normal53_table.h', 'sort_networks.h')]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(s) for s in srcs):
        # four translation units (field sizes n % 4 == k) compiled side by side, then linked
        flags = ['-O1', '-std=c++17', '-ffp-contract=off', '-fno-fast-math', '-fPIC', '-I' + EMU_DIR, '-DEMU_PARTS=4']
        flags += VARIANTS[variant]
        objs = [os.path.join(EMU_DIR, f'emu_part{k}{tag}.o') for k in range(4)]
        procs = [subprocess.Popen(['g++'] + flags + [f'-DEMU_PART={k}', '-c', '-o', objs[k],
                                                     os.path.join(EMU_DIR, 'emu_kernel.cpp')]) for k in range(4)]
        for pr in procs:
            if pr.wait() != 0:
                raise RuntimeError('host build of the kernel sources failed')
        subprocess.check_call(['g++', '-shared', '-o', LIB] + objs)
    return LIB


def lib(variant=None):
    if variant not in _libs:
        L = C.CDLL(build(variant))
        L.emu_run.restype = C.c_int
        _libs[variant] = L
    return _libs[variant]


def run(case, n_sims, seed, sim_offset=0, set_pop=None, fixed_grid=None, variant=None, deviates=32):
    """(hist, orders) of the kernel source executed on the host for a golden-case dict."""
    from monte_carlo_gp_amd import RaceConfig
    from monte_carlo_gp_amd.simulation import RaceSimulator, _Problem, _dptr
    import oracle_py as O
    drivers = list(case['grid_probs'])
    p = _Problem(RaceConfig(**case['config']), drivers, case['base_pace'], case['tire_deg'], case['driver_variance'],
                 case['driver_dnf_rates'], case['track_condition'], set_pop or O.load_cases()['set_pop'], deviates)
    g = RaceSimulator._grid_matrix(case['grid_probs'], drivers)
    n = p.n
    hist = np.zeros((n, n), np.uint64)
    orders = np.zeros((n_sims, n), np.uint8)
    err = C.c_char_p()
    fg = None
    if fixed_grid is not None:
        fg = np.ascontiguousarray(fixed_grid, np.uint8).ctypes.data_as(C.c_void_p)
    rc = lib(variant).emu_run(C.byref(p.cfg), C.byref(p.drv), _dptr(g), C.c_uint32(n), C.c_uint64(n_sims),
                       C.c_uint64(sim_offset), C.c_uint64(seed), hist.ctypes.data_as(C.c_void_p),
                       orders.ctypes.data_as(C.c_void_p), fg, C.byref(err))
    if rc == -100:
        raise NotServed(err.value.decode())
    assert rc == 0, err.value
    return hist.astype(np.int64), orders


class NotServed(Exception):
    """The register kernel hands this problem to the generic kernel (csrc: reg_kernel_serves)."""


# ---------------------------------------------------------------- the generic kernel family (tools/emu/emu_generic.cpp)
GENERIC_LIB = os.path.join(EMU_DIR, 'libmcgp_emu_generic.so')
TRACE_PIT, TRACE_POS_MASK = 0x80, 0x3F          # csrc/trace.hip.h: kTracePit, kTracePosMask


def build_generic():
    """tools/emu/libmcgp_emu_generic.so: race_kernel, race_resume_kernel, race_trace_kernel, race_scenario_kernel and
    race_gaps_kernel compiled for the host (build()'s flags; rebuilt when one of the product's headers, every csrc/*.h
    and include/mcgp.h, is newer)."""
    srcs = [os.path.join(EMU_DIR, f) for f in ('emu_generic.cpp', 'hip/hip_runtime.h')]
    srcs += glob.glob(os.path.join(CSRC, '*.h')) + [os.path.join(ROOT, 'include', 'mcgp.h')]
    if not os.path.exists(GENERIC_LIB) or os.path.getmtime(GENERIC_LIB) < max(os.path.getmtime(s) for s in srcs):
        tmp = f'{GENERIC_LIB[:-3]}.tmp{os.getpid()}.so'          # (renamed into place: a parallel run never maps half a file)
        subprocess.check_call(['g++', '-O1', '-std=c++17', '-ffp-contract=off', '-fno-fast-math', '-fPIC', '-shared',
                               '-I' + EMU_DIR, '-o', tmp, os.path.join(EMU_DIR, 'emu_generic.cpp')])
        os.replace(tmp, GENERIC_LIB)
    return GENERIC_LIB


def generic_lib():
    if 'generic' not in _libs:
        L = C.CDLL(build_generic())
        for f in ('emu_generic_run', 'emu_generic_resume', 'emu_generic_trace', 'emu_generic_strategy', 'emu_gaps_run'):
            getattr(L, f).restype = C.c_int
        _libs['generic'] = L
    return _libs['generic']


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ok(rc, err):
    assert rc == 0, (rc, err.value)


def generic_problem(case):
    """(the library's problem struct, the dense grid matrix) of a case dict."""
    import oracle_py as O
    import resume_ref as RR
    return RR.problem(case), np.ascontiguousarray(O.Problem(case).grid_probs, np.float64)


def generic_run(case, n_sims, seed, sim_offset=0, fixed_grid=None, prob=None):
    """(hist, orders) of race_kernel on the host; it takes every problem (no reg_kernel_serves here)."""
    p, g = prob or generic_problem(case)
    n = p.n
    hist, orders, err = np.zeros((n, n), np.uint64), np.zeros((n_sims, n), np.uint8), C.c_char_p()
    fg = np.ascontiguousarray(fixed_grid, np.uint8) if fixed_grid is not None else None
    _ok(generic_lib().emu_generic_run(C.byref(p.cfg), C.byref(p.drv), _vp(g), C.c_uint32(n), C.c_uint64(n_sims),
                                      C.c_uint64(sim_offset), C.c_uint64(seed), _vp(hist), _vp(orders), _vp(fg),
                                      C.byref(err)), err)
    return hist.astype(np.int64), orders


def generic_resume(case, states, n_sims, sim_offsets, seed, prob=None):
    """race_resume_kernel on the host: states = [(mcgp_race_state arrays, lap, drs_disabled_until)] ->
    (hist [S][n][n], orders [S][n_sims][n])."""
    import resume_ref as RR
    from monte_carlo_gp_amd import _native as N
    p, _ = prob or generic_problem(case)
    S, n = len(states), p.n
    cs = (N.McgpRaceState * S)(*[RR.c_state(a, k, dd) for a, k, dd in states])
    offs = (C.c_uint64 * S)(*[int(x) for x in sim_offsets])
    hist, orders, err = np.zeros((S, n, n), np.uint64), np.zeros((S, n_sims, n), np.uint8), C.c_char_p()
    _ok(generic_lib().emu_generic_resume(C.byref(p.cfg), C.byref(p.drv), C.c_uint32(n), C.c_uint32(S), cs,
                                         C.c_uint64(n_sims), offs, C.c_uint64(seed), _vp(hist), _vp(orders),
                                         C.byref(err)), err)
    return hist.astype(np.int64), orders


def trace_counts_from_staging(stage, rec, m, n, L):
    """mcgp_run_trace's five count arrays from race_trace_kernel's raw output, by the layout documented at the top of
    csrc/trace.hip.h: stage[(lap - 1) n + driver][simulation] = running position or n, | kTracePit; rec[simulation] =
    fastest-lap driver (0xFFFF: none) | red flags << 16 | safety cars << 32 | VSCs << 48."""
    b = stage[:, :m].reshape(L, n, m)
    assert ((b & ~np.uint8(TRACE_PIT | TRACE_POS_MASK)) == 0).all()
    pos = (b & TRACE_POS_MASK).astype(np.int64)
    assert pos.max() <= n
    out = dict(lap_pos=np.zeros((L, n, n + 1), np.int64), laps_led=np.zeros((n, L + 1), np.int64),
               stops=np.zeros((n, L + 1), np.int64), fastest=np.zeros(n, np.int64), events=np.zeros((3, L + 1), np.int64))
    for k in range(L):
        for d in range(n):
            out['lap_pos'][k, d] = np.bincount(pos[k, d], minlength=n + 1)
    led, stops = (pos == 0).sum(axis=0), ((b & TRACE_PIT) != 0).sum(axis=0)          # [n][m]
    for d in range(n):
        out['laps_led'][d] = np.bincount(led[d], minlength=L + 1)
        out['stops'][d] = np.bincount(stops[d], minlength=L + 1)
    rec = rec[:m]
    f = (rec & np.uint64(0xFFFF)).astype(np.int64)
    assert ((f < n) | (f == 0xFFFF)).all()
    out['fastest'] = np.bincount(f[f < n], minlength=n)
    for kind in range(3):
        c = ((rec >> np.uint64(16 * (kind + 1))) & np.uint64(0xFFFF)).astype(np.int64)
        out['events'][kind] = np.bincount(c, minlength=L + 1)
    return out


def generic_trace(case, n_sims, seed, sim_offset=0, prob=None):
    """race_trace_kernel on the host -> the dict trace_ref.trace_counts returns (hist and the five count arrays)."""
    p, g = prob or generic_problem(case)
    n, L = p.n, int(p.cfg.total_laps)
    stride = (n_sims + 255) // 256 * 256
    hist, err = np.zeros((n, n), np.uint64), C.c_char_p()
    stage, rec = np.full((L * n, stride), 0x7F, np.uint8), np.zeros(stride, np.uint64)
    _ok(generic_lib().emu_generic_trace(C.byref(p.cfg), C.byref(p.drv), _vp(g), C.c_uint32(n), C.c_uint64(n_sims),
                                        C.c_uint64(sim_offset), C.c_uint64(seed), _vp(hist), _vp(stage),
                                        C.c_uint64(stride), _vp(rec), C.byref(err)), err)
    assert (stage[:, n_sims:] == 0x7F).all() and (rec[n_sims:] == 0).all()       # nothing written past the chunk
    out = trace_counts_from_staging(stage, rec, n_sims, n, L)
    out['hist'] = hist.astype(np.int64)
    return out


def generic_strategy(case, scenarios, n_sims, seed, sim_offset=0, state=None, prob=None):
    """race_scenario_kernel<false, 0> (state None) or <true, 0> on the host: scenarios as strategy_ref.c_plans takes them ->
    (hist [S][n][n], orders [S][n_sims][n])."""
    import resume_ref as RR
    import strategy_ref as SR
    p, g = prob or generic_problem(case)
    n, S = p.n, len(scenarios)
    counts, plans = SR.c_plans(scenarios)
    cs = RR.c_state(*state) if state is not None else None
    hist, pos, err = np.zeros((S, n, n), np.uint64), np.full((S, n_sims, n), 0xFF, np.uint8), C.c_char_p()
    _ok(generic_lib().emu_generic_strategy(C.byref(p.cfg), C.byref(p.drv), _vp(g) if state is None else None,
                                           C.byref(cs) if cs is not None else None, C.c_uint32(n), C.c_uint32(S), counts,
                                           plans, C.c_uint64(n_sims), C.c_uint64(sim_offset), C.c_uint64(seed),
                                           _vp(hist), _vp(pos), C.byref(err)), err)
    assert (np.sort(pos, axis=2) == np.arange(n, dtype=np.uint8)).all()            # every row a permutation
    return hist.astype(np.int64), np.argsort(pos, axis=2).astype(np.uint8)


# ---------------------------------------------------------------- the standings kernels (tools/emu/emu_champ.cpp)
CHAMP_HEADERS = ('championship.hip.h', 'champ_pack.h', 'race_common.hip.h')
CHAMP_VARIANTS = {
    None: [],
    # the host's undefined-behaviour sanitizer over the kernels' shifts and indices (reports go to stderr)
    'ubsan': ['-fsanitize=undefined'],
}


def build_champ(variant=None):
    """tools/emu/libmcgp_emu_champ.so: champ_accumulate and champ_rank compiled for the host with blocks of 256 real
    threads (rebuilt when a source it includes is newer)."""
    out = os.path.join(EMU_DIR, 'libmcgp_emu_champ.so' if variant is None else f'libmcgp_emu_champ_{variant}.so')
    srcs = [os.path.join(EMU_DIR, f) for f in ('emu_champ.cpp', 'hip/hip_runtime.h')]
    srcs += [os.path.join(CSRC, f) for f in CHAMP_HEADERS] + [os.path.join(ROOT, 'include', 'mcgp.h')]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(s) for s in srcs):
        tmp = f'{out[:-3]}.tmp{os.getpid()}.so'
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fPIC', '-shared', '-pthread', '-I' + EMU_DIR]
                              + CHAMP_VARIANTS[variant] + ['-o', tmp, os.path.join(EMU_DIR, 'emu_champ.cpp')])
        os.replace(tmp, out)
    return out


def champ_lib(variant=None):
    if ('champ', variant) not in _libs:
        L = C.CDLL(build_champ(variant))
        L.emu_champ_run.restype = C.c_int
        _libs['champ', variant] = L
    return _libs['champ', variant]


def champ_run(orders_list, points_list, countback, team, n_teams, init_points=None, init_counts=None, cap=None,
              gain_in_lds=-1, lds_per_block=160 * 1024, acc_grid=1 << 20, rank_grid=1 << 20, want_keys=False,
              variant=None):
    """champ_accumulate (once per race) and champ_rank on the host over the orders [sims][n] of each race ->
    dict(champ, team, gain: the histograms; info: words, team_cbits, team_words, gain_cols, gain_in_lds, lds_bytes;
    keys: [words][n][cap] u64 of the last chunk when want_keys).  Points tables are padded with zeros to n."""
    R = len(orders_list)
    sims, n = orders_list[0].shape
    orders = np.ascontiguousarray(np.stack([np.asarray(o, np.uint8) for o in orders_list]))
    pts = np.zeros((R, n), np.int32)
    for r, t in enumerate(points_list):
        t = [int(x) for x in t][:n]
        pts[r, :len(t)] = t
    G = int(pts.max(axis=1).sum())
    cb = np.ascontiguousarray(countback, np.uint8)
    tm = np.ascontiguousarray(team, np.int32)
    ip = None if init_points is None else np.ascontiguousarray(init_points, np.int32)
    ic = None if init_counts is None else np.ascontiguousarray(init_counts, np.int32)
    cap = sims if cap is None else int(cap)
    champ, teams = np.zeros((n, n), np.uint64), np.zeros((n_teams, n_teams), np.uint64)
    gain, info, err = np.zeros((n, G + 1), np.uint64), np.zeros(6, np.uint32), C.c_char_p()
    words = (16 + 5 * n + 63) // 64
    keys = np.zeros((words, n, max(min(cap, sims), 1)), np.uint64) if want_keys else None
    rc = champ_lib(variant).emu_champ_run(
        C.c_uint32(R), C.c_uint32(n), C.c_uint64(sims), C.c_uint64(cap), _vp(orders), _vp(pts), _vp(cb), _vp(ip), _vp(ic),
        _vp(tm), C.c_uint32(n_teams), C.c_int32(gain_in_lds), C.c_uint32(lds_per_block), C.c_uint32(acc_grid),
        C.c_uint32(rank_grid), _vp(champ), _vp(teams), _vp(gain), _vp(keys), _vp(info), C.byref(err))
    _ok(rc, err)
    names = ('words', 'team_cbits', 'team_words', 'gain_cols', 'gain_in_lds', 'lds_bytes')
    return dict(champ=champ.astype(np.int64), team=teams.astype(np.int64), gain=gain.astype(np.int64),
                info={k: int(v) for k, v in zip(names, info)}, keys=keys)
