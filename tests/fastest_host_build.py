"""Host DEBUGGING builds of the fastest-lap bonus kernels: race_fastest_kernel (csrc/fastest.hip.h) through
tools/emu/emu_generic.cpp (emu_fastest_run: one simulation after another) and champ_bonus (csrc/champ_bonus.hip.h) behind
champ_accumulate through tools/emu/emu_champ.cpp (emu_champ_bonus_run: blocks of 256 real threads, the library's own key
layout from csrc/champ_pack.h).  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and
has no CPU path."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

import kernel_host_build as KH

BONUS_LIB = os.path.join(KH.EMU_DIR, 'libmcgp_emu_champ_bonus.so')
_lib = None


def fastest_run(case, n_sims, seed, sim_offset=0, prob=None):
    """race_fastest_kernel on the host -> (hist [n][n], orders [n_sims][n] u8, fl_driver [n_sims] u8, fl_pos [n_sims]
    u8), after checking that nothing was written past the chunk."""
    p, g = prob or KH.generic_problem(case)
    n, pad = p.n, 64
    hist, err = np.zeros((n, n), np.uint64), C.c_char_p()
    orders = np.full((n_sims + pad, n), 0x7E, np.uint8)
    fl_driver, fl_pos = np.full(n_sims + pad, 0x7E, np.uint8), np.full(n_sims + pad, 0x7E, np.uint8)
    L = KH.generic_lib()
    L.emu_fastest_run.restype = C.c_int
    KH._ok(L.emu_fastest_run(C.byref(p.cfg), C.byref(p.drv), KH._vp(g), C.c_uint32(n), C.c_uint64(n_sims),
                             C.c_uint64(sim_offset), C.c_uint64(seed), KH._vp(hist), KH._vp(orders), KH._vp(fl_driver),
                             KH._vp(fl_pos), C.byref(err)), err)
    assert (orders[n_sims:] == 0x7E).all() and (fl_driver[n_sims:] == 0x7E).all() and (fl_pos[n_sims:] == 0x7E).all()
    return hist.astype(np.int64), orders[:n_sims], fl_driver[:n_sims], fl_pos[:n_sims]


def build_bonus():
    """tools/emu/libmcgp_emu_champ_bonus.so (rebuilt when emu_champ.cpp, the stand-in runtime, a header of csrc/ or
    include/mcgp.h is newer)."""
    srcs = [os.path.join(KH.EMU_DIR, f) for f in ('emu_champ.cpp', 'hip/hip_runtime.h')]
    srcs += glob.glob(os.path.join(KH.CSRC, '*.h')) + [os.path.join(KH.ROOT, 'include', 'mcgp.h')]
    if not os.path.exists(BONUS_LIB) or os.path.getmtime(BONUS_LIB) < max(os.path.getmtime(s) for s in srcs):
        tmp = f'{BONUS_LIB[:-3]}.tmp{os.getpid()}.so'         # (renamed into place: a parallel run never maps half a file)
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fPIC', '-shared', '-pthread', '-I' + KH.EMU_DIR, '-o', tmp,
                               os.path.join(KH.EMU_DIR, 'emu_champ.cpp')])
        os.replace(tmp, BONUS_LIB)
    return BONUS_LIB


def bonus_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build_bonus())
        _lib.emu_champ_bonus_run.restype = C.c_int
    return _lib


def bytes_of(races):
    """(fl_driver, fl_pos) [R][m] u8 as race_fastest_kernel writes them, from championship_bonus_ref race dicts."""
    to_byte = lambda a: np.where(a < 0, 0xFF, a).astype(np.uint8)
    return (np.ascontiguousarray([to_byte(r['fl_driver']) for r in races]),
            np.ascontiguousarray([to_byte(r['fl_pos']) for r in races]))


def bonus_run(orders_list, points_list, countback, team, n_teams, bonus_points, bonus_within, fl_driver, fl_pos,
              init_points=None, init_counts=None, cap=None, acc_grid=1 << 20, into=None, expect_rc=0):
    """champ_accumulate and, for the races with a bonus, champ_bonus on the host -> dict(keys [words][n][cap] u64 of the
    last chunk, bonus_hist and fastest_hist [R][n], info: words, team_cbits, team_words, gain_cols), or (rc, message)
    when expect_rc is not 0.  into: an earlier result whose uint64 arrays are accumulated into."""
    R = len(orders_list)
    sims, n = orders_list[0].shape
    orders = np.ascontiguousarray(np.stack([np.asarray(o, np.uint8) for o in orders_list]))
    pts = np.zeros((R, n), np.int32)
    for r, t in enumerate(points_list):
        t = [int(x) for x in t][:n]
        pts[r, :len(t)] = t
    cb = np.ascontiguousarray(countback, np.uint8)
    tm = np.ascontiguousarray(team, np.int32)
    ip = None if init_points is None else np.ascontiguousarray(init_points, np.int32)
    ic = None if init_counts is None else np.ascontiguousarray(init_counts, np.int32)
    bp, bw = np.ascontiguousarray(bonus_points, np.int32), np.ascontiguousarray(bonus_within, np.int32)
    fd, fp = np.ascontiguousarray(fl_driver, np.uint8), np.ascontiguousarray(fl_pos, np.uint8)
    assert fd.shape == (R, sims) == fp.shape
    cap = max(sims, 1) if cap is None else int(cap)
    words = (16 + 5 * n + 63) // 64
    keys = np.zeros((words, n, max(min(cap, sims), 1)), np.uint64)
    raw = into['raw'] if into else dict(bonus_hist=np.zeros((R, n), np.uint64), fastest_hist=np.zeros((R, n), np.uint64))
    info, err = np.zeros(4, np.uint32), C.c_char_p()
    rc = bonus_lib().emu_champ_bonus_run(
        C.c_uint32(R), C.c_uint32(n), C.c_uint64(sims), C.c_uint64(cap), KH._vp(orders), KH._vp(pts), KH._vp(cb), KH._vp(ip),
        KH._vp(ic), KH._vp(tm), C.c_uint32(n_teams), KH._vp(bp), KH._vp(bw), KH._vp(fd), KH._vp(fp), C.c_uint32(acc_grid),
        KH._vp(keys), KH._vp(raw['bonus_hist']), KH._vp(raw['fastest_hist']), KH._vp(info), C.byref(err))
    if expect_rc:
        assert rc == expect_rc, (rc, err.value)
        return rc, err.value.decode()
    assert rc == 0, (rc, err.value)
    return dict(keys=keys, bonus_hist=raw['bonus_hist'].astype(np.int64), fastest_hist=raw['fastest_hist'].astype(np.int64),
                raw=raw, info={k: int(v) for k, v in zip(('words', 'team_cbits', 'team_words', 'gain_cols'), info)})


def decode_keys(keys, n):
    """(points [sims][n], counts [sims][n][n]) of a key buffer [words][n][sims], every field with Python integers: key =
    sum of word w << 64 w; points above bit 5 n, the count of position p + 1 at bit 5 (n - 1 - p), 5 bits."""
    words, n_, sims = keys.shape
    assert n_ == n
    pts, cnt = np.zeros((sims, n), np.int64), np.zeros((sims, n, n), np.int64)
    for s in range(sims):
        for d in range(n):
            key = sum(int(keys[w, d, s]) << (64 * w) for w in range(words))
            pts[s, d] = key >> (5 * n)
            assert pts[s, d] < 1 << 16                              # nothing above the points field
            for p in range(n):
                cnt[s, d, p] = (key >> (5 * (n - 1 - p))) & 31
    return pts, cnt
