"""Host DEBUGGING build of csrc/champ_rounds.hip.h (tools/emu/emu_champ.cpp: emu_champ_rounds_run): champ_accumulate and
champ_round run on the CPU in blocks of 256 real threads, with the library's own key layout and remaining-points tables
(csrc/champ_pack.h).  Test infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no CPU
path."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

import kernel_host_build as KH

LIB = os.path.join(KH.EMU_DIR, 'libmcgp_emu_champ_rounds.so')
_lib = None


def build():
    """tools/emu/libmcgp_emu_champ_rounds.so (rebuilt when emu_champ.cpp, the stand-in runtime, a header of csrc/ or
    include/mcgp.h is newer)."""
    srcs = [os.path.join(KH.EMU_DIR, f) for f in ('emu_champ.cpp', 'hip/hip_runtime.h')]
    srcs += glob.glob(os.path.join(KH.CSRC, '*.h')) + [os.path.join(KH.ROOT, 'include', 'mcgp.h')]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(s) for s in srcs):
        tmp = f'{LIB[:-3]}.tmp{os.getpid()}.so'               # (renamed into place: a parallel run never maps half a file)
        subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fPIC', '-shared', '-pthread', '-I' + KH.EMU_DIR, '-o', tmp,
                               os.path.join(KH.EMU_DIR, 'emu_champ.cpp')])
        os.replace(tmp, LIB)
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_champ_rounds_run.restype = C.c_int
    return _lib


def rounds_run(orders_list, points_list, countback, team, n_teams, init_points=None, init_counts=None, cap=None, teams=True,
               acc_grid=1 << 20, round_grid=1 << 20, into=None):
    """champ_accumulate and champ_round after every race, on the host, over the orders [sims][n] of each race -> the six
    count arrays of championship_rounds_ref.rounds (the team ones None when teams is False), rem = (M [R], B [R][T]) as
    the library's host side computes them, and info (words, team_cbits, team_words, lds_bytes).  into: an earlier
    result whose uint64 arrays are accumulated into."""
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
    cap = max(sims, 1) if cap is None else int(cap)
    T = n_teams
    raw = into['raw'] if into else dict(
        round_hist=np.zeros((R, n, n), np.uint64), contend=np.zeros((R, n), np.uint64), secure=np.zeros((R, n), np.uint64),
        team_round_hist=np.zeros((R, T, T), np.uint64) if teams else None,
        team_contend=np.zeros((R, T), np.uint64) if teams else None, team_secure=np.zeros((R, T), np.uint64) if teams else None)
    rem, info, err = np.zeros(R + R * T, np.uint32), np.zeros(4, np.uint32), C.c_char_p()
    rc = lib().emu_champ_rounds_run(
        C.c_uint32(R), C.c_uint32(n), C.c_uint64(sims), C.c_uint64(cap), KH._vp(orders), KH._vp(pts), KH._vp(cb), KH._vp(ip),
        KH._vp(ic), KH._vp(tm), C.c_uint32(T), C.c_uint32(1 if teams else 0), C.c_uint32(acc_grid), C.c_uint32(round_grid),
        KH._vp(raw['round_hist']), KH._vp(raw['contend']), KH._vp(raw['secure']), KH._vp(raw['team_round_hist']),
        KH._vp(raw['team_contend']), KH._vp(raw['team_secure']), KH._vp(rem), KH._vp(info), C.byref(err))
    assert rc == 0, (rc, err.value)
    out = {k: (None if v is None else v.astype(np.int64)) for k, v in raw.items()}
    out['raw'] = raw
    out['rem'] = (rem[:R].astype(np.int64), rem[R:].reshape(R, T).astype(np.int64))
    out['info'] = {k: int(v) for k, v in zip(('words', 'team_cbits', 'team_words', 'lds_bytes'), info)}
    return out
