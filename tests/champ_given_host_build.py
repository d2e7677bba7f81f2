"""Host DEBUGGING build of csrc/champ_given.hip.h (tools/emu/emu_champ.cpp: emu_champ_given_run): champ_accumulate and
champ_given run on the CPU in blocks of 256 real threads, with the library's own key layout (csrc/champ_pack.h).  Test
infrastructure only -- the product (monte_carlo_gp_amd/) never imports this and has no CPU path."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

import kernel_host_build as KH

LIB = os.path.join(KH.EMU_DIR, 'libmcgp_emu_champ_given.so')
_lib = None


def build():
    """tools/emu/libmcgp_emu_champ_given.so (rebuilt when emu_champ.cpp, the stand-in runtime, a header of csrc/ or
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
        _lib.emu_champ_given_run.restype = C.c_int
    return _lib


def given_run(orders_list, points_list, countback, given_race, init_points=None, init_counts=None, cap=None, in_lds=True,
              acc_grid=1 << 20, given_grid=1 << 20, into=None):
    """champ_accumulate after every race and champ_given behind the last, on the host, over the orders [sims][n] of each
    race -> (given [n][n][n] int64, info {words, lds_bytes}).  in_lds: the kernel's LDS table, or global atomics.  into:
    a uint64 table that is accumulated into (and returned as int64)."""
    R = len(orders_list)
    sims, n = orders_list[0].shape
    orders = np.ascontiguousarray(np.stack([np.asarray(o, np.uint8) for o in orders_list]))
    pts = np.zeros((R, n), np.int32)
    for r, t in enumerate(points_list):
        t = [int(x) for x in t][:n]
        pts[r, :len(t)] = t
    cb = np.ascontiguousarray(countback, np.uint8)
    tm = np.zeros(n, np.int32)
    ip = None if init_points is None else np.ascontiguousarray(init_points, np.int32)
    ic = None if init_counts is None else np.ascontiguousarray(init_counts, np.int32)
    cap = max(sims, 1) if cap is None else int(cap)
    raw = into if into is not None else np.zeros((n, n, n), np.uint64)
    info, err = np.zeros(2, np.uint32), C.c_char_p()
    rc = lib().emu_champ_given_run(
        C.c_uint32(R), C.c_uint32(n), C.c_uint64(sims), C.c_uint64(cap), KH._vp(orders), KH._vp(pts), KH._vp(cb), KH._vp(ip),
        KH._vp(ic), KH._vp(tm), C.c_uint32(1), C.c_uint32(given_race), C.c_uint32(1 if in_lds else 0), C.c_uint32(acc_grid),
        C.c_uint32(given_grid), KH._vp(raw), KH._vp(info), C.byref(err))
    assert rc == 0, (rc, err.value)
    return raw.astype(np.int64), {'words': int(info[0]), 'lds_bytes': int(info[1])}
