#!/usr/bin/env python3
"""How often a wave of 64 races has a pit stop or a retirement in some lane, by slot, by batch of four slots and by lap: what
the branch over the lap step's pit region (csrc/race_isa.hip.h step_commit*) is worth.  From the host build of the kernel's
source (tests/kernel_host_build.py) with its per-(simulation, lap, slot) trace (MCGP_TRACE_STEP, tools/emu/emu_kernel.cpp):
64 consecutive simulation ids are one wave, a car's slot is its position at the end of the previous lap, laps 2 .. L.

    python tools/step_rare_stats.py [--sims 768] [--seed 42] [workload ...]        (default: S60 S78 N21)
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

STOP, RETIRE, SLOTS = 1, 2, 32


def trace(case, set_pop, n_sims, seed):
    """[sim][lap][slot] bytes of STOP | RETIRE for laps 2 .. L (rows 0 and 1 stay empty) and the field size."""
    import kernel_host_build as K
    L = int(case['config']['total_laps'])
    buf = np.zeros((n_sims, L + 1, SLOTS), np.uint8)
    lib = K.lib()
    C.c_void_p.in_dll(lib, 'emu_step_buf').value = buf.ctypes.data
    C.c_ulonglong.in_dll(lib, 'emu_step_sims').value = n_sims
    C.c_ulonglong.in_dll(lib, 'emu_step_laps').value = L + 1
    try:
        K.run(case, n_sims, seed, set_pop=set_pop)
    finally:
        C.c_void_p.in_dll(lib, 'emu_step_buf').value = None
    return buf, len(case['grid_probs'])


def shares(buf, n):
    """The shares of wave-slot-laps, wave-batch-laps and wave-laps that have the event in at least one of the 64 lanes."""
    sims, rows, _ = buf.shape
    waves = sims // 64
    w = buf[:waves * 64, 2:, :n].reshape(waves, 64, rows - 2, n)
    any_lane = np.bitwise_or.reduce(w, axis=1)                                   # [wave][lap][slot]
    pad = (-n) % 4
    batches = np.pad(any_lane, ((0, 0), (0, 0), (0, pad))).reshape(waves, rows - 2, -1, 4)
    by_batch = np.bitwise_or.reduce(batches, axis=3)                             # [wave][lap][batch]
    by_lap = np.bitwise_or.reduce(any_lane, axis=2)                              # [wave][lap]
    return {
        'wave-slot-laps with a pit stop': float(((any_lane & STOP) != 0).mean()),
        'wave-batch-laps (4 slots) with a pit stop': float(((by_batch & STOP) != 0).mean()),
        'wave-laps with a pit stop in any slot': float(((by_lap & STOP) != 0).mean()),
        'wave-slot-laps with a retirement on that lap': float(((any_lane & RETIRE) != 0).mean()),
        'wave-batch-laps with a stop or a retirement': float((by_batch != 0).mean()),
        'lane-slot-laps with a pit stop': float(((w & STOP) != 0).mean()),
        'lane-slot-laps with a retirement': float(((w & RETIRE) != 0).mean()),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('workloads', nargs='*', default=['S60', 'S78', 'N21'])
    ap.add_argument('--sims', type=int, default=768, help='simulations per workload (a multiple of 64)')
    ap.add_argument('--seed', type=int, default=42)
    a = ap.parse_args()
    if a.sims % 64:
        ap.error('--sims must be a multiple of 64')
    import bench
    table = {}
    for wl in a.workloads:
        case, set_pop = bench.load_workload(wl)
        buf, n = trace(case, set_pop, a.sims, a.seed)
        table[wl] = shares(buf, n)
    rows = list(next(iter(table.values())))
    print(f'{a.sims} simulations per workload (seed {a.seed}), 64 consecutive ids to a wave, laps 2 .. L')
    print('| share of ... that has the event in at least one of the 64 lanes | ' + ' | '.join(a.workloads) + ' |')
    print('|---|' + '---|' * len(a.workloads))
    for r in rows:
        print(f'| {r} | ' + ' | '.join(f'{table[wl][r]:.3f}' for wl in a.workloads) + ' |')


if __name__ == '__main__':
    main()
