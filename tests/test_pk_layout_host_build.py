"""The pk word and the block-shared LDS map of the register kernel (csrc/race_kernel_reg.hip.h: RegTables, reg_tables, RegGeo)
on the CPU: the kernel's source compiled for the host (tests/kernel_host_build.py) against the oracle on fields in which every
table row decides something, and the map's own arithmetic checked at compile time.

Field sizes: 4, 19, 20, 22, 26 and 30 run the re-laid map with the {delta, DRS gain} rows inside the per-(compound, driver)
table (30 is the largest size with room for them); 31 and 32 the re-laid map with the separate delta table; 2 and 3 (nothing
packs), 9 and 21 (reg_pk_earlier_layout) the earlier map.  Both deviate widths; finishing orders equal the oracle's, race by
race."""
import os
import subprocess

import numpy as np
import pytest

import kernel_host_build as K
import pk_layout_cases as P

N_SIMS = 300


@pytest.mark.parametrize('deviates', [32, 53])
@pytest.mark.parametrize('n', P.SIZES)
def test_finishing_orders_equal_the_oracle(n, deviates):
    shown = set()
    for track in P.TRACKS:
        case = P.field(n, track)
        ref = P.reference(n, track, N_SIMS, deviates, 0, N_SIMS)
        # from the oracle's output alone: the run reaches every row of the tables the layout moves
        s = P.what_the_run_shows(case, ref['trace'])
        assert s['regimes'] == {0, 1, 2, 3}, (track, s['regimes'])
        missing = [k for k, v in s.items() if v is False]
        assert not missing, (track, missing)
        shown |= s['compounds']
        hist, orders = K.run(case, N_SIMS, P.seed_of(n, track), deviates=deviates)
        bad = np.nonzero((orders != ref['orders']).any(axis=1))[0]
        assert bad.size == 0, f'{n} cars, {track}: {bad.size} finishing orders differ, first {bad[:5]}'
        assert np.array_equal(hist, ref['hist'])
    assert shown == {0, 1, 2, 3, 4}, shown


# the launch's LDS bytes at the sizes tests/test_gpu_parity.py pins (default block shapes: 12, 11 and 16 waves)
PINNED_LAUNCH_BYTES = {20: 15808 + 768 * 192, 21: 157168, 10: 69072}

_CHECKS = r'''
#include <cstdint>
#define MCGP_COOPERATIVE_EVENTS 0
#include "race_isa_host.h"
#include "race_kernel_reg.hip.h"
using namespace mcgp;
// the bytes of the block-shared tables before the re-laid map: what the launch has always reserved for them
constexpr uint32_t earlier_bytes(int n, bool wide)
{
    return (uint32_t)((wide ? 0 : kNormalRows * 16) + n * 16 + (kMaxCars + n) * 16 + ((kNumCompounds - 1) * kMaxCars + n) * 16 +
                      kCompStride * 16 + 64 + 128 + (n * n * 4 + 15) / 16 * 16 + (n * n * 8 + 15) / 16 * 16);
}
template <class G, int N, bool WIDE>
constexpr bool geometry_ok()
{
    // the map ends within the earlier byte count and the per-lane planes start exactly there
    static_assert(G::T.end <= earlier_bytes(N, WIDE) && G::oW == earlier_bytes(N, WIDE), "shared bytes");
    static_assert(WIDE || (G::oW == shared_lds_bytes_reg(N) && G::kBytes == shared_lds_bytes_reg(N) + (uint32_t)G::B * per_thread_lds_bytes_reg(N)), "launch bytes");
    // the NaN copy of the overtake pace sits at the geometry's distance: the dnf bit of pk IS that byte offset
    static_assert(G::kSlotMask == (k3IdMask | G::kDnf), "slot mask");
    static_assert(G::kRelaid ? (G::kDnf == 4096u || G::kDnf == 8192u) && G::kDirty == (G::kDnf ^ 0x3000u) && G::kCompMask == 0xE00u
                             : G::kDnf == 512u && G::kDirty == 8192u && G::kCompMask == 0x1C00u, "pk word");
    // ... and nothing else lies in [copy, copy + 16 N), nor between the live table and the copy's tables
    constexpr uint32_t live = G::oDrvB, copy = G::oDrvB + G::kDnf;
    constexpr uint32_t starts[] = {G::oDrvA, G::oIc, G::oDrs, G::oLut, G::oHist, G::oGrid, WIDE ? G::oHist : G::oNorm, G::kPair ? G::oIc : G::oComp};
    constexpr uint32_t sizes[] = {N * 16, (uint32_t)((kNumCompounds - 1) * kMaxCars + N) * 16 + (G::kPair ? 32u : 0u), 64, 128,
                                  (uint32_t)(N * N * 4 + 15) / 16 * 16, (uint32_t)(N * N * 8 + 15) / 16 * 16,
                                  WIDE ? 0u : (uint32_t)kNormalRows * 16, G::kPair ? 0u : (uint32_t)kCompStride * 16};
    for (int i = 0; i < 8; ++i) {
        if (sizes[i] == 0) continue;
        if (starts[i] + sizes[i] > G::T.end) return false;
        if (starts[i] < live + N * 16 && live < starts[i] + sizes[i]) return false;        // overlaps the live table
        if (starts[i] < copy + N * 16 && copy < starts[i] + sizes[i]) return false;        // overlaps the NaN copy
        for (int j = 0; j < i; ++j)
            if (sizes[j] != 0 && starts[i] < starts[j] + sizes[j] && starts[j] < starts[i] + sizes[i]) return false;
    }
    if (copy + N * 16 > G::T.end) return false;
    // the pair rows lie in the padding of the per-(compound, driver) table, and their base fits the read2 offsets
    if (G::kPair && !(N <= 30 && G::oPair == G::oIc + N * 16 && G::oPair % 8 == 0 && G::oPair / 8 + 2 <= 255 && G::kPairMask == 0xE08u)) return false;
    if (G::kRelaid && G::kIcMask != 0xFF0u) return false;
    return true;
}
#define CHECK_SIZE(N) \
    static_assert(geometry_ok<RegGeo<N>, N, false>(), "default width, " #N " cars"); \
    static_assert(geometry_ok<RegGeo<N, 4>, N, false>(), "4-wave blocks, " #N " cars"); \
    static_assert(geometry_ok<BatchGeo<N>, N, false>(), "batch, " #N " cars"); \
    static_assert(geometry_ok<WideGeo<N>, N, true>(), "reference width, " #N " cars");
SIZES
// which sizes run which map (RegTables; reg_pk_earlier_layout)
static_assert(RegGeo<20>::kRelaid && RegGeo<20>::kPair && RegGeo<30>::kPair && RegGeo<4>::kPair, "re-laid, pair rows");
static_assert(RegGeo<31>::kRelaid && !RegGeo<31>::kPair && RegGeo<32>::kRelaid && !RegGeo<32>::kPair, "re-laid, separate delta table");
static_assert(!RegGeo<2>::kRelaid && !RegGeo<3>::kRelaid && !RegGeo<9>::kRelaid && !RegGeo<21>::kRelaid, "earlier map");
static_assert(!BatchGeo<20>::kRelaid && BatchGeo<19>::kRelaid && WideGeo<20>::kRelaid && !WideGeo<10>::kRelaid, "per kernel");
PINNED
'''


def test_the_map_keeps_every_launch_size_and_its_own_promises(tmp_path):
    """One compile-time check per field size, in all four instantiations: the map ends within the bytes the launch had before
    (the per-lane planes start where they did), no two tables overlap, the NaN copy of the overtake pace sits exactly at the
    distance the dnf bit gives, the pair rows' base fits the 8-bit offsets of ds_read2_b64 -- and the launch sizes
    tests/test_gpu_parity.py pins are what RegGeo computes."""
    sizes = sorted(set(P.SIZES) | set(PINNED_LAUNCH_BYTES))
    src = _CHECKS.replace('SIZES', '\n'.join(f'CHECK_SIZE({n})' for n in sizes))
    src = src.replace('PINNED', '\n'.join(f'static_assert(RegGeo<{n}>::kBytes == {b}u, "launch bytes of {n} cars");'
                                          for n, b in PINNED_LAUNCH_BYTES.items()))
    path = tmp_path / 'pk_layout_checks.cpp'
    path.write_text(src)
    r = subprocess.run(['g++', '-std=c++17', '-fsyntax-only', '-I' + K.EMU_DIR, '-I' + K.CSRC, str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
