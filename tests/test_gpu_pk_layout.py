"""The pk word and the block-shared LDS map of the register kernel (csrc/race_kernel_reg.hip.h: RegTables, RegGeo) on the
device: race_kernel_reg<N>, race_kernel_reg_wide<N> and race_kernel_reg_batch<N> against the CPU oracle, finishing order by
finishing order, on the fields of tests/pk_layout_cases.py -- cars on every compound, stops in every regime of the pit rule,
retirements on lap 1 and later, DRS on and off, dirty air, event laps (proved from the oracle's trace by
tests/test_pk_layout_host_build.py on the same fields and seeds).

Field sizes: the re-laid map with pair rows (4, 19, 20, 22, 26, 30), the re-laid map with the separate delta table (31, 32),
and the earlier map: 2 and 3 (nothing packs), 9 and 21 (on reg_pk_earlier_layout's list at both widths); the batch kernel's
own list is met by a batch of 19-car (re-laid) and 20-car (earlier map) problems in one call."""
import numpy as np
import pytest

import pk_layout_cases as P
from batch_cases import last_launch, run_batch
from helpers import product_run

pytestmark = pytest.mark.gpu

N_SIMS = 24 * 64 + 37           # 24 full wave-chunks and a ragged one


@pytest.mark.parametrize('deviates', [32, 53])
@pytest.mark.parametrize('n', P.SIZES)
def test_finishing_orders_equal_the_oracle(require_gpu, n, deviates):
    offset = 1000003 + 64 * n           # no multiple of the chunk size
    for track in P.TRACKS:
        ref = P.reference(n, track, N_SIMS, deviates, offset)
        hist, _, orders = product_run(P.field(n, track), N_SIMS, P.seed_of(n, track), sim_offset=offset, orders=True,
                                      deviates=deviates)
        name = last_launch()[0]
        # (the register kernel itself, not the generic one: 'mcgp::race_kernel_reg<20>', '..<20, 4>' for the small block)
        assert name.startswith((f'mcgp::race_kernel_reg_wide<{n}>',) if deviates == 53
                               else (f'mcgp::race_kernel_reg<{n}>', f'mcgp::race_kernel_reg<{n},')), name
        bad = np.nonzero((orders != ref['orders']).any(axis=1))[0]
        assert bad.size == 0, f'{n} cars, {track}: {bad.size} finishing orders differ, first {bad[:5]}'
        assert np.array_equal(hist, ref['hist'])


def test_a_batch_of_both_layouts(require_gpu):
    """mcgp_run_batch with 19-car problems (the batch kernel's re-laid map) and 20-car problems (its earlier map) interleaved,
    on all three tracks."""
    specs = []
    for i, track in enumerate(P.TRACKS):
        for n in (19, 20):
            specs.append((P.field(n, track), P.seed_of(n, track), 64 * i + 5, 32))
    hists = run_batch(specs, N_SIMS)
    assert last_launch()[0].startswith('mcgp::race_kernel_reg_batch<'), last_launch()
    for (case, seed, off, dev), h in zip(specs, hists):
        n = len(case['grid_probs'])
        ref = P.reference(n, case['track_condition'], N_SIMS, dev, off)
        assert np.array_equal(h, ref['hist']), (n, case['track_condition'])
