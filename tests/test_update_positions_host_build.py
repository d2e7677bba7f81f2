"""The position update (csrc/race_isa.hip.h upd_commit*, stood in for by tools/emu/race_isa_host.h; the select form of
csrc/race_kernel_reg.hip.h where two times are equal) in the host build of the register kernel's source, against the CPU
oracle: a close field and a spread one per size -- retired cars in front of the first running car and between two
running ones, DRS on and off, gaps on both sides of the dirty-air bound, equal times -- every path asserted from the
oracle's trace before anything is compared.  The CPU twin of tests/test_gpu_update_positions.py."""
import numpy as np
import pytest

import kernel_host_build as K
import oracle_py as O
import update_positions_cases as U


@pytest.mark.parametrize('kind', U.KINDS)
@pytest.mark.parametrize('n', U.SIZES)
def test_position_update_matches_the_oracle(n, kind):
    case, orders, hist = U.reference(n, kind)
    got_hist, got = K.run(case, U.N_SIMS, U.seed_of(n))
    bad = np.nonzero((got != orders).any(axis=1))[0]
    assert bad.size == 0, f'n = {n}, {kind}: {bad.size} finishing orders differ, first {bad[:5]}'
    assert np.array_equal(got_hist, hist)


@pytest.mark.parametrize('kind', U.KINDS)
@pytest.mark.parametrize('n', [3, 20, 22])
def test_position_update_at_reference_width(n, kind):
    case, orders, hist = U.reference(n, kind, O.RNG_PHILOX53)
    got_hist, got = K.run(case, U.N_SIMS, U.seed_of(n), deviates=53)
    assert np.array_equal(got, orders) and np.array_equal(got_hist, hist)


def test_a_run_that_ends_inside_a_wave():
    case, orders, hist = U.reference(20, 'spread', O.RNG_PHILOX, U.TAIL_SIMS)
    got_hist, got = K.run(case, U.TAIL_SIMS, U.seed_of(20))
    assert np.array_equal(got, orders) and np.array_equal(got_hist, hist)
