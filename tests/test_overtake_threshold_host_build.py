"""The threshold stage of an overtake pass (csrc/race_isa.hip.h ovt_threshold_x and, at the field sizes of
reg_threshold_by_selects, ovt_threshold; both stood in for by tools/emu/race_isa_host.h) in the host build of the register
kernel's source, against the CPU oracle at both deviate widths.  The CPU twin of tests/test_gpu_overtake_threshold.py."""
import numpy as np
import pytest

import kernel_host_build as K
import oracle_py as O
import overtake_threshold_cases as T

N_SIMS = 400


def test_the_select_form_list_is_read():
    sizes = T.select_form_sizes()
    assert sizes and 5 not in sizes and 20 not in sizes       # (the sizes below run the EXEC form's stand-in)


# 5 and 20 run ovt_threshold_x, the first size of the list the kept ovt_threshold
@pytest.mark.parametrize('n', [5, 20, T.select_form_sizes()[0]])
@pytest.mark.parametrize('deviates,rng', T.WIDTHS)
def test_threshold_stage_matches_the_oracle(n, deviates, rng):
    case = T.field(n)
    seed = 11 + n
    ref = O.Problem(case).run(N_SIMS, rng=rng, seed=seed, sim_offset=3, want_orders=True)
    hist, orders = K.run(case, N_SIMS, seed, sim_offset=3, deviates=deviates)
    bad = np.nonzero((orders != ref['orders']).any(axis=1))[0]
    assert bad.size == 0, f'n = {n}, deviates {deviates}: {bad.size} finishing orders differ, first {bad[:5]}'
    assert np.array_equal(hist, ref['hist'])
    if deviates == 32:
        assert T.overtakes_change(case, N_SIMS, seed, sim_offset=3) >= 0.1
