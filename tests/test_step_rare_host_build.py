"""The lap step with its pit writes behind a branch (csrc/race_isa.hip.h step_commit*, stood in for by
tools/emu/race_isa_host.h: the rule word is fetched on a stop only, from the old pk word and the lap's rule row) in the host
build of the register kernel's source, against the CPU oracle's Philox back-ends: finishing orders exactly equal, at both
deviate widths.  Configurations (tests/step_rare_cases.py): the window never opens; a stop on every lap of the window, through
all four regimes of the pit rule; the same with retirements on most laps; S60's parameters as they are; safety cars, VSCs
and red flags in most races.  The CPU twin of tests/test_gpu_step_rare.py."""
import numpy as np
import pytest

import kernel_host_build as K
import oracle_py as O
import step_rare_cases as R


@pytest.mark.parametrize('config', R.CONFIGS)
@pytest.mark.parametrize('n', R.SIZES)
def test_orders_match_the_oracle(n, config):
    case, orders, hist = R.reference(n, config)
    got_hist, got = K.run(case, R.N_SIMS, R.seed_of(n, config))
    bad = np.nonzero((got != orders).any(axis=1))[0]
    assert bad.size == 0, f'n = {n}, {config}: {bad.size} finishing orders differ, first {bad[:5]}'
    assert np.array_equal(got_hist, hist)


@pytest.mark.parametrize('config', R.CONFIGS)
@pytest.mark.parametrize('n', R.SIZES)
def test_orders_match_the_oracle_at_reference_width(n, config):
    case, orders, hist = R.reference(n, config, O.RNG_PHILOX53)
    got_hist, got = K.run(case, R.N_SIMS, R.seed_of(n, config), deviates=53)
    bad = np.nonzero((got != orders).any(axis=1))[0]
    assert bad.size == 0, f'n = {n}, {config}: {bad.size} finishing orders differ, first {bad[:5]}'
    assert np.array_equal(got_hist, hist)


def test_the_sizes_cover_both_forms_and_every_tail():
    """What tests/step_rare_cases.py says about its sizes, read from the kernel source's own lists."""
    import os
    import re
    src = open(os.path.join(K.CSRC, 'race_kernel_reg.hip.h')).read()

    def sizes(fn):
        body = re.search(r'constexpr bool %s\(int n\) \{ return ([^;]*); \}' % fn, src).group(1)
        return {int(x) for x in re.findall(r'n == (\d+)', body)}
    selects, plain = sizes('reg_step_by_selects'), sizes('reg_step_plain')
    assert not (selects & plain)
    branch = [n for n in R.SIZES if n not in selects | plain]
    assert {n % 4 for n in branch} == {0, 1, 2, 3}, branch          # step_commit4 alone, and the tails of 1, 2, 3 slots
    assert any(n in selects for n in R.SIZES) and any(n in plain for n in R.SIZES)
