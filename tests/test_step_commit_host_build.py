"""The lap step's commits (csrc/race_isa.hip.h step_commit*, stood in for by tools/emu/race_isa_host.h) in the host build
of the register kernel's source, against the CPU oracle: fields in which most cars stop several times, several on the
same lap, cars retire in mid-race, and the pit window opens and closes inside the run -- every path asserted from the
oracle's trace before anything is compared.  The CPU twin of tests/test_gpu_step_commit.py."""
import numpy as np
import pytest

import kernel_host_build as K
import oracle_py as O
import step_commit_cases as S


@pytest.mark.parametrize('n', S.SIZES)
def test_lap_step_commits_match_the_oracle(n):
    case, orders, hist = S.reference(n)
    got_hist, got = K.run(case, S.N_SIMS, S.seed_of(n))
    bad = np.nonzero((got != orders).any(axis=1))[0]
    assert bad.size == 0, f'n = {n}: {bad.size} finishing orders differ, first {bad[:5]}'
    assert np.array_equal(got_hist, hist)


@pytest.mark.parametrize('n', [3, 20, 22])
def test_lap_step_commits_at_reference_width(n):
    case, orders, hist = S.reference(n, O.RNG_PHILOX53)
    got_hist, got = K.run(case, S.N_SIMS, S.seed_of(n), deviates=53)
    assert np.array_equal(got, orders) and np.array_equal(got_hist, hist)


def test_a_run_that_ends_inside_a_wave():
    case, orders, hist = S.reference(20, O.RNG_PHILOX, S.TAIL_SIMS)
    got_hist, got = K.run(case, S.TAIL_SIMS, S.seed_of(20))
    assert np.array_equal(got, orders) and np.array_equal(got_hist, hist)
