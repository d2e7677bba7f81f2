"""Race movement on the GPU (mcgp_run_moves / RaceSimulator.run_moves): every count equals, cell for cell, what the numpy
restatement (moves_ref) derives from the CPU oracle's per-lap trace (cumulative time, retirement, tyre age, grids,
orders) of the same simulations.  From the grid and from mid-race states; coverage conditions asserted from the
reference before comparing, so that equality is not vacuous; the caps; NULL outputs; accumulation; split, shard and
staging-chunk invariance; the identities at 10^6 simulations with mcgp_run_trace.  All comparisons are integer
equality."""
import ctypes as C
import copy

import numpy as np
import pytest

import moves_ref as MR
import oracle_py as O
import resume_ref as RR
import trace_ref as TR
from helpers import product_run
from monte_carlo_gp_amd import RaceConfig, RaceSimulator, _native as N

pytestmark = pytest.mark.gpu

KEYS = MR.KEYS


def _equal(a, b, what, keys=KEYS):
    for k in keys:
        assert a[k].shape == b[k].shape, (what, k)
        bad = np.argwhere(a[k] != b[k])
        assert bad.size == 0, (what, k, bad[:5].tolist(), a[k][tuple(bad[0])], b[k][tuple(bad[0])])


def _err():
    return N.lib().mcgp_last_error()


def _invariants(got, m, from_grid=True):
    assert np.array_equal(got['grid_fin'].sum(axis=1), got['hist'])
    assert (got['passes'].sum(axis=2) == m).all() and got['race_passes'].sum() == m
    assert not got['lap_passes'][:2].any() and not np.diag(got['pair_passes']).any()
    assert (got['start_gain'].sum(axis=1) == (m if from_grid else 0)).all()
    assert got['pair_passes'].sum() == got['lap_passes'][:, 0].sum()


# ---------------------------------------------------------------- from the grid
@pytest.mark.parametrize('name', ['S60', 'EVT', 'WET', 'N10', 'HET', 'S78', 'DMP'])
def test_golden_cases_equal_the_oracle_trace(require_gpu, name):
    case, m = O.load_case(name), 256
    ref, t = MR.move_counts(case, m, seed=42, with_tallies=True)
    # coverage (conditions, not measurements), from the reference alone
    if name == 'S60':
        assert (int(t['race'].min()), int(t['race'].max())) == (151, 421) and t['kinds'][:, :, 0].max() == 52
        assert t['kinds'][:, :, 2].sum() > 0 and ref['start_gain'][:, -1].sum() > 0   # pit passes, lap-1 retirements
        assert t['kinds'].max() < MR.DRIVER_CAP and t['race'].max() < MR.RACE_CAP
    if name == 'S78':
        assert t['kinds'][:, :, 0].max() == 62
    if name == 'N10':
        assert int((t['race'] == 0).sum()) == 6 and int(t['race'].max()) == 26        # races without a pass
    if name == 'WET':
        assert not t['kinds'][:, :, 2:].any() and t['kinds'][:, :, 0].any()            # no stop on wet tyres
    rc, got = MR.run_c(case, m, seed=42)
    assert rc == 0, _err()
    assert N.lib().mcgp_last_kernel_name(0).decode() == 'mcgp::race_moves_kernel'
    _equal(got, ref, name)
    _invariants(got, m)
    if name == 'WET':
        assert not got['passes'][:, 2:, 1:].any() and not got['lap_passes'][:, 1].any()
    hist, _, _ = product_run(case, m, 42)                                        # the histogram is mcgp_run's
    assert np.array_equal(got['hist'], hist)


def test_the_caps(require_gpu):
    """S78 over 400 laps: a driver's count saturates at 127 and a race's at 1023; the sums do not saturate."""
    case = MR.cap_case()
    ref, t = MR.move_counts(case, 32, seed=42, with_tallies=True)
    made = t['kinds'][:, :, 0]
    assert int((made > 127).sum()) == 16 and int(made.max()) == 214               # checked on the CPU oracle
    assert int((t['race'] > 1023).sum()) == 8 and int(t['race'].max()) == 1725
    assert ref['passes'][:, 0, 127].sum() >= 16 and ref['race_passes'][1023] == 8
    rc, got = MR.run_c(case, 32, seed=42)
    assert rc == 0, _err()
    _equal(got, ref, 'caps')
    _invariants(got, 32)
    assert got['lap_passes'][:, 0].sum() == t['race'].sum()


@pytest.mark.parametrize('n', [1, 2, 32])
def test_synthetic_fields_equal_the_oracle_trace(require_gpu, n):
    case = RR.field_case(n)
    rc, got = MR.run_c(case, 256, seed=3)
    assert rc == 0, _err()
    _equal(got, MR.move_counts(case, 256, seed=3), f'n={n}')
    _invariants(got, 256)


# ---------------------------------------------------------------- from a state
def test_oracle_states_continue_into_the_oracle_trace(require_gpu):
    """Oracle states continued as their own simulation: the counts are the oracle trace's of laps k + 1 .. L against the
    baseline after lap k, the histogram is mcgp_run_from_state's.  From lap L every pass count is 0."""
    total = with_pass = 0
    for name in ('S60', 'EVT', 'N10'):
        case = O.load_case(name)
        L, seed, base = case['config']['total_laps'], 11, 500
        ref = RR.traced_run(case, 4, seed, base)
        prob = RR.problem(case)
        for i in range(4):
            for k in (1, L // 2, L - 1, L):
                st = (RR.state_arrays(ref, i, k), k, RR.drs_disabled_until(case, seed, base + i, k))
                rc, got = MR.run_c(case, 1, seed, sim_offset=base + i, state=st, prob=prob)
                assert rc == 0, _err()
                want = MR.continued_counts(ref, [i], k)
                _equal(got, want, (name, i, k))
                _invariants(got, 1, from_grid=False)
                rc, hist, _ = RR.run_c(prob, [st], 1, [base + i], seed, orders=False)
                assert rc == 0 and np.array_equal(got['hist'], hist[0])
                total += 1
                with_pass += bool(want['pair_passes'].any())
                if k == L:
                    assert not got['lap_passes'].any() and got['race_passes'][0] == 1
    assert total == 48 and with_pass >= 16


def test_one_state_continued_as_many_into_nonzero_buffers(require_gpu):
    case = O.load_case('S60')
    seed, k, m = 13, 31, 256
    ref = RR.traced_run(case, 3, seed)
    st = (RR.state_arrays(ref, 2, k), k, RR.drs_disabled_until(case, seed, 2, k))
    want = MR.restated_counts(case, m, seed, sim_offset=1000, state=st)
    assert not want['lap_passes'][:k + 1].any() and want['lap_passes'][k + 1:, 0].all()  # passes after the state only
    assert (want['grid_fin'].sum(axis=2) > 0).sum() == 20                                # one slot per driver: the state's
    into = {key: np.full_like(v, 5, dtype=np.uint64) for key, v in want.items()}
    rc, got = MR.run_c(case, m, seed, sim_offset=1000, state=st, into=into)
    assert rc == 0, _err()
    assert (got['start_gain'] == 5).all()                                              # NULL with a state: untouched
    got = {key: v - 5 for key, v in got.items()}
    _equal(got, want, 'many from one')
    _invariants(got, m, from_grid=False)
    rc, hist, _ = RR.run_c(RR.problem(case), [st], m, [1000], seed, orders=False)
    assert rc == 0 and np.array_equal(got['hist'], hist[0])


# ---------------------------------------------------------------- NULL outputs, accumulation, splits
def _sum(a, b):
    return {k: a[k] + b[k] for k in KEYS}


def test_null_outputs_accumulation_and_an_odd_split(require_gpu):
    case = O.load_case('EVT')
    N_ = 3001
    rc, whole = MR.run_c(case, N_, seed=9, sim_offset=100)
    assert rc == 0, _err()
    _invariants(whole, N_)
    # every optional output left out: the required ones are unchanged, the others untouched
    rc, part = MR.run_c(case, N_, seed=9, sim_offset=100, skip=MR.OPTIONAL)
    assert rc == 0, _err()
    _equal(part, whole, 'required only', keys=('hist', 'grid_fin'))
    assert not any(part[k].any() for k in MR.OPTIONAL)
    # one left out at a time: the rest is unchanged
    for k in MR.OPTIONAL:
        rc, part = MR.run_c(case, N_, seed=9, sim_offset=100, skip=(k,))
        assert rc == 0, _err()
        assert not part[k].any()
        _equal(part, whole, ('without', k), keys=[x for x in KEYS if x != k])
    # a split at an odd offset, the second call accumulating into the first's buffers
    h = 1237
    into = {k: np.zeros_like(v, dtype=np.uint64) for k, v in whole.items()}
    rc1, _ = MR.run_c(case, h, seed=9, sim_offset=100, into=into)
    rc2, both = MR.run_c(case, N_ - h, seed=9, sim_offset=100 + h, into=into)
    assert rc1 == rc2 == 0
    _equal(both, whole, 'split')
    # two-device-style shards through the simulator surface: device [0, 0] shards by offset
    args = (case['grid_probs'], case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'])
    kw = dict(seed=9, sim_offset=100, track_condition=case['track_condition'])
    one = RaceSimulator(RaceConfig(**case['config']), device=0, set_pop=RR.SET_POP).run_moves(N_, *args, **kw)
    two = RaceSimulator(RaceConfig(**case['config']), device=[0, 0], set_pop=RR.SET_POP).run_moves(N_, *args, **kw)
    for k in KEYS:
        assert np.array_equal(getattr(one, k), getattr(two, k)) and np.array_equal(getattr(one, k), whole[k]), k
    assert one.expected_race_passes() == whole['lap_passes'][:, 0].sum() / N_


def test_a_run_across_a_staging_chunk(require_gpu):
    """32 cars over 1000 laps: the staging budget holds 16 640 simulations, so a call of a few hundred more crosses a
    chunk boundary (the chunk is the budget or, rounded to the device, less); it equals the sum of its halves.  The
    counting kernel's LDS is at its largest here."""
    case = copy.deepcopy(RR.field_case(32))
    case['config']['total_laps'] = 1000
    budget = MR.budget_sims(32, 1000)
    assert budget == (512 << 20) // (1002 * 32) // 256 * 256 == 16640
    N_ = budget + 777
    rc, whole = MR.run_c(case, N_, seed=9, sim_offset=100)
    assert rc == 0, _err()
    assert MR.chunk_sims(32, 1000, TR.device_round()) <= budget < N_
    h = N_ // 2 + 1
    rc1, a = MR.run_c(case, h, seed=9, sim_offset=100)
    rc2, b = MR.run_c(case, N_ - h, seed=9, sim_offset=100 + h)
    assert rc1 == rc2 == 0
    _equal(whole, _sum(a, b), 'across a chunk')
    _invariants(whole, N_)
    assert whole['lap_passes'][2:12, 0].all() and whole['lap_passes'][:, 1].any()   # on track and through the pits
    # the first 64 simulations against the oracle
    rc, got = MR.run_c(case, 64, seed=9, sim_offset=100)
    assert rc == 0, _err()
    _equal(got, MR.move_counts(case, 64, seed=9, sim_offset=100), 'first 64')


# ---------------------------------------------------------------- the identities at a million
def test_identities_at_a_million(require_gpu):
    case = O.load_case('S60')
    N_, n = 10 ** 6, 20
    rc, s = MR.run_c(case, N_, seed=21)
    assert rc == 0, _err()
    f = C.c_float()
    assert N.lib().mcgp_last_kernel_ms(0, C.byref(f)) == 0 and f.value > 0
    rc, t = TR.run_c(case, N_, seed=21)
    assert rc == 0, _err()
    assert np.array_equal(s['hist'], t['hist'])
    assert np.array_equal(s['grid_fin'].sum(axis=1), s['hist'])
    assert np.array_equal(s['start_gain'][:, 2 * n - 1], t['lap_pos'][0, :, n])
    counts = np.arange(128)
    assert not s['passes'][:, :, 127].any() and not s['race_passes'][1023]        # no cap is reached on S60
    by_kind = (s['passes'] * counts[None, None, :]).sum(axis=(0, 2))
    track = int(s['lap_passes'][:, 0].sum())
    assert by_kind[0] == by_kind[1] == s['pair_passes'].sum() == track == (s['race_passes'] * np.arange(1024)).sum()
    assert by_kind[2] == by_kind[3] == s['lap_passes'][:, 1].sum() > 0
    _invariants(s, N_)
