"""mcgp_run_batch on the device -- race_kernel_reg_batch<N> and the host code around it -- against the CPU oracle: whole
integer histograms, cell for cell, no tolerance anywhere.

The batch instantiation of a field size is compiled by itself (its own register allocation and spills) and has a block
driver the single-problem kernel has not: the 64-at-a-time scan of the problems' ticket counters, table reloads between
problems, the LDS word behind RegGeo<N>::kBytes, a flush per problem.  So: every field size 1..32 (blocks of every shape
reg_block_waves gives), seeds and simulation offsets whose high words matter, the scan at problem counts around multiples of
64 and at the ABI's 4096, launches with fewer chunks than a block has waves and with more blocks than problems, parameter
blocks whose stride follows the longest race, shared and solo problems in one call, the workspace re-used by calls of other
sizes, sim_offsets = NULL, and a device that offers less LDS than the batch kernel's block needs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
from batch_cases import RawBatch, field, last_launch, problems_and_references, reference, run_batch
from helpers import product_run

pytestmark = pytest.mark.gpu

HI = 1 << 32


def _check(specs, n_sims, hists, refs=None):
    refs = refs if refs is not None else [reference(s[0], n_sims, *s[1:]) for s in specs]
    assert len(hists) == len(specs) == len(refs)
    bad = [i for i, (h, r) in enumerate(zip(hists, refs)) if not np.array_equal(h, r)]
    assert not bad, f'{len(bad)} of {len(specs)} histograms differ from the oracle, first problems {bad[:8]}'


# ---- 1. every field size

N_SIMS_1 = 3 * 64 + 37          # three full wave-chunks and a ragged one


def _six_problems(n):
    """Six problems of one batch.  2 and 5 differ in the seed's high word only; 3's seed has bit 63 set; 4 starts at
    simulation 3 + 2^32."""
    seed = 1000 + 7 * n
    return [(field(n, 1, shift=0, track_condition='damp'), seed, 11, 32),
            (field(n, 2, shift=1, pace=0.07, track_condition='wet'), seed + 1, 64, 32),
            (field(n, 7, shift=2, pace=0.11), seed + 2, 5, 32),
            (field(n, 60, shift=3, pace=0.03), (1 << 63) | (seed + 3), 1000003, 32),
            (field(n, 70, shift=4, pace=0.13, **({'overtake_delta': 0.0} if n >= 10 else {})), seed + 4, 3 + HI, 32),
            (field(n, 7, shift=2, pace=0.11), seed + 2 + HI, 5, 32)]


@pytest.mark.parametrize('n', range(1, 33))
def test_every_field_size(require_gpu, n):
    """24 wave-chunks over 6 problems: more than one block's waves at every size, so at least two blocks run and each walks
    several problems, reloading its tables."""
    specs = _six_problems(n)
    problems, refs = problems_and_references(specs, N_SIMS_1)
    if n > 1:
        # from the reference alone: the high words of the seed and of the offset matter (at n = 1 nothing can differ)
        assert not np.array_equal(refs[2], refs[5]), 'the seed pair is vacuous'
        case, seed, off, dev = specs[4]
        assert not np.array_equal(refs[4], reference(case, N_SIMS_1, seed, off - HI, dev)), 'the offset pair is vacuous'
    hists = run_batch(specs, N_SIMS_1)
    name, grid, block, lds = last_launch()
    assert name == f'mcgp::race_kernel_reg_batch<{n}>'
    assert grid >= 2 and 24 > block // 64
    _check(specs, N_SIMS_1, hists, refs)
    for h in hists:
        assert (h.sum(axis=0) == N_SIMS_1).all() and (h.sum(axis=1) == N_SIMS_1).all()
    case, seed, off, dev = specs[3]
    assert np.array_equal(hists[3], product_run(case, N_SIMS_1, seed, sim_offset=off)[0])


# ---- 2. the scan's boundaries

N_SIMS_2 = 65                   # one full chunk and one of a single simulation


def _many(n, k, laps=6, seed0=0):
    return [(field(n, laps, shift=i % 6, pace=0.01 * (i % 17)), seed0 + 31 * i + 1, 64 * (i % 5), 32) for i in range(k)]


@functools.lru_cache(maxsize=None)
def _many_references(n, k, n_sims, laps=6, seed0=0):
    return tuple(reference(s[0], n_sims, *s[1:]) for s in _many(n, k, laps, seed0))


@pytest.mark.parametrize('k', [1, 2, 63, 64, 65, 127, 128, 129])
@pytest.mark.parametrize('n', [3, 23])
def test_problem_counts_around_the_scan_step(require_gpu, n, k):
    specs = _many(n, k)
    hists = run_batch(specs, N_SIMS_2)
    name, grid, block, lds = last_launch()
    assert name == f'mcgp::race_kernel_reg_batch<{n}>'
    if k == 129:
        assert grid < k, (grid, block)          # blocks walk several problems: the scan goes past its first 64 counters
    _check(specs, N_SIMS_2, hists, _many_references(n, 129, N_SIMS_2)[:k])


@pytest.mark.parametrize('n', [3, 23])
def test_one_chunk_and_more_blocks_than_problems(require_gpu, n):
    one = _many(n, 1, seed0=500)
    for n_sims in (1, 64):      # one wave-chunk: one block, all its waves but one idle
        hists = run_batch(one, n_sims)
        name, grid, block, lds = last_launch()
        assert name == f'mcgp::race_kernel_reg_batch<{n}>' and grid == 1, (name, grid)
        _check(one, n_sims, hists)
        assert hists[0].sum() == n * n_sims
    two = _many(n, 2, seed0=900)
    n_sims = 64 * 300 + 1
    hists = run_batch(two, n_sims)
    name, grid, block, lds = last_launch()
    assert name == f'mcgp::race_kernel_reg_batch<{n}>'
    assert grid > 2, grid        # several blocks flush into one histogram
    _check(two, n_sims, hists)


# ---- 3. the ABI limit

def test_4096_problems(require_gpu):
    n, n_sims = 2, 70
    cases = [field(n, 3, shift=s, pace=0.05 * q) for s in range(6) for q in range(4)]
    specs = [(cases[i % 24], i, 64 * i + 5, 32) for i in range(4096)]
    hists = run_batch(specs, n_sims)
    assert last_launch()[0] == 'mcgp::race_kernel_reg_batch<2>'
    problems = [O.Problem(c) for c in cases]
    refs = [problems[i % 24].run(n_sims, rng=O.RNG_PHILOX, seed=i, sim_offset=64 * i + 5)['hist'] for i in range(4096)]
    # (2 x 2 histograms take few values, but a problem given its neighbour's histogram, or that of the problem 32 or 64
    # places on, would show: from the reference alone, most such pairs differ)
    for step in (1, 32, 64):
        assert sum(not np.array_equal(refs[i], refs[i + step]) for i in range(4096 - step)) > 3000, step
    _check(specs, n_sims, hists, refs)


# ---- 4. the parameter blocks' stride

@pytest.mark.parametrize('n', [20, 5])
def test_parameter_stride_follows_the_longest_race(require_gpu, n):
    specs = [(field(n, 1, shift=1), 41, 3, 32), (field(n, 130, shift=2, pace=0.05), 42, 70, 32), (field(n, 5, shift=3), 43, 9, 32)]
    refs = [reference(s[0], N_SIMS_1, *s[1:]) for s in specs]
    for order in ([1, 0, 2], [0, 2, 1]):            # the longest first, the longest last
        hists = run_batch([specs[i] for i in order], N_SIMS_1)
        assert last_launch()[0] == f'mcgp::race_kernel_reg_batch<{n}>'
        _check([specs[i] for i in order], N_SIMS_1, hists, [refs[i] for i in order])


# ---- 5. shared and solo problems

def test_shared_and_solo_problems_of_eight_cars(require_gpu):
    n_sims = N_SIMS_1
    specs = _many(8, 7, laps=9, seed0=70)
    specs[0] = (field(8, 9, overtake_delta=-50.0), 71, 2, 32)           # only the generic kernel takes it
    specs[6] = (specs[6][0], specs[6][1], specs[6][2], 53)              # reference width: a launch of its own
    hists = run_batch(specs, n_sims)
    assert last_launch()[0] == 'mcgp::race_kernel_reg_wide<8>'          # the last launch of the call
    _check(specs, n_sims, hists)


def test_a_batch_of_solo_problems_only(require_gpu):
    n_sims = N_SIMS_1
    specs = [(c, s, o, 53) for c, s, o, _ in _many(5, 3, laps=9, seed0=30)]
    hists = run_batch(specs, n_sims)
    assert last_launch()[0].startswith('mcgp::race_kernel_reg_wide<')   # no shared launch
    _check(specs, n_sims, hists)


def test_field_sizes_interleaved(require_gpu):
    n_sims = N_SIMS_1
    e, f = _many(8, 3, laps=9, seed0=10), _many(5, 2, laps=9, seed0=20)
    specs = [e[0], f[0], e[1], f[1], e[2]]
    hists = run_batch(specs, n_sims)
    assert [h.shape[0] for h in hists] == [8, 5, 8, 5, 8]
    _check(specs, n_sims, hists)


# ---- 6. the workspace, re-used

def test_calls_of_other_sizes_on_one_context(require_gpu):
    big, refs = _many(3, 200), _many_references(3, 129, N_SIMS_2)
    refs = list(refs) + [reference(s[0], N_SIMS_2, *s[1:]) for s in big[129:]]
    first = run_batch(big, N_SIMS_2)
    small = _many(3, 2, seed0=7000)
    second = run_batch(small, N_SIMS_2)
    other = _many(23, 3, seed0=8000)
    third = run_batch(other, N_SIMS_2)
    last = run_batch(big, N_SIMS_2)
    _check(big, N_SIMS_2, first, refs)
    _check(small, N_SIMS_2, second)
    _check(other, N_SIMS_2, third)
    _check(big, N_SIMS_2, last, refs)
    assert all(np.array_equal(a, b) for a, b in zip(first, last))


# ---- 7. sim_offsets = NULL

def test_null_offsets_mean_zero(require_gpu):
    n_sims = N_SIMS_1
    specs = [(c, s, 0, d) for c, s, _, d in _many(6, 4, seed0=60)]
    null, zeros = RawBatch(specs), RawBatch(specs)
    assert null.call(n_sims, offsets=None) == 0
    assert last_launch()[0] == 'mcgp::race_kernel_reg_batch<6>'
    assert zeros.call(n_sims) == 0
    assert np.array_equal(null.hist, zeros.hist)
    _check(specs, n_sims, list(null.hist.astype(np.int64)))


# ---- 8. a device with less LDS than the batch kernel's block needs

_CHILD = (
    "import sys, numpy as np\n"
    "sys.path.insert(0, 'tests')\n"
    "from batch_cases import field, last_launch, reference, run_batch\n"
    "for n, k in ((20, 3), (21, 2), (10, 3)):\n"
    "    specs = [(field(n, (7, 60, 3)[i], shift=i, pace=0.04 * i), 90 + i, 64 * i + 1, 32) for i in range(k)]\n"
    "    hists = run_batch(specs, 600)\n"
    "    name, grid, block, lds = last_launch()\n"
    "    for (c, s, o, d), h in zip(specs, hists):\n"
    "        assert np.array_equal(h, reference(c, 600, s, o, d)), (n, s)\n"
    "    print(n, block, lds, name)\n")


def _child(limit):
    env = dict(os.environ, MCGP_LDS_PER_BLOCK=str(limit))
    return subprocess.run([sys.executable, '-c', _CHILD], capture_output=True, text=True, env=env, cwd=O.ROOT, timeout=600)


def test_a_device_with_less_lds_runs_the_problems_one_by_one(require_gpu):
    """The batch kernel has the default block shape only.  At 80 KB per block the 20- and 21-car blocks (163 264 and
    157 168 B, plus the batch's 16) do not fit: their problems run through the single-problem path in blocks of 4 waves, with
    the oracle's histograms; the 10-car block (69 072 + 16 B) fits and the shared launch runs."""
    r = _child(81920)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = {ln.split()[0]: ln.split(None, 3)[1:] for ln in r.stdout.strip().splitlines()}
    assert lines['20'][2] == 'mcgp::race_kernel_reg<20, 4>' and lines['20'][0] == '256', lines
    assert lines['21'][2] == 'mcgp::race_kernel_reg<21, 4>' and lines['21'][0] == '256', lines
    assert lines['10'][2] == 'mcgp::race_kernel_reg_batch<10>' and int(lines['10'][1]) == 69072 + 16, lines
    assert all(int(v[1]) <= 81920 for v in lines.values()), lines


def test_a_device_with_too_little_lds_fails_with_a_message(require_gpu):
    """At 32 KB not even the small block fits: the batch fails as mcgp_run does, with an error that says so."""
    r = _child(32768)
    assert r.returncode != 0 and 'bytes of LDS' in r.stderr, (r.returncode, r.stderr[-2000:])
