"""champ_given run from its source on the host (tools/emu/emu_champ.cpp: blocks of 256 real threads, the library's own
key layout from csrc/champ_pack.h) behind champ_accumulate, against championship_live_ref: every cell of the
[driver][position][champion] table equal, with the table in LDS and by global atomics."""
import numpy as np
import pytest

import champ_given_host_build as H
import championship_live_ref as LR
import championship_ref as CR

SIZES = [1, 2, 3, 9, 10, 22, 23, 32]                # key widths of 1 (n <= 9), 2 (n <= 22) and 3 words
SIMS = [1, 63, 64, 65, 500]                         # tail tiles; at odd n a tail whose byte count is no multiple of 4
TABLES = [[3, 2, 1], [2, 1], [3, 2, 1]]             # short tables: many ties on points, decided by countback or index
CB = [1, 0, 1]


def _perms(rng, sims, n):
    return rng.permuted(np.tile(np.arange(n, dtype=np.uint8), (sims, 1)), axis=1)


@pytest.mark.parametrize('sims', SIMS)
@pytest.mark.parametrize('n', SIZES)
def test_random_orders(n, sims):
    """Three races of random orders, the given race first, middle and last, a key buffer of exactly the simulations and
    a wider one, both histogram modes; carried-in points that tie."""
    rng = np.random.default_rng(1000 * n + sims)
    orders = [_perms(rng, sims, n) for _ in TABLES]
    ip = rng.integers(0, 3, n)
    ic = rng.integers(0, 2, (n, n))
    champ = CR.histogram(CR.rank(*CR.standings(orders, TABLES, CB, ip, ic)), n)
    assert H.given_run(orders, TABLES, CB, 0, ip, ic)[1]['words'] == (16 + 5 * n + 63) // 64
    for given in (0, 1, 2):
        ref = LR.title_given(orders, TABLES, CB, given, ip, ic)
        LR.check_invariants(ref, CR.race_histogram(orders[given]), champ)
        for in_lds in (True, False):
            for cap in (sims, sims + 37):
                out, info = H.given_run(orders, TABLES, CB, given, ip, ic, cap=cap, in_lds=in_lds)
                assert np.array_equal(out, ref), (given, in_lds, cap)
                assert info['lds_bytes'] == (256 * n + 15) // 16 * 16 + (4 * n ** 3 if in_lds else 0)


@pytest.mark.parametrize('n,b', [(10, 14), (11, 9), (12, 4), (23, 13), (24, 8), (25, 3)])
def test_points_across_the_word_boundary(n, b):
    """The sizes at which the points field straddles a key word, b of its bits in the lower word: every driver carries in
    2^b - (1 .. 6) points, so the tables (8 points at most) take some totals, not all, to 2^b and above, where the upper
    word's part of the field is no longer zero and the compare has to order it above the lower word.  259 simulations: a
    tail tile of 3."""
    rng = np.random.default_rng(7000 + n)
    sims = 259
    orders = [_perms(rng, sims, n) for _ in TABLES]
    ip = (1 << b) - rng.integers(1, 7, n)
    ic = rng.integers(0, 2, (n, n))
    pts, cnt = CR.standings(orders, TABLES, CB, ip, ic)
    above = (pts >= 1 << b).sum(axis=1)
    mixed = int(((above > 0) & (above < n)).sum())
    champions = len(set(np.argmin(CR.rank(pts, cnt), axis=1).tolist()))
    print(f'n = {n}: {mixed} of {sims} simulations with totals on both sides of 2^{b}, {champions} distinct champions')
    assert mixed >= 200 and champions >= 10
    for given in (0, 2):
        ref = LR.title_given(orders, TABLES, CB, given, ip, ic)
        for in_lds in (True, False):
            out, info = H.given_run(orders, TABLES, CB, given, ip, ic, in_lds=in_lds)
            assert np.array_equal(out, ref), (given, in_lds)
            assert info['words'] == (16 + 5 * n + 63) // 64


@pytest.mark.parametrize('in_lds', [True, False])
@pytest.mark.parametrize('n', [3, 23])
def test_chunks_and_grid_stride(n, in_lds):
    """700 simulations in chunks of 300 (the last chunk shorter than the key stride; every chunk starts the kept orders
    and the keys afresh), three tiles on one block and on two, and a second run that accumulates."""
    rng = np.random.default_rng(n)
    orders = [_perms(rng, 700, n) for _ in TABLES]
    ref = LR.title_given(orders, TABLES, CB, 1)
    for grid in (1, 2):
        out, _ = H.given_run(orders, TABLES, CB, 1, cap=300, in_lds=in_lds, acc_grid=grid, given_grid=grid)
        assert np.array_equal(out, ref), grid
    raw = np.zeros((n, n, n), np.uint64)
    H.given_run(orders, TABLES, CB, 1, in_lds=in_lds, into=raw)
    twice, _ = H.given_run(orders, TABLES, CB, 1, in_lds=in_lds, into=raw)
    assert np.array_equal(twice, 2 * ref)


@pytest.mark.parametrize('in_lds', [True, False])
def test_full_tie_goes_to_driver_0(in_lds):
    """Two drivers, points [1, 0], two races that do not count back, the wins split in every simulation: both end on one
    point with equal keys, and the champion is the lower index."""
    sims = 130
    a = np.tile(np.array([[0, 1]], np.uint8), (sims, 1))
    a[::2] = [1, 0]
    b = a[:, ::-1].copy()
    for given, o in ((0, a), (1, b)):
        out, _ = H.given_run([a, b], [[1, 0]] * 2, [0, 0], given, in_lds=in_lds)
        assert np.array_equal(out, LR.title_given([a, b], [[1, 0]] * 2, [0, 0], given))
        assert out[:, :, 1].sum() == 0 and np.array_equal(out[:, :, 0], CR.race_histogram(o))


@pytest.mark.parametrize('in_lds', [True, False])
@pytest.mark.parametrize('n', [1, 10, 23])
def test_zero_points_table(n, in_lds):
    """No race scores or counts back: every key is the initial (zero) key and the champion is driver 0 everywhere."""
    rng = np.random.default_rng(n)
    orders = [_perms(rng, 100, n) for _ in range(2)]
    out, _ = H.given_run(orders, [[0] * n] * 2, [0, 0], 1, in_lds=in_lds)
    assert out[:, :, 1:].sum() == 0 and np.array_equal(out[:, :, 0], CR.race_histogram(orders[1]))
