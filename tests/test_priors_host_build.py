"""race_scenario_kernel<false / true, kRulePriors> and priors_count executed on the host (tools/emu/emu_generic.cpp,
through priors_host_build) against a reference that is not a restatement of the kernel (priors_ref): the drawn offsets
from the oracle's Philox and inverse-normal in the header's arithmetic, bit for bit; every simulation's finishing order
from the pinned C oracle under base_pace[d] + float(x_d(i)), and from a state from paces_ref's restatement with LAPS
offsets of x_d(i).  Then the identities against the emulated strategy kernel, the groups, the bins, the limits, and the
100 inputs of generic_cases.run_inputs().  The staged data stay inside the chunk (guard items on both sides of all three
stagings, checked by priors_host_build on every call)."""
import numpy as np
import pytest

import kernel_host_build as KH
import oracle_py as O
import paces_ref as PR
import priors_host_build as QH
import priors_ref as QR
import resume_ref as RR
import strategy_ref as SR

SEED, OFFSET = 47, 300
EDGES = QR.SWEEP_EDGES


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the offsets
@pytest.mark.parametrize('n', [1, 2, 5, 32])
def test_offsets_are_the_reference_bit_for_bit(n):
    case = RR.field_case(n)
    items = QR.sweep_items(n)
    for seed, off in ((SEED, OFFSET), (SEED, 2 ** 32 - 3), (0x9E3779B97F4A7C15, 5)):    # across 2^32; a seed's high word
        got = QH.priors(case, None, [[], items], EDGES, 8, seed, off)
        want = QR.offsets(items, n, 8, seed, off)
        assert np.array_equal(_bits(got['offsets'][1]), _bits(want)), (seed, off)
        assert not _bits(got['offsets'][0]).any()                   # no item: +0.0f
        assert np.array_equal(got['bins'], QR.bins_of(got['offsets'], EDGES))
    assert len(np.unique(want)) == want.size                         # ... and the deviates are all different


def test_the_high_words_of_seed_and_id_reach_the_draw():
    n = 5
    items = QR.sweep_items(n)
    a = QR.offsets(items, n, 3, SEED, 2 ** 32 - 1)                   # ids 2^32 - 1, 2^32, 2^32 + 1
    assert not np.array_equal(a[1:], QR.offsets(items, n, 2, SEED, 0))
    assert not np.array_equal(QR.offsets(items, n, 2, SEED | 1 << 40, 0), QR.offsets(items, n, 2, SEED, 0))


# ---------------------------------------------------------------- every simulation against the pinned oracle
@pytest.mark.parametrize('name,m', [('S60', 64), ('EVT', 64), ('N10', 64), ('n32', 16), ('n2', 16), ('n1', 16)])
def test_every_simulation_is_the_oracle_under_its_drawn_base_pace(name, m):
    case = _case(name)
    n = len(case['grid_probs'])
    items = QR.sweep_items(n)
    got = QH.priors(case, None, [[], items], EDGES, m, SEED, OFFSET)
    x = QR.offsets(items, n, m, SEED, OFFSET)
    assert np.array_equal(_bits(got['offsets'][1]), _bits(x))
    base = O.Problem(case).run(m, rng=O.RNG_PHILOX, seed=SEED, sim_offset=OFFSET, want_orders=True)['orders']
    want = QR.orders(case, items, m, SEED, OFFSET, x=x)
    both = np.stack([base, want])
    bad = [i for i in range(m) if not np.array_equal(got['orders'][1, i], want[i])]
    assert not bad, f'{len(bad)} of {m} orders differ, first sim {bad[0]}'
    assert np.array_equal(got['orders'][0], base)
    assert np.array_equal(got['hist'], PR.hist_counts(both, n))
    assert np.array_equal(got['delta'], SR.delta_counts(both, n))
    assert np.array_equal(got['draws'], QR.draw_counts(both, np.stack([np.zeros_like(x), x]), EDGES))
    assert (got['draws'].sum(axis=(2, 3)) == m).all()
    if name == 'S60':
        assert (want != base).any(axis=1).all()                      # all 64 orders move against the undrawn race


@pytest.mark.parametrize('start', ['lap 1', 'lap L // 2', 'lap L - 1'])
@pytest.mark.parametrize('name', ['S60', 'n32'])
def test_from_a_state_every_simulation_is_the_restatement_under_laps_offsets(name, start):
    case = _case(name)
    n, L = len(case['grid_probs']), case['config']['total_laps']
    k = {'lap 1': 1, 'lap L // 2': L // 2, 'lap L - 1': L - 1}[start]
    ref = RR.traced_run(case, 4, SEED, OFFSET)
    state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFFSET + 3, k))
    items = QR.sweep_items(n)
    m = 16
    got = QH.priors(case, None, [[], items], EDGES, m, SEED, OFFSET, state=state)
    x = QR.offsets(items, n, m, SEED, OFFSET)                        # the deviates are those of the grid's simulations
    assert np.array_equal(_bits(got['offsets'][1]), _bits(x))
    want = QR.orders(case, items, m, SEED, OFFSET, state=state, x=x)
    base = PR.orders(case, m, SEED, OFFSET, state=state)[0]
    assert np.array_equal(got['orders'][1], want) and np.array_equal(got['orders'][0], base)
    if k < L - 1:
        assert not np.array_equal(want, base)


# ---------------------------------------------------------------- identities
def test_no_items_and_zero_sigmas_are_the_strategy_kernel():
    case = _case('EVT')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    plans = [{}, {0: (-1, 0, [(8, 2)])}, {1: (-1, 0, [(15, 1), (L - 5, 0)]), 0: (-1, 0, [])}]
    zero = [[QR.driver(d, 0.0) for d in range(n)], [QR.group(range(n), 0.0)],
            [QR.driver(0, 0.0), QR.group([0, n - 1], 0.0)]]
    m = 24
    hist, orders = KH.generic_strategy(case, plans, m, SEED, OFFSET)
    for scen in ([[]] * 3, zero):
        got = QH.priors(case, plans, scen, EDGES, m, SEED, OFFSET)
        assert np.array_equal(got['orders'], orders) and np.array_equal(got['hist'], hist)
        assert not (got['offsets'] != 0).any()
    ref = RR.traced_run(case, 4, SEED, OFFSET)
    k = L // 2
    state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFFSET + 3, k))
    plans = [{}, {0: (-1, 0, [(k + 1, 2)])}]
    hist, orders = KH.generic_strategy(case, plans, m, SEED, OFFSET, state=state)
    for scen in ([[]] * 2, zero[:2]):
        got = QH.priors(case, plans, scen, EDGES, m, SEED, OFFSET, state=state)
        assert np.array_equal(got['orders'], orders) and np.array_equal(got['hist'], hist)


def test_an_empty_scenario_beside_a_drawn_one_and_the_same_items_twice():
    case = _case('S60')
    n = len(case['grid_probs'])
    items = QR.sweep_items(n)
    m = 24
    _, orders = KH.generic_strategy(case, [{}], m, SEED, OFFSET)
    got = QH.priors(case, None, [[], items, list(reversed(items))], EDGES, m, SEED, OFFSET)
    assert np.array_equal(got['orders'][0], orders[0])
    assert not np.array_equal(got['orders'][1], orders[0])
    for key in ('orders', 'hist', 'delta', 'draws', 'bins'):
        assert np.array_equal(got[key][1], got[key][2]), key
    assert np.array_equal(_bits(got['offsets'][1]), _bits(got['offsets'][2]))


def test_doubling_every_sigma_doubles_every_offset():
    case = RR.field_case(32)
    items = QR.sweep_items(32)
    twice = [(kind, who, 2.0 * sigma) for kind, who, sigma in items]
    got = QH.priors(case, None, [items, twice], EDGES, 8, SEED, OFFSET)
    assert np.array_equal(_bits(got['offsets'][1]), _bits(np.float32(2.0) * got['offsets'][0]))
    assert (got['offsets'][0] != 0).all()


# ---------------------------------------------------------------- groups
def test_one_group_of_all_thirty_two_drivers():
    case = RR.field_case(32)
    got = QH.priors(case, None, [[QR.group(range(32), 0.3)]], EDGES, 8, SEED, OFFSET)
    x = got['offsets'][0]
    assert (_bits(x) == _bits(x[:, :1])).all() and len(np.unique(x[:, 0])) == 8
    assert np.array_equal(_bits(x), _bits(QR.offsets([QR.group(range(32), 0.3)], 32, 8, SEED, OFFSET)))


def test_groups_at_the_philox_block_boundary_and_members_without_an_own_item():
    case = RR.field_case(32)
    n = 32
    items = [QR.group([4, 9, 31], 0.2), QR.group([28, 29], 0.4), QR.group([3, 30], 0.1), QR.driver(9, 0.15),
             QR.driver(28, 0.05), QR.driver(0, 0.25)]
    m = 8
    got = QH.priors(case, None, [items], EDGES, m, SEED, OFFSET)
    x = got['offsets'][0]
    want = QR.offsets(items, n, m, SEED, OFFSET)
    assert np.array_equal(_bits(x), _bits(want))
    z4 = np.array([QR.deviate(SEED, OFFSET + i, 32 + 4) for i in range(m)])
    z28 = np.array([QR.deviate(SEED, OFFSET + i, 32 + 28) for i in range(m)])
    assert np.array_equal(x[:, 4], (0.2 * z4).astype(np.float32)) and np.array_equal(x[:, 31], x[:, 4])
    assert np.array_equal(x[:, 29], (0.4 * z28).astype(np.float32))
    assert not np.array_equal(x[:, 9], x[:, 4]) and not np.array_equal(x[:, 28], x[:, 29])
    untouched = [d for d in range(n) if d not in (0, 3, 4, 9, 28, 29, 30, 31)]
    assert not _bits(x[:, untouched]).any()
    assert np.array_equal(got['orders'][0], QR.orders(case, items, m, SEED, OFFSET, x=want))


# ---------------------------------------------------------------- bins
@pytest.mark.parametrize('edges', [(), tuple(-0.35 + 0.05 * i for i in range(15))])
def test_no_edges_and_fifteen_edges(edges):
    case = _case('N10')
    n = len(case['grid_probs'])
    items = QR.sweep_items(n)
    m = 48
    got = QH.priors(case, None, [[], items], edges, m, SEED, OFFSET)
    assert got['draws'].shape == (2, n, len(edges) + 1, n)
    assert np.array_equal(got['bins'], QR.bins_of(got['offsets'], edges))
    assert np.array_equal(got['draws'], QR.draw_counts(got['orders'], got['offsets'], edges))
    assert (got['draws'].sum(axis=(2, 3)) == m).all()
    if edges:
        assert len(np.unique(got['bins'][1])) == 16                 # every bin is hit
    else:
        assert np.array_equal(got['draws'][:, :, 0, :], got['hist'])


def test_an_edge_at_zero_takes_plus_and_minus_zero_into_the_upper_bin():
    case = RR.field_case(5)
    m = 16
    got = QH.priors(case, None, [[QR.driver(1, 0.0), QR.driver(2, 0.3)]], (0.0,), m, SEED, OFFSET)
    x = got['offsets'][0]
    assert not _bits(x[:, 0]).any()                                  # no item: +0.0f
    sign = _bits(x[:, 1]) >> 31
    assert not (x[:, 1] != 0).any() and sign.any() and not sign.all()      # sigma 0: -0.0f where z is negative
    assert (got['bins'][0][:, :2] == 1).all()
    assert np.array_equal(got['bins'][0][:, 2], (x[:, 2] >= 0).astype(np.uint8)) and len(set(got['bins'][0][:, 2])) == 2


def test_an_edge_at_a_drawn_value_takes_it_into_the_upper_bin():
    case = RR.field_case(5)
    items = QR.sweep_items(5)
    first = QH.priors(case, None, [items], (), 8, SEED, OFFSET)['offsets'][0]
    e = float(first[3, 2])
    below = float(np.nextafter(np.float32(e), np.float32(-np.inf)))
    got = QH.priors(case, None, [items], (below, e), 8, SEED, OFFSET)
    assert got['bins'][0][3, 2] == 2
    got = QH.priors(case, None, [items], (e, float(np.nextafter(np.float32(e), np.float32(np.inf)))), 8, SEED, OFFSET)
    assert got['bins'][0][3, 2] == 1
    assert np.array_equal(got['bins'], QR.bins_of(got['offsets'], (e, float(np.nextafter(np.float32(e), np.float32(np.inf))))))


@pytest.mark.parametrize('grid_x', [1, 3, 7])
def test_counting_kernel_does_not_depend_on_its_grid(grid_x):
    case = _case('S60')
    n = len(case['grid_probs'])
    items = QR.sweep_items(n)
    m = 37                                                          # no multiple of any grid
    hist, stage, bins, offs, delta, draws = QH.priors_raw(case, None, [[], items, items[:n]], EDGES, m, SEED, 11,
                                                          grid_x=grid_x, fill=5)
    orders = np.argsort(stage, axis=2).astype(np.uint8)
    want_d = SR.delta_counts(orders, n)
    want_d[:, :, n - 1] = 0                                         # the centre bin is the host's
    assert np.array_equal(delta, want_d) and np.array_equal(draws, QR.draw_counts(orders, offs, EDGES))
    assert np.array_equal(hist, PR.hist_counts(orders, n))
    # without the counting kernel nothing is counted, without offsets_out nothing is staged for it
    _, stage2, bins2, offs2, d2, c2 = QH.priors_raw(case, None, [[], items, items[:n]], EDGES, m, SEED, 11, count=False,
                                                    want_offsets=False)
    assert np.array_equal(stage2, stage) and np.array_equal(bins2, bins) and offs2 is None and not d2.any() and not c2.any()


# ---------------------------------------------------------------- limits
@pytest.mark.parametrize('L', [1, 2])
def test_races_of_one_and_two_laps(L):
    case = RR.field_case(5)
    case['config'] = dict(case['config'], total_laps=L)
    items = [QR.driver(d, 1.5) for d in range(5)] + [QR.group([0, 4], 1.0)]
    m = 32
    got = QH.priors(case, None, [[], items], EDGES, m, SEED, 5)
    x = QR.offsets(items, 5, m, SEED, 5)
    want = QR.orders(case, items, m, SEED, 5, x=x)
    assert np.array_equal(got['orders'][1], want) and not np.array_equal(got['orders'][1], got['orders'][0])
    if L == 2:
        ref = RR.traced_run(case, 2, SEED, 5)
        state = (RR.state_arrays(ref, 1, 1), 1, 0)
        got = QH.priors(case, None, [items], EDGES, m, SEED, 5, state=state)
        assert np.array_equal(got['orders'][0], QR.orders(case, items, m, SEED, 5, state=state, x=x))


def test_a_thousand_laps():
    case = RR.field_case(2)
    case['config'] = dict(case['config'], total_laps=1000)
    items = QR.sweep_items(2)
    got = QH.priors(case, None, [[], items], EDGES, 4, SEED, 1)
    assert np.array_equal(got['orders'][1], QR.orders(case, items, 4, SEED, 1))
    assert np.array_equal(got['draws'], QR.draw_counts(got['orders'], got['offsets'], EDGES))


def test_sixty_four_scenarios_of_sixty_four_items():
    n = 32
    case = RR.field_case(n)
    scen = [[QR.driver(d, 0.01 * ((s + d) % 40)) for d in range(n)] + [QR.group([(d + s) % n], 0.02 * ((s * 7 + d) % 11))
                                                                          for d in range(n)] for s in range(64)]
    assert all(len(sc) == 64 for sc in scen)
    m = 2
    got = QH.priors(case, None, scen, EDGES, m, SEED, 9)
    for s, items in enumerate(scen):
        x = QR.offsets(items, n, m, SEED, 9)
        assert np.array_equal(_bits(got['offsets'][s]), _bits(x)), s
        assert np.array_equal(got['orders'][s], QR.orders(case, items, m, SEED, 9, x=x)), s
    assert np.array_equal(got['draws'], QR.draw_counts(got['orders'], got['offsets'], EDGES))
    assert np.array_equal(got['delta'], SR.delta_counts(got['orders'], n))


def test_a_thousand_simulations_split_at_389():
    case = RR.field_case(3)
    items = QR.sweep_items(3)
    scen = [[], items]
    whole = QH.priors(case, None, scen, EDGES, 1000, SEED, OFFSET)
    a = QH.priors(case, None, scen, EDGES, 389, SEED, OFFSET)
    b = QH.priors(case, None, scen, EDGES, 611, SEED, OFFSET + 389)
    for key in ('hist', 'delta', 'draws'):
        assert np.array_equal(whole[key], a[key] + b[key]), key
    for key in ('orders', 'bins'):
        assert np.array_equal(whole[key], np.concatenate([a[key], b[key]], axis=1)), key
    assert np.array_equal(_bits(whole['offsets']), _bits(np.concatenate([a['offsets'], b['offsets']], axis=1)))
    assert (whole['draws'].sum(axis=(2, 3)) == 1000).all()


# ---------------------------------------------------------------- every input
def test_emulated_kernel_on_every_input():
    QR.check_sweep(lambda case, seed, scen: QH.priors(case, None, scen, QR.SWEEP_EDGES, QR.SWEEP_SIMS, seed, QR.SWEEP_OFFSET))
