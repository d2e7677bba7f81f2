"""Pace scenarios on the device (mcgp_run_paces, through the C ABI) against two independent references -- the pinned C
oracle under another base_pace (whole-race LAPS offsets from the grid and from states, an UNTIL_STOP offset no stop
clears) and the Python restatement (paces_ref) under mixed scenarios, at the limits and under the generated offset sets of
paces_cases on every input, from the grid and from states -- and against itself: the outputs are accumulated into, a split
by sim_offset sums to the one call, several staging chunks equal one, and hist, delta and carried are the counts of the
returned orders at simulation counts that leave a wave and a counting block ragged.  Wall time on an MI355X machine, in
one visit: this file 12.7 s (the two sweeps 4.0 s and 1.9 s) against 28.2 s for tests/test_gpu_stints_moves_fuzz.py, the
family's yardstick."""
import functools

import numpy as np
import pytest

import oracle_py as O
import paces_cases as PC
import paces_ref as PR
import resume_ref as RR
import strategy_ref as SR
from monte_carlo_gp_amd import _native as N

pytestmark = pytest.mark.gpu

KERNEL = 'mcgp::race_paces_kernel'
M, SEED, OFF = 200, 47, 300
X = [0.37, -0.21, 0.113, -0.57, 0.29, -0.083, 0.61]      # not round in binary, mixed signs


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


def _x(n):
    x = [X[d % 7] + 0.001 * (d // 7) for d in range(n)]
    if n >= 2:
        x[min(2, n - 1)] = 0.0
    return x


def _run(case, scen, m, seed, off=0, **kw):
    """mcgp_run_paces under [(offsets, plans)] -> dict(hist, delta, carried, orders)."""
    rc, h, dl, ca, o = PR.run_c(case, [pl for _, pl in scen], [offs for offs, _ in scen], m, seed, sim_offset=off, **kw)
    assert rc == 0, N.lib().mcgp_last_error().decode()
    assert N.lib().mcgp_last_kernel_name(0).decode() == KERNEL
    return dict(hist=h, delta=dl, carried=ca, orders=o)


_traced = {}


def _ref(name, shifted=False, m=M):
    key = (name, shifted, m)
    if key not in _traced:
        case = _case(name)
        if shifted:
            case = PR.with_base_pace(case, _x(len(case['grid_probs'])))
        _traced[key] = RR.traced_run(case, m, SEED, OFF)
    return _traced[key]


# ---------------------------------------------------------------- 1. the pinned oracle under another base pace
@pytest.mark.parametrize('name', ['S60', 'EVT', 'n32', 'n2', 'n1'])
def test_whole_race_offsets_are_the_oracle_under_another_base_pace(require_gpu, name):
    case = _case(name)
    n, L = len(case['grid_probs']), case['config']['total_laps']
    x = _x(n)
    same, want = _ref(name), _ref(name, shifted=True)
    got = _run(case, [([], {}), ([PR.laps(d, 1, L, x[d]) for d in range(n)], {})], M, SEED, OFF)
    for s, ref in enumerate((same, want)):
        bad = [i for i in range(M) if not np.array_equal(got['orders'][s, i], ref['orders'][i])]
        assert not bad, f'scenario {s}: {len(bad)} of {M} orders differ, first sim {bad[0]}'
        assert np.array_equal(got['hist'][s], RR.counts(ref['orders'], n))
    assert np.array_equal(got['delta'], SR.delta_counts(np.stack([same['orders'], want['orders']]), n))
    assert (got['carried'][:, :, 0] == M).all() and not got['carried'][:, :, 1:].any()
    assert not np.array_equal(want['trace']['cum'], same['trace']['cum'])       # the offset matters
    if n >= 2:
        assert not np.array_equal(want['orders'], same['orders'])
    # from the state of oracle simulation i under the other base pace after lap k, continued under the original case
    for k in sorted({1, L // 2, L - 1}):
        offs = [PR.laps(d, k + 1, L, x[d]) for d in range(n)]
        for i in (0, 17, M - 1):
            state = (RR.state_arrays(want, i, k), k, RR.drs_disabled_until(case, SEED, OFF + i, k))
            o = _run(case, [(offs, {})], 1, SEED, OFF + i, state=state)['orders']
            assert np.array_equal(o[0, 0], want['orders'][i]), (k, i)


def test_until_stop_that_no_stop_clears_is_the_oracle_under_another_base_pace(require_gpu):
    case = dict(O.load_case('S60'))
    case['config'] = dict(case['config'], total_laps=5)
    case['driver_dnf_rates'] = {d: 0.05 for d in case['driver_dnf_rates']}
    n, L, x = len(case['grid_probs']), 5, 0.437
    same = RR.traced_run(case, M, SEED, OFF)
    want = RR.traced_run(PR.with_base_pace(case, [x] + [0.0] * (n - 1)), M, SEED, OFF)
    got = _run(case, [([], {}), ([PR.until_stop(0, 1, x)], {})], M, SEED, OFF)
    assert np.array_equal(got['orders'][0], same['orders']) and np.array_equal(got['orders'][1], want['orders'])
    assert not np.array_equal(want['orders'], same['orders'])
    tr = want['trace']
    out = np.where(tr['dnf'][:, L - 1, 0] != 0, tr['dnf_lap'][:, L - 1, 0], 0)       # driver 0's retirement lap, or 0
    assert (out != 0).any() and (out == 0).any()
    assert np.array_equal(got['carried'][1, 0], np.bincount(np.where(out != 0, out - 1, 5), minlength=L + 1))
    assert (got['carried'][0, :, 0] == M).all() and (got['carried'][1, 1:, 0] == M).all()


# ---------------------------------------------------------------- 2. the restatement
def _against_the_restatement(case, scen, m, seed, off, state=None, grids=None):
    kw = dict(state=state) if state is not None else dict(grids=grids)
    got = _run(case, scen, m, seed, off, state=state)
    want = [PR.orders(case, m, seed, off, plans=pl, offsets=offs, **kw) for offs, pl in scen]
    want_o, want_c = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    PC.check_against(got, case, want_o, want_c, m)
    assert (got['carried'].sum(axis=2) == m).all()
    return want_o, want_c


@pytest.mark.parametrize('start', ['grid', 'state'])
@pytest.mark.parametrize('name', ['S60', 'EVT', 'n32'])
def test_device_equals_the_restatement(require_gpu, name, start):
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    m = 40
    ref = _ref(name)
    if start == 'grid':
        state, first = None, 1
    else:
        k = L // 2
        state, first = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFF + 3, k)), k + 1
    want_o, _ = _against_the_restatement(case, PR.scenarios(first, L, n), m, SEED, OFF, state=state, grids=ref['grids'])
    if start == 'grid':
        assert np.array_equal(want_o[0], ref['orders'][:m])


def test_offsets_of_cars_that_retire_before_and_after_their_first_lap(require_gpu):
    case = dict(O.load_case('S60'))
    case['driver_dnf_rates'] = {d: 0.03 for d in case['driver_dnf_rates']}
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    p, who = L // 2, [0, 7, n - 1]
    scen = [([], {}), ([PR.until_stop(d, p, 0.45 + 0.1 * d) for d in who], {d: (-1, 0, []) for d in who})]
    _, want_c = _against_the_restatement(case, scen, 40, SEED, OFF)
    c = want_c[1][:, who]
    assert (c == 0).any() and ((c > 0) & (c < L - p + 1)).any() and (c == L - p + 1).any()


# ---------------------------------------------------------------- 3. limits
def test_sixty_four_scenarios_of_sixty_four_single_lap_offsets(require_gpu):
    case = RR.field_case(3)
    case['config'] = dict(case['config'], total_laps=70)
    scen = [([PR.laps((s + lap) % 3, lap, lap, 0.05 * ((s + lap) % 9 - 4)) for lap in range(1, 65)], {}) for s in range(64)]
    _against_the_restatement(case, scen, 2, SEED, 9)


def test_a_thousand_laps(require_gpu):
    case = RR.field_case(2)
    case['config'] = dict(case['config'], total_laps=1000, dnf_rates={t: 0.0 for t in case['config']['dnf_rates']})
    case['driver_dnf_rates'] = {d: 0.0 for d in case['driver_dnf_rates']}       # both cars see the flag
    scen = [([], {}), ([PR.until_stop(0, 1, 0.4)], {0: (-1, 0, [])}),
            ([PR.until_stop(1, 1000, -0.3), PR.laps(0, 1, 1000, 0.25)], {}),
            ([PR.laps(1, 1, 500, 0.2), PR.laps(1, 501, 1000, -0.2), PR.until_stop(1, 2, 0.1)], {1: (-1, 0, [(1000, 1)])})]
    m = 2
    got = _run(case, scen, m, SEED, 1)
    _, want_c = _against_the_restatement(case, scen, m, SEED, 1)
    assert (want_c[1][:, 0] == 1000).all() and got['carried'][1, 0, 1000] == m      # c = L lands in column L


def test_a_race_of_one_lap(require_gpu):
    case = RR.field_case(3)
    case['config'] = dict(case['config'], total_laps=1)
    scen = [([], {}), ([PR.laps(0, 1, 1, 1.7)], {}), ([PR.until_stop(1, 1, -0.9), PR.laps(1, 1, 1, -0.8)], {})]
    want_o, _ = _against_the_restatement(case, scen, 40, SEED, 5)
    assert not np.array_equal(want_o[1], want_o[0]) and not np.array_equal(want_o[2], want_o[0])


# ---------------------------------------------------------------- 4. every input under generated offset sets
@functools.lru_cache(maxsize=None)
def _fuzz_inputs():
    return PC.fuzz_inputs()


def test_device_on_every_input_from_the_grid(require_gpu):
    def compare(case, seed, scen, want_o, want_c):
        got = _run(case, scen, PC.FUZZ_SIMS, seed, PC.FUZZ_OFFSET)
        PC.check_against(got, case, want_o, want_c, PC.FUZZ_SIMS)

    PC.fuzz_sweep(*_fuzz_inputs(), compare)


def test_device_on_every_input_from_a_state(require_gpu):
    """The gains of buffers of fives are the restatement's counts."""
    def compare(case, seed, scen, want_o, want_c, state):
        got = _run(case, scen, PC.FUZZ_SIMS, seed, 0, state=state, fill=5)
        got = {k: v - 5 if k != 'orders' else v for k, v in got.items()}
        PC.check_against(got, case, want_o, want_c, PC.FUZZ_SIMS)
        assert (got['carried'].sum(axis=2) == PC.FUZZ_SIMS).all()

    PC.state_sweep(*_fuzz_inputs(), compare)


def test_chunks_from_a_state(require_gpu, monkeypatch):
    """200 simulations under a cap of 64 per launch are four staging chunks with a short last one, with and without the
    staging of the laps carried."""
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    k, m = L // 2, 200
    state = (RR.state_arrays(_ref('S60'), 3, k), k, RR.drs_disabled_until(case, SEED, OFF + 3, k))
    scen = PR.scenarios(k + 1, L, n)
    whole = _run(case, scen, m, SEED, OFF, state=state)
    monkeypatch.setenv('MCGP_MAX_SIMS_PER_LAUNCH', '64')
    chunked = _run(case, scen, m, SEED, OFF, state=state)
    bare = _run(case, scen, m, SEED, OFF, state=state, carried=False, orders=False)
    monkeypatch.delenv('MCGP_MAX_SIMS_PER_LAUNCH')
    for key in ('hist', 'delta', 'carried', 'orders'):
        assert np.array_equal(chunked[key], whole[key]), key
    assert np.array_equal(bare['hist'], whole['hist']) and np.array_equal(bare['delta'], whole['delta'])
    assert not bare['carried'].any() and bare['orders'] is None
    o = whole['orders']
    assert np.array_equal(whole['hist'], PR.hist_counts(o, n)) and np.array_equal(whole['delta'], SR.delta_counts(o, n))
    assert (whole['carried'].sum(axis=2) == m).all() and (whole['carried'][1:, :, 1:] > 0).any() and (o[1:] != o[0]).any()


@pytest.mark.parametrize('n', [31, 3])
def test_ragged_counts(require_gpu, n):
    """Simulation counts one short of, one past and far from a wave, two waves and a counting block: the restatement up to
    65 simulations, beyond that the counts of the returned orders and the sum of split calls."""
    name, seed, off = f'n{n}', 5, PC.FUZZ_OFFSET
    case = _case(name)
    L = case['config']['total_laps']
    scen = PC.scenarios(name, case) + PR.scenarios(1, L, n)[3:6]
    grids = RR.traced_run(case, 65, seed, off)['grids']
    want = [PR.orders(case, 65, seed, off, plans=pl, offsets=offs, grids=grids) for offs, pl in scen]       # once, cut to m
    want_o, want_c = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    for m in (1, 63, 65, 129, 257):
        got = _run(case, scen, m, seed, off)
        assert np.array_equal(got['hist'], PR.hist_counts(got['orders'], n)), (n, m)
        assert np.array_equal(got['delta'], SR.delta_counts(got['orders'], n)), (n, m)
        assert (got['carried'].sum(axis=2) == m).all(), (n, m)
        if m <= 65:
            PC.check_against(got, case, want_o[:, :m], want_c[:, :m], m)
        else:
            a = m // 2 + 1
            lo, hi = _run(case, scen, a, seed, off), _run(case, scen, m - a, seed, off + a)
            for key in ('hist', 'delta', 'carried'):
                assert np.array_equal(got[key], lo[key] + hi[key]), (n, m, key)
            assert np.array_equal(got['orders'], np.concatenate([lo['orders'], hi['orders']], axis=1))
            assert (got['carried'][1:, :, 1:] > 0).any()


# ---------------------------------------------------------------- 5. accumulation, split, counts of the orders
def test_a_thousand_simulations_accumulate_split_and_count_their_orders(require_gpu):
    """1 000 simulations are several blocks and no multiple of 64 or 256."""
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    full = PR.scenarios(1, L, n)
    scen = [full[0], full[4], full[5]]          # none; UNTIL_STOP cleared by rule stops; cleared by a planned stop
    m, a, fill = 1000, 389, 7
    one = _run(case, scen, m, SEED, OFF, fill=fill)
    lo = _run(case, scen, a, SEED, OFF)
    hi = _run(case, scen, m - a, SEED, OFF + a)
    for k in ('hist', 'delta', 'carried'):
        assert np.array_equal(one[k], lo[k] + hi[k] + fill), k      # accumulated into what the buffers held
    assert np.array_equal(one['orders'], np.concatenate([lo['orders'], hi['orders']], axis=1))
    o = one['orders']
    assert np.array_equal(one['hist'] - fill, PR.hist_counts(o, n))
    assert np.array_equal(one['delta'] - fill, SR.delta_counts(o, n))
    carried = one['carried'] - fill
    assert (carried.sum(axis=2) == m).all() and (carried[0, :, 0] == m).all()
    assert carried[1, n - 1, 1:].sum() > 0 and carried[2, 0, 1] > m // 2
    # the laps carried of the first 40 ids are the restatement's
    first = _run(case, scen, 40, SEED, OFF)
    ref = RR.traced_run(case, 40, SEED, OFF)
    want = [PR.orders(case, 40, SEED, OFF, plans=pl, offsets=offs, grids=ref['grids']) for offs, pl in scen]
    assert np.array_equal(first['orders'], o[:, :40]) and np.array_equal(np.stack([w[0] for w in want]), o[:, :40])
    assert np.array_equal(first['carried'], PR.carried_counts(np.stack([w[1] for w in want]), L))
    # without delta, carried or orders the histogram is the same
    rc, h1, d1, c1, _ = PR.run_c(case, [pl for _, pl in scen], [offs for offs, _ in scen], m, SEED, sim_offset=OFF,
                                 orders=False, delta=False, carried=False)
    assert rc == 0 and np.array_equal(h1, one['hist'] - fill) and not d1.any() and not c1.any()


# ---------------------------------------------------------------- 6. the kernel's name
def test_last_kernel_name(require_gpu):
    case = _case('n2')
    rc = PR.run_c(case, None, [[]], 64, 1)[0]
    assert rc == 0 and N.lib().mcgp_last_kernel_name(0).decode() == KERNEL
