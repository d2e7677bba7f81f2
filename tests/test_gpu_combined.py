"""Combined what-if scenarios on the device (mcgp_run_combined, through the C ABI):

  1. the identities of include/mcgp.h: with no table, or with one table non-empty, the call is mcgp_run_strategies,
     mcgp_run_penalties, mcgp_run_events or mcgp_run_paces on the same arguments -- hist, delta, that call's own output and
     every order -- from the grid and from a lap-L // 2 state, on S60, EVT and fields of 32, 2 and 1 cars;
  2. the Python restatement (combined_ref) on the scenarios where the rule sets meet (combined_ref.meeting_scenarios);
  3. itself: the outputs are accumulated into, a split by sim_offset sums to the one call, several staging chunks equal
     one, and every count is the count of the returned orders and of the restatement's per-simulation results;
  4. the kernel's name, the `what-if` CLI end to end, and RaceSimulator.run_combined against the C call."""
import json

import numpy as np
import pytest

import combined_host_build as CH
import combined_ref as CR
import events_ref as ER
import oracle_py as O
import paces_ref as PR
import penalties_ref as NR
import resume_ref as RR
import strategy_ref as SR
from monte_carlo_gp_amd import PaceOffset, PitPlan, RaceConfig, RaceEvent, RaceSimulator, TimePenalty, cli
from monte_carlo_gp_amd import _native as N
from monte_carlo_gp_amd.simulation import DEFAULT_SET_POP

pytestmark = pytest.mark.gpu

KERNEL = 'mcgp::race_combined_kernel'
FIELDS = ['S60', 'EVT', 'n32', 'n2', 'n1']
M, M_REF, SEED, OFF = 200, 40, 47, 300
KEYS = ('hist', 'delta', 'fate', 'events', 'carried', 'orders')


def _case(name):
    return RR.field_case(int(name[1:])) if name[0] == 'n' else O.load_case(name)


def _run(case, scen, m, seed=SEED, off=OFF, **kw):
    """mcgp_run_combined under scenario() dicts -> dict(hist, delta, fate, events, carried, orders)."""
    rc, *out = CR.run_c(case, scen, m, seed, sim_offset=off, **kw)
    assert rc == 0, N.lib().mcgp_last_error().decode()
    assert N.lib().mcgp_last_kernel_name(0).decode() == KERNEL
    return dict(zip(KEYS, out))


def _ok(rc, *out):
    assert rc == 0, N.lib().mcgp_last_error().decode()
    return out


_traced = {}


def _ref(name):
    """The oracle's traced run of the case, computed once and shared."""
    if name not in _traced:
        _traced[name] = RR.traced_run(_case(name), M_REF, SEED, OFF)
    return _traced[name]


def _start(name, start):
    """(state or None, first lap with a pit step, keyword arguments of combined_ref.ref_run)."""
    case, ref = _case(name), _ref(name)
    if start == 'grid':
        return None, 2, dict(grids=ref['grids'])
    k = case['config']['total_laps'] // 2
    state = (RR.state_arrays(ref, 3, k), k, RR.drs_disabled_until(case, SEED, OFF + 3, k))
    return state, k + 1, dict(state=state)


def _leader(name):
    return int(np.bincount(_ref(name)['orders'][:, 0]).argmax())


def _trivial(a, m):
    return (a[:, :, 0] == m).all() and not a[:, :, 1:].any()


# ---------------------------------------------------------------- 1. the identities
def _single_kind_scenarios(n, L, first, pace_first):
    """[(plans)], [(penalties, plans)], [(overrides, plans)], [(offsets, plans)]: the siblings' own test scenarios where
    the field has the three drivers they name, else small ones on drivers 0 and n - 1."""
    z = n - 1
    plans = [{}, {0: (-1, 0, [(first + 3, 2)])}, {z: (-1, 0, [(first + 1, 1), (L - 5, 0)]), 0: (-1, 0, [])}]
    if n >= 3:
        return plans, NR.scenarios(first, L, n), ER.scenarios(first, L, n), PR.scenarios(pace_first, L, n)
    pens = [([], {}), ([(0, NR.FLAG, 0, 5.0)], {}), ([(z, NR.SERVE, first, 5.0), (0, NR.LAP, L, 3.0)], {}),
            ([(0, NR.SERVE, first, 10.0)], {0: (-1, 0, [(L, 0)])})]
    evs = [([], {}), ([(first, first, ER.SC)], {}), ([(first, L, ER.NONE)], {}), ([(L, L, ER.RED)], {}),
           ([(first + 2, first + 2, ER.VSC)], {z: (-1, 0, [(first + 2, 2)])})]
    offs = [([], {}), ([PR.laps(0, pace_first, L, 0.3)], {}), ([PR.until_stop(z, pace_first, 0.4)], {}),
            ([PR.until_stop(0, first + 2, 0.9), PR.laps(z, L, L, -0.5)], {0: (-1, 0, [(first + 2, 2)])})]
    return plans, pens, evs, offs


@pytest.mark.parametrize('start', ['grid', 'state'])
@pytest.mark.parametrize('name', FIELDS)
def test_with_at_most_one_table_the_call_is_that_table_s_own_call(require_gpu, name, start):
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    state, first, _ = _start(name, start)
    plans, pens, evs, offs = _single_kind_scenarios(n, L, first, 1 if start == 'grid' else first)
    kw = dict(sim_offset=OFF, state=state)
    # every count zero: mcgp_run_strategies, with zero count arrays and with NULL ones
    h, dl, o = _ok(*SR.run_c(case, plans, M, SEED, **kw))
    _, _, drawn, _ = _ok(*ER.run_c(case, plans, [[]] * len(plans), M, SEED, **kw))
    for null in (False, True):
        got = _run(case, [CR.scenario(p) for p in plans], M, state=state, null_counts=null)
        assert np.array_equal(got['orders'], o) and np.array_equal(got['hist'], h) and np.array_equal(got['delta'], dl)
        assert _trivial(got['fate'], M) and _trivial(got['carried'], M) and np.array_equal(got['events'], drawn)
    # penalties only
    pl = [p for _, p in pens]
    h, dl, ft, o = _ok(*NR.run_c(case, pl, [x for x, _ in pens], M, SEED, **kw))
    _, _, drawn, _ = _ok(*ER.run_c(case, pl, [[]] * len(pl), M, SEED, **kw))
    got = _run(case, [CR.scenario(p, penalties=x) for x, p in pens], M, state=state, null_counts=True)
    assert np.array_equal(got['orders'], o) and np.array_equal(got['hist'], h) and np.array_equal(got['delta'], dl)
    assert np.array_equal(got['fate'], ft) and _trivial(got['carried'], M) and np.array_equal(got['events'], drawn)
    # events only
    h, dl, ev, o = _ok(*ER.run_c(case, [p for _, p in evs], [x for x, _ in evs], M, SEED, **kw))
    got = _run(case, [CR.scenario(p, events=x) for x, p in evs], M, state=state, null_counts=True)
    assert np.array_equal(got['orders'], o) and np.array_equal(got['hist'], h) and np.array_equal(got['delta'], dl)
    assert np.array_equal(got['events'], ev) and _trivial(got['fate'], M) and _trivial(got['carried'], M)
    # offsets only
    pl = [p for _, p in offs]
    h, dl, ca, o = _ok(*PR.run_c(case, pl, [x for x, _ in offs], M, SEED, **kw))
    _, _, drawn, _ = _ok(*ER.run_c(case, pl, [[]] * len(pl), M, SEED, **kw))
    got = _run(case, [CR.scenario(p, paces=x) for x, p in offs], M, state=state, null_counts=True)
    assert np.array_equal(got['orders'], o) and np.array_equal(got['hist'], h) and np.array_equal(got['delta'], dl)
    assert np.array_equal(got['carried'], ca) and _trivial(got['fate'], M)
    # (offsets move the overtakes, not the events: the counts are those of the race as drawn)
    assert np.array_equal(got['events'], drawn)


def test_overrides_equal_to_what_a_simulation_drew_change_nothing_for_it(require_gpu):
    case = _case('EVT')
    L = case['config']['total_laps']
    base = _run(case, [CR.scenario()], M_REF)
    for i in (0, 7, M_REF - 1):
        evs = [(lap, lap, ER.drawn_event(case, SEED, OFF + i, lap)[0]) for lap in range(2, L + 1)]
        got = _run(case, [CR.scenario(events=evs)], 1, off=OFF + i)
        assert np.array_equal(got['orders'][0, 0], base['orders'][0, i])


# ---------------------------------------------------------------- 2. the restatement where the rules meet
@pytest.mark.parametrize('start', ['grid', 'state'])
@pytest.mark.parametrize('name', ['S60', 'EVT', 'n32'])
def test_device_equals_the_restatement_where_the_rules_meet(require_gpu, name, start):
    case = _case(name)
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    state, first, kw = _start(name, start)
    scen = CR.meeting_scenarios(first, L, n, _leader(name))
    want = CR.ref_run(case, scen, M_REF, SEED, OFF, **kw)
    want_o, want_f, _, _ = want
    # on the CPU first: every scenario changes an order, and both ways a penalty to serve can end occur
    for s in range(1, len(scen)):
        assert not np.array_equal(want_o[s], want_o[0]), s
    assert (want_f == CR.FATE_SERVED).any() and (want_f == CR.FATE_FLAG).any()
    got = _run(case, scen, M_REF, state=state)
    CH.check_against(got, case, want, M_REF)
    if start == 'grid':
        assert np.array_equal(got['orders'][0], _ref(name)['orders'])


# ---------------------------------------------------------------- 3. accumulation, split, chunks, counts of the orders
def test_outputs_accumulate_split_chunk_and_count_their_orders(require_gpu, monkeypatch):
    """200 simulations are several blocks and, under a cap of 64 per launch, four staging chunks with a short last one."""
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    scen = CR.meeting_scenarios(2, L, n, _leader('S60'))
    m, a, fill = M, 77, 7
    one = _run(case, scen, m, fill=fill)
    lo, hi = _run(case, scen, a), _run(case, scen, m - a, off=OFF + a)
    for k in KEYS[:-1]:
        assert np.array_equal(one[k], lo[k] + hi[k] + fill), k         # accumulated into what the buffers held
    assert np.array_equal(one['orders'], np.concatenate([lo['orders'], hi['orders']], axis=1))
    monkeypatch.setenv('MCGP_MAX_SIMS_PER_LAUNCH', '64')
    chunked = _run(case, scen, m)
    monkeypatch.delenv('MCGP_MAX_SIMS_PER_LAUNCH')
    for k in KEYS[:-1]:
        assert np.array_equal(chunked[k], one[k] - fill), k
    assert np.array_equal(chunked['orders'], one['orders'])
    o = one['orders']
    assert np.array_equal(chunked['hist'], NR.hist_counts(o, n)) and np.array_equal(chunked['delta'], SR.delta_counts(o, n))
    for k in ('fate', 'events', 'carried'):
        assert (chunked[k].sum(axis=2) == m).all(), k
    # fates, events and laps carried of the first 40 ids are the counts of the restatement's
    want = CR.ref_run(case, scen, M_REF, SEED, OFF, grids=_ref('S60')['grids'])
    first = _run(case, scen, M_REF)
    assert np.array_equal(first['orders'], o[:, :M_REF])
    CH.check_against(first, case, want, M_REF)
    # without delta, the three own outputs or orders the histogram is the same, and each output alone is itself
    none = _run(case, scen, m, orders=False, delta=False, fate=False, events=False, carried=False)
    assert np.array_equal(none['hist'], chunked['hist']) and not any(none[k].any() for k in KEYS[1:-1])
    for only in ('delta', 'fate', 'events', 'carried'):
        got = _run(case, scen, m, orders=False, **{k: k == only for k in ('delta', 'fate', 'events', 'carried')})
        assert np.array_equal(got[only], chunked[only]) and np.array_equal(got['hist'], chunked['hist']), only


# ---------------------------------------------------------------- 4. the kernel's name and the front door
def test_last_kernel_name(require_gpu):
    case = _case('n2')
    rc = CR.run_c(case, [CR.scenario()], 64, 1)[0]
    assert rc == 0 and N.lib().mcgp_last_kernel_name(0).decode() == KERNEL


def test_what_if_cli_end_to_end(require_gpu, tmp_path, capsys):
    out, pred = tmp_path / 'w.json', tmp_path / 'p.json'
    seed, m = 7, 20_000
    assert cli.main(['predict', '--race', 'Bahrain', '--offline', '--simulations', str(m), '--seed', str(seed),
                     '--json', str(pred)]) == 0
    win = json.load(open(pred))['win_probabilities']
    a, b = sorted(win, key=win.get, reverse=True)[:2]
    assert cli.main(['what-if', '--race', 'Bahrain', '--offline', '--driver', a, '--event', 'sc=sc@31', '--plan',
                     'sc=:31/HARD', '--give', f'sc={a}:5', '--offset', f'sc={b}:0.4@31+', '--simulations', str(m), '--seed',
                     str(seed), '--json', str(out)]) == 0
    text = capsys.readouterr().out
    assert 'scenario: as drawn' in text and 'scenario: sc   (laps with: safety car' in text
    assert 'penalty served at a stop' in text and 'offset carried' in text
    doc = json.load(open(out))
    rows = doc['scenarios']
    assert [r['scenario'] for r in rows] == ['as drawn', 'sc'] and doc['baseline'] == 'as drawn'
    for d in win:                                           # the race as drawn is predict's race
        assert rows[0]['win_probabilities'][d] == pytest.approx(win[d], abs=1e-12)
    assert list(rows[1]['drivers']) == [a, b] and rows[0]['drivers'][a]['p_same'] == 1.0
    fate = rows[1]['drivers'][a]['fate']
    assert fate['none'] == 0.0 and fate['served'] > 0.5 and sum(fate.values()) == pytest.approx(1.0)
    assert rows[1]['expected_events']['sc'] >= 1.0 and sum(rows[1]['drivers'][b]['laps_carried']) == pytest.approx(1.0)


@pytest.mark.parametrize('start', ['grid', 'state'])
def test_run_combined_is_the_c_call(require_gpu, start):
    case = _case('S60')
    L, n = case['config']['total_laps'], len(case['grid_probs'])
    d = list(case['grid_probs'])
    state, first, _ = _start('S60', start)
    k = first + 10
    scen = [CR.scenario(),
            CR.scenario({0: (-1, 0, [(k, 2)])}, [(0, CR.SERVE, k - 1, 5.0), (n - 1, CR.FLAG, 0, 10.0)], [(k, k, CR.SC)],
                        [PR.until_stop(1, k - 1, 0.4), PR.laps(2, first, L, -0.2)])]
    want = _run(case, scen, M, state=state)
    sim = RaceSimulator(RaceConfig(**case['config']), set_pop=DEFAULT_SET_POP)
    rs = RR.race_state(*state, d) if state is not None else None
    res = sim.run_combined(M, {
        'as drawn': {},
        'sc': dict(plans=[PitPlan(d[0], [(k, 'HARD')])],
                   penalties=[TimePenalty(d[0], 5.0, 'serve', k - 1), TimePenalty(d[n - 1], 10.0, 'flag')],
                   events=[RaceEvent('sc', k)],
                   paces=[PaceOffset(d[1], 0.4, until_stop_from=k - 1), PaceOffset(d[2], -0.2, laps=(first, L))]),
    }, case['base_pace'], case['tire_deg'], case['driver_variance'], case['driver_dnf_rates'],
        grid_probs=case['grid_probs'] if rs is None else None, state=rs, seed=SEED, sim_offset=OFF, drivers=d,
        return_orders=True, allow_single_compound=True)
    for key in KEYS:
        assert np.array_equal(getattr(res, key), want[key]), key
    assert res.names == ['as drawn', 'sc'] and res.until_from == {('sc', d[1]): k - 1}
    assert res.fate_probabilities('sc', d[0])['served'] > 0.5 and res.probability_of('sc', 'sc') == 1.0
