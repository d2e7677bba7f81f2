"""In-race odds, host side: the C-ABI argument checks of mcgp_run_from_state (no device needed), the shifted retirement
chain of race_common.hip.h compiled for the host against its numpy restatement, RaceState's JSON form and C arrays, and
the `in-race` CLI with a stand-in predictor."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
import resume_ref as RR
from monte_carlo_gp_amd import CarState, RaceConfig, RaceSimulator, RaceState, cli
from monte_carlo_gp_amd import _native as N

ROOT = O.ROOT


# ---------------------------------------------------------------- the C ABI without a device
def _arrays(n, lap=10, L=60):
    """A valid state of n cars after `lap` laps: car d on grid slot n - 1 - d, car 1 retired on lap 4."""
    a = dict(cumulative_time=np.array([100.0 * lap + d for d in range(n)], np.float64),
             last_lap_time=np.full(n, 91.5, np.float64),
             grid_slot=np.array([n - 1 - d for d in range(n)], np.uint8),
             compound=np.full(n, 1, np.uint8), used_compounds=np.full(n, 0b011, np.uint8),
             tire_age=np.full(n, 7, np.int16), retired_lap=np.zeros(n, np.int16))
    if n > 1:
        a['retired_lap'][1] = 4
    return a


def _abi_call(n=3, states=None, n_states=None, n_sims=100, device=0, deviates=32, hist=True, fill=0, orders=True,
              null_states=False):
    lib = N.lib()
    c = O.load_case('S60')
    from monte_carlo_gp_amd.simulation import _Problem, DEFAULT_SET_POP
    m = max(n, 1)
    prob = _Problem(RaceConfig(**c['config']), [f'D{i:02d}' for i in range(m)], {}, {}, {}, None, 'dry', DEFAULT_SET_POP,
                    deviates)
    states = states if states is not None else [(_arrays(m), 10, 0)]
    S = len(states)
    cs = (N.McgpRaceState * S)(*[RR.c_state(a, k, dd) for a, k, dd in states])
    h = np.full(S * 32 * 32, fill, np.uint64)
    o = np.full(S * max(n_sims, 1) * 32, fill % 256, np.uint8)
    rc = lib.mcgp_run_from_state(C.byref(prob.cfg), C.byref(prob.drv), n, S if n_states is None else n_states,
                                 None if null_states else cs, n_sims, None, 1, device,
                                 h.ctypes.data_as(C.POINTER(C.c_uint64)) if hist else None,
                                 o.ctypes.data_as(C.POINTER(C.c_uint8)) if orders else None)
    return rc, lib.mcgp_last_error().decode(), h, o


def _with(n=3, lap=10, dd=0, **fields):
    a = _arrays(n)
    for k, v in fields.items():
        a[k] = np.ascontiguousarray(v, a[k].dtype)
    return [(_arrays(n), 10, 0), (a, lap, dd)]          # the bad one is state 1


BAD = [
    (dict(lap=0), 'state 1: lap'),
    (dict(lap=61), 'state 1: lap'),
    (dict(dd=-1), 'state 1: drs_disabled_until'),
    (dict(dd=63), 'state 1: drs_disabled_until'),
    (dict(cumulative_time=[1.0, float('nan'), 3.0]), 'state 1: car 1: cumulative_time is not finite'),
    (dict(cumulative_time=[1.0, 2.0, float('inf')]), 'state 1: car 2: cumulative_time is not finite'),
    (dict(last_lap_time=[float('-inf'), 90.0, 90.0]), 'state 1: car 0: last_lap_time is not finite'),
    (dict(grid_slot=[0, 0, 1]), 'state 1: car 1: grid_slot'),
    (dict(grid_slot=[0, 1, 3]), 'state 1: car 2: grid_slot'),
    (dict(compound=[5, 1, 1]), 'state 1: car 0: compound'),
    (dict(used_compounds=[0b011, 0b100, 0b011]), 'state 1: car 1: used_compounds'),      # lacks its compound
    (dict(used_compounds=[0b100010, 0b010, 0b010]), 'state 1: car 0: used_compounds'),   # a sixth bit
    (dict(tire_age=[-1, 0, 0]), 'state 1: car 0: tire_age'),
    (dict(tire_age=[0, 0, 1023 - 50 + 1]), 'state 1: car 2: tire_age'),                   # 1023 - (60 - 10) is the most
    (dict(retired_lap=[0, 11, 0]), 'state 1: car 1: retired_lap'),
    (dict(retired_lap=[-2, 0, 0]), 'state 1: car 0: retired_lap'),
]


@pytest.mark.parametrize('fields,msg', BAD, ids=[m for _, m in BAD])
def test_library_rejects_each_bad_field_before_any_device_lookup(fields, msg):
    rc, err, h, o = _abi_call(states=_with(**fields), fill=7)
    assert rc == -1 and msg in err, (rc, err)
    assert (h == 7).all() and (o == 7).all()


def test_library_rejects_bad_calls():
    a = _arrays(3)
    cases = [
        (dict(hist=False), 'hist_out'),
        (dict(null_states=True), 'states'),
        (dict(n_states=0), 'n_states'),
        (dict(n_states=4097), 'n_states'),
        (dict(deviates=53), 'deviates'),
        (dict(n=0), 'n must be in [1, 32]'),
        (dict(n=33), 'n must be in [1, 32]'),
    ]
    for kw, msg in cases:
        rc, err, _, _ = _abi_call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    for key in ('cumulative_time', 'last_lap_time', 'grid_slot', 'compound', 'used_compounds', 'tire_age', 'retired_lap'):
        st = RR.c_state(a, 10, 0)
        setattr(st, key, None)
        cs = (N.McgpRaceState * 1)(st)
        lib = N.lib()
        from monte_carlo_gp_amd.simulation import _Problem, DEFAULT_SET_POP
        prob = _Problem(RaceConfig(**O.load_case('S60')['config']), ['A', 'B', 'C'], {}, {}, {}, None, 'dry',
                        DEFAULT_SET_POP)
        h = np.zeros(9, np.uint64)
        rc = lib.mcgp_run_from_state(C.byref(prob.cfg), C.byref(prob.drv), 3, 1, cs, 10, None, 1, 0,
                                     h.ctypes.data_as(C.POINTER(C.c_uint64)), None)
        assert rc == -1 and f'state 0: {key} is NULL' in lib.mcgp_last_error().decode()


def test_zero_simulations_need_no_device_and_limits_are_inclusive():
    edge = _arrays(3)
    edge['tire_age'][:] = [0, 1023 - 50, 5]
    edge['retired_lap'][:] = [10, 1, 0]
    edge['compound'][:] = [4, 0, 2]
    edge['used_compounds'][:] = [0b11111, 0b1, 0b100]
    first = _arrays(3)
    first['retired_lap'][1] = 1
    states = [(edge, 10, 12), (_arrays(3), 60, 62), (first, 1, 0)]
    rc, err, h, _ = _abi_call(states=states, n_sims=0, fill=3)
    assert rc == 0, err
    assert (h == 3).all()
    rc, err, _, _ = _abi_call(n=1, states=[(_arrays(1), 5, 0)] * 4096, n_sims=0, orders=False)
    assert rc == 0, err


def test_outputs_untouched_when_the_device_lookup_fails():
    rc, err, h, o = _abi_call(device=999, fill=7)
    assert rc == -2 and 'device' in err
    assert (h == 7).all() and (o == 7).all()


# ---------------------------------------------------------------- the shifted retirement chain on the host
@pytest.fixture(scope='module')
def chain(tmp_path_factory):
    d = tmp_path_factory.mktemp('chain')
    src = d / 'chain.cpp'
    src.write_text('#include "race_common.hip.h"\n'
                   'extern "C" uint32_t lap_after(uint32_t w, uint64_t t, int k, int L) '
                   '{ return mcgp::draw_retirement_lap_after(w, t, k, L); }\n'
                   'extern "C" uint32_t lap_full(uint32_t w, uint64_t t, int L) '
                   '{ return mcgp::draw_retirement_lap(w, t, L); }\n')
    so = d / 'chain.so'
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'tools', 'emu'),
                           '-I' + os.path.join(ROOT, 'monte_carlo_gp_amd', 'csrc'), '-o', str(so), str(src)])
    L = C.CDLL(str(so))
    for f in (L.lap_after, L.lap_full):
        f.restype = C.c_uint32
    L.lap_after.argtypes = [C.c_uint32, C.c_uint64, C.c_int, C.c_int]
    L.lap_full.argtypes = [C.c_uint32, C.c_uint64, C.c_int]
    return L


def test_shifted_chain_matches_the_restatement(chain):
    rng = np.random.default_rng(5)
    for p in (0.0, 1e-4, 0.02, 0.3, 1.0):
        t = RR.threshold(p)
        for L, k in ((60, 1), (60, 20), (60, 59), (60, 60), (25, 12), (2, 1)):
            ws = [0, 1, 2 ** 32 - 1, 2 ** 31] + [int(x) for x in rng.integers(0, 2 ** 32, 300)]
            for w in ws:
                got = chain.lap_after(w, t, k, L)
                assert got == RR.retirement_lap_after(w, t, k, L), (p, L, k, w)
                assert got == 0 or k + 1 <= got <= L
                assert chain.lap_full(w, t, L) == RR.retirement_lap(w, t, L)


def test_shifted_chain_hand_values(chain):
    # p = 1/2: t = q = 2^31; S_2 = 2^31, S_3 = 2^30, S_4 = 2^29 ...  w = 2^29 + 5 survives S_2, S_3 and fails S_4:
    # the full chain's lap 4 (its third lap), the chain shifted to start at lap 21 gives its third lap, 23
    t = 2 ** 31
    assert chain.lap_full(2 ** 29 + 5, t, 60) == 4
    assert chain.lap_after(2 ** 29 + 5, t, 20, 60) == 23
    assert chain.lap_after(2 ** 31, t, 20, 60) == 21          # fails the first threshold: the first lap after k
    assert chain.lap_after(0, t, 20, 40) == 0                 # survives every threshold of laps 21 .. 40 (S >= 2^12)
    assert chain.lap_after(0, t, 20, 60) == 53                # ... until S reaches 0 on the chain's lap 34 (S_j = 2^(33 - j)): lap 19 + 34
    assert chain.lap_after(123, 0, 20, 60) == 0               # t = 0 never retires
    assert chain.lap_after(0, 2 ** 32, 20, 60) == 21          # p >= 1 retires on the first lap after k
    # no lap left: L - k + 1 == 1
    for w in (0, 7, 2 ** 32 - 1):
        assert chain.lap_after(w, 2 ** 32, 60, 60) == 0
        assert chain.lap_after(w, t, 60, 60) == 0


# ---------------------------------------------------------------- RaceState
def _state():
    return RaceState.from_json({'lap': 30, 'drs_disabled_until': 31, 'cars': [
        {'driver': 'VER', 'cumulative_time': 2700.5, 'last_lap_time': 90.1, 'tire_compound': 'HARD', 'tire_age': 12,
         'used_compounds': ['MEDIUM', 'HARD'], 'retired_lap': 0},
        {'driver': 'NOR', 'cumulative_time': 1800.0, 'last_lap_time': 95.0, 'tire_compound': 'MEDIUM', 'tire_age': 20,
         'used_compounds': ['MEDIUM'], 'retired_lap': 20},
        {'driver': 'LEC', 'cumulative_time': 2702.25, 'last_lap_time': 90.3, 'tire_compound': 'SOFT', 'tire_age': 3,
         'used_compounds': ['SOFT', 'HARD'], 'retired_lap': 0},
    ]})


def test_race_state_json_round_trip():
    st = _state()
    assert all(isinstance(c, CarState) for c in st.cars)
    assert [c.driver for c in st.cars] == ['VER', 'NOR', 'LEC']
    assert st.cars[1].dnf and st.cars[1].lap == 20 and not st.cars[0].dnf and st.cars[0].lap == 30
    obj = st.to_json()
    assert RaceState.from_json(json.loads(json.dumps(obj))).to_json() == obj
    assert obj['cars'][0]['used_compounds'] == ['MEDIUM', 'HARD']
    assert obj['cars'][1]['retired_lap'] == 20 and obj['cars'][0]['retired_lap'] == 0
    assert RaceState.from_json({'lap': 3, 'cars': []}).drs_disabled_until == 0


def test_race_state_c_arrays():
    a = _state().arrays(['LEC', 'VER', 'NOR'], total_laps=57)
    assert a['grid_slot'].tolist() == [2, 0, 1]                     # the list index
    assert a['compound'].tolist() == [0, 2, 1]
    assert a['used_compounds'].tolist() == [0b101, 0b110, 0b010]     # bit per compound id
    assert a['retired_lap'].tolist() == [0, 0, 20]
    assert a['tire_age'].tolist() == [3, 12, 20]
    assert a['cumulative_time'].tolist() == [2702.25, 2700.5, 1800.0]
    assert a['last_lap_time'].tolist() == [90.3, 90.1, 95.0]
    # the current compound counts as used even if the JSON leaves it out (CarState.__post_init__)
    st = RaceState.from_json({'lap': 2, 'cars': [{'driver': 'A', 'cumulative_time': 1.0, 'last_lap_time': 1.0,
                                                   'tire_compound': 'WET', 'tire_age': 0, 'used_compounds': []}]})
    assert st.arrays(['A'])['used_compounds'].tolist() == [0b10000]


@pytest.mark.parametrize('edit,msg', [
    (lambda s: setattr(s.cars[2], 'tire_compound', 'ULTRA'), 'LEC: tire_compound'),
    (lambda s: s.cars[0].used_compounds.add('SUPER'), 'VER: used_compounds'),
    (lambda s: setattr(s.cars[0], 'cumulative_time', float('nan')), 'VER: cumulative_time'),
    (lambda s: setattr(s.cars[2], 'last_lap_time', float('inf')), 'LEC: last_lap_time'),
    (lambda s: setattr(s.cars[2], 'tire_age', -1), 'LEC: tire_age'),
    (lambda s: setattr(s.cars[0], 'tire_age', 1023), 'VER: tire_age'),
    (lambda s: setattr(s.cars[1], 'lap', 31), 'NOR: a retired car'),
    (lambda s: setattr(s, 'lap', 58), 'lap must be'),
    (lambda s: setattr(s, 'drs_disabled_until', 60), 'drs_disabled_until'),
    (lambda s: setattr(s.cars[1], 'driver', 'VER'), 'each once'),
])
def test_race_state_errors_name_the_driver(edit, msg):
    st = _state()
    edit(st)
    with pytest.raises(ValueError, match=msg):
        st.arrays(['VER', 'NOR', 'LEC'], total_laps=57)


def test_run_from_state_validates_before_the_device():
    case = O.load_case('S60')
    sim = RaceSimulator(RaceConfig(**case['config']))
    st = _state()
    st.cars[0].tire_compound = 'ULTRA'
    with pytest.raises(ValueError, match='VER'):
        sim.run_from_state(10, st, {}, {}, {})
    res = sim.run_from_state(0, [_state(), _state()], {}, {}, {})
    assert res == [{}, {}] and sim.last_histogram.shape == (2, 3, 3)
    assert sim.run_from_state(0, _state(), {}, {}, {}) == {} and sim.last_histogram.shape == (3, 3)


# ---------------------------------------------------------------- the CLI
class _FakePredictor:
    """predict_from_state's result shape from synthetic probabilities (no device)."""
    calls = []

    def __init__(self, device=0):
        pass

    def predict_from_state(self, season, race, fixture, state, n_simulations=0, seed=None):
        _FakePredictor.calls.append((race, season, len(state), n_simulations, seed))
        out = []
        for j, st in enumerate(state):
            drivers = [c.driver for c in st.cars]
            n = len(drivers)
            win = {d: (1.0 if i == j % n else 0.0) for i, d in enumerate(drivers)}
            pod = {d: (1.0 if i < 3 else 0.0) for i, d in enumerate(drivers)}
            out.append({'lap': st.lap, 'win_probabilities': win, 'podium_probabilities': pod,
                        'points_probabilities': pod, 'full_distributions': {}})
        return out


def test_in_race_cli(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, 'F1Predictor', _FakePredictor)
    _FakePredictor.calls = []
    a, b = tmp_path / 'a.json', tmp_path / 'b.json'
    a.write_text(json.dumps(_state().to_json()))
    st = _state()
    st.cars = [st.cars[2], st.cars[1], st.cars[0]]
    b.write_text(json.dumps(st.to_json()))
    out_json = tmp_path / 'out.json'
    base = ['in-race', '--race', 'Bahrain', '--season', '2024', '--offline', '--simulations', '50', '--seed', '3']
    assert cli.main(base + ['--state', str(a)]) == 0
    out = capsys.readouterr().out
    assert 'RACE WINNER PROBABILITIES' in out and 'PODIUM PROBABILITIES' in out and 'after lap 30' in out
    assert cli.main(base + ['--state', str(a), '--state', str(b), '--json', str(out_json)]) == 0
    out = capsys.readouterr().out
    assert _FakePredictor.calls == [('Bahrain', 2024, 1, 50, 3), ('Bahrain', 2024, 2, 50, 3)]
    header = [line for line in out.splitlines() if line.strip().startswith('S1')]
    assert header and header[0].split() == ['S1', 'S2']
    ver = [line.split() for line in out.splitlines() if line.startswith('VER ')]
    assert ver[0] == ['VER', '100.0%', '0.0%']                   # winner column per state
    res = json.loads(out_json.read_text())
    assert [r['state'] for r in res] == [str(a), str(b)] and res[1]['lap'] == 30
    assert 'full_distributions' not in res[0]
    # neither --offline nor --fixture: refused as predict refuses it
    assert cli.main(['in-race', '--race', 'Bahrain', '--state', str(a)]) == 2
    # the existing subcommands are still there
    with pytest.raises(SystemExit):
        cli.main(['in-race', '--race', 'Bahrain'])              # --state is required
