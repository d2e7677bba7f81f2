"""Offline race-weekend orchestrator: the caller side of the hot path.

Builds every input of RaceSimulator.run_monte_carlo the way the reference's
F1Predictor.predict_weekend does (reference src/predictor.py:186-319), but from a RACE FIXTURE
(a plain dict / JSON file) instead of FastF1 sessions, so it runs without network
("next" rows 1 and 3 of SURVEY.md 8f).  Differences from the reference, on purpose:
`n_simulations` and `seed` are real arguments (the reference hard-codes 10000 and passes no seed,
:283-291; its CLI flag is ignored, main.py:14-15,27-31).

Race fixture keys
    drivers            list of driver codes (order = practice-data order in the reference, :186)
    quali_ratings      {driver: Elo quali rating}            (what the Elo history would have produced)
    quali_features     {driver: {teammate_delta, form_score, circuit_affinity}}   optional
    race_features      {driver: {clutch_factor, dnf_probability, team_trend, wet_performance}}  optional
    practice           {base_pace: {}, tire_deg: {}, tire_compounds: {}}   (outputs of :409-569)
    weather            {rainfall: bool, ...}
"""
from __future__ import annotations

import json

import numpy as np

from . import config as K
from .elo import F1EloSystem
from .simulation import RaceConfig, RaceSimulator

PENALTY_TYPES = {'engine': 10, 'full_pu': 20, 'gearbox': 5, 'pitlane_start': 20}   # reference src/config.py:81-86
UNCERTAINTY = {'fp1': 1.5, 'fp2': 1.2, 'fp3': 1.0, 'quali': 0.9, 'sprint': 0.85}   # reference :241-247
CONFIDENCE = {'fp1': 'low', 'fp2': 'moderate', 'fp3': 'good', 'quali': 'high', 'sprint': 'high'}   # :294-300


def circuit_info(race: str) -> dict:
    """CIRCUITS lookup by exact key, else by substring of the event name, else defaults (:20-43)."""
    if race in K.CIRCUITS:
        return K.CIRCUITS[race]
    low = race.lower()
    for name, info in K.CIRCUITS.items():
        if name.lower() in low:
            return info
    return {'laps': 58, 'pit_loss': 22.0, 'drs_zones': 2, 'overtake_delta': 0.8}


def create_race_config(info: dict, tire_compounds: dict | None = None) -> RaceConfig:
    """RaceConfig with the reference's hard-coded SC / VSC / red-flag / DRS constants (:45-67)."""
    return RaceConfig(
        total_laps=info.get('laps', 58), pit_loss=info.get('pit_loss', 22.0),
        overtake_delta=info.get('overtake_delta', 0.8), sc_probability=K.SC_PROBABILITY,
        vsc_probability=K.VSC_PROBABILITY, red_flag_probability=K.RED_FLAG_PROBABILITY,
        dnf_rates=K.DEFAULT_DNF_RATES, drs_zones=info.get('drs_zones', 2), drs_delta=K.DRS_DELTA,
        tire_compounds=tire_compounds or K.TIRE_COMPOUNDS, driver_teams=K.DRIVER_TEAMS)


def _penalty_value(p):
    return PENALTY_TYPES.get(p, 0) if isinstance(p, str) else p


def apply_grid_penalties(quali_positions: dict, penalties: dict) -> dict:
    """Grid after penalties: sort by (position + penalty, original position) (:69-97)."""
    ranked = sorted(quali_positions.items(), key=lambda kv: kv[1])
    shifted = sorted(((pos + _penalty_value(penalties.get(d, 0)), pos, d) for d, pos in ranked))
    return {d: i + 1 for i, (_, _, d) in enumerate(shifted)}


def predict_quali(elo: F1EloSystem, drivers, features: dict) -> dict:
    """Grid-slot distribution per driver: softmax pole probability, teammate / form / circuit
    adjustments, then a Gaussian bump around (1 - p) n with sigma max(1, n/4) (:321-375; Q22)."""
    if not drivers:
        return {}
    pole = elo.predict_quali_probs(drivers)
    for d in drivers:
        delta = features.get(d, {}).get('teammate_delta', 0)
        if delta != 0 and d in pole:
            pole[d] = pole[d] * max(0.5, min(1.5, 1 + (delta * 0.25)))
    total = sum(pole.values())
    if total > 0:
        pole = {d: p / total for d, p in pole.items()}
    n = len(drivers)
    sigma = max(1.0, n / 4)
    slots = np.arange(n)
    out = {}
    for d in drivers:
        f = features.get(d, {})
        p = pole.get(d, 1 / n) * (1 + f.get('form_score', 0) * 0.15 + f.get('circuit_affinity', 0) * 0.10)
        p = max(0.001, min(0.999, p))
        expected = (1 - p) * n
        bump = [np.exp(-((pos - expected) ** 2) / (2 * sigma ** 2)) for pos in slots.tolist()]
        s = sum(bump)
        out[d] = [b / s for b in bump] if s > 0 else [1.0 / n] * n
    return out


def adjust_for_penalties(quali_probs: dict, penalties: dict) -> dict:
    """Shift each penalised driver's distribution towards the back; mass past the last slot piles
    up there, a penalty >= n puts all mass on the last slot (:377-407)."""
    out = {}
    for d, probs in quali_probs.items():
        pen = _penalty_value(penalties.get(d, 0))
        n = len(probs)
        if pen > 0 and n > 0:
            if pen >= n:
                out[d] = [0.0] * (n - 1) + [1.0]
            else:
                shifted = [0.0] * n
                for i, p in enumerate(probs):
                    shifted[min(i + pen, n - 1)] += p
                out[d] = shifted
        else:
            out[d] = probs
    return out


def actual_grid_probs(drivers, actual_grid: dict) -> dict:
    """One-hot grid distributions from a known grid; unknown / out-of-range drivers on the last slot (:189-205)."""
    n = len(drivers)
    out = {}
    for d in drivers:
        probs = [0.0] * n
        pos = actual_grid[d] - 1 if d in actual_grid else -1
        probs[pos if 0 <= pos < n else -1] = 1.0
        out[d] = probs
    return out


def _open_fixture(fixture, season, race) -> dict:
    """The race fixture, read from its JSON file if `fixture` is a path; a weekend without drivers raises (:183-184)."""
    if isinstance(fixture, str):
        with open(fixture) as f:
            fixture = json.load(f)
    if not fixture.get('drivers'):
        raise ValueError(f"No practice data available for {season} {race}")
    return fixture


class F1Predictor:
    """predict_weekend over a race fixture; the Monte Carlo step runs on the GPU."""

    def __init__(self, device: int = 0, device_front_end: bool = False):
        """device_front_end: build the grid-probability matrix on the GPU next to the race kernel
        instead of on the host; the matrices agree to ~1e-15 (the device uses its own exp, csrc/frontend_exp.h)."""
        self.elo_system = F1EloSystem()
        self.device = device
        self.device_front_end = device_front_end

    def simulator_inputs(self, fixture: dict, race: str, grid_penalties=None, circuit=None,
                         prediction_point: str = 'fp2', actual_grid=None):
        """Everything predict_weekend computes before the run_monte_carlo call (:186-281)."""
        grid_penalties = grid_penalties or {}
        circuit = circuit or circuit_info(race)
        drivers = list(fixture['drivers'])
        for d, r in fixture.get('quali_ratings', {}).items():
            self.elo_system.ratings.setdefault(d, {'quali': self.elo_system.initial, 'race': self.elo_system.initial})
            self.elo_system.ratings[d]['quali'] = r
        if actual_grid and prediction_point in ('quali', 'sprint'):
            quali_probs = actual_grid_probs(drivers, actual_grid)
        else:
            quali_probs = predict_quali(self.elo_system, drivers, fixture.get('quali_features', {}))
        if grid_penalties:
            quali_probs = adjust_for_penalties(quali_probs, grid_penalties)

        practice = fixture.get('practice', {})
        base_pace = dict(practice.get('base_pace', {}))
        tire_deg = dict(practice.get('tire_deg', {}))
        feats = fixture.get('race_features', {})
        mult = UNCERTAINTY.get(prediction_point, 1.0)
        variance = {}
        for d in drivers:                                            # :235-252
            v = max(0.05, min(0.25, 0.15 * (1 - feats.get(d, {}).get('clutch_factor', 0) * 0.2)))
            variance[d] = min(0.3, v * mult)
        config = create_race_config(circuit, practice.get('tire_compounds'))
        dnf = {d: feats.get(d, {}).get('dnf_probability', 0.05) / config.total_laps for d in drivers}   # :258-261
        weather = fixture.get('weather', {})
        track = 'damp' if weather.get('rainfall', False) else 'dry'                                    # :268
        for d in drivers:                                            # :271-274
            base_pace[d] = base_pace.get(d, 90.0) - (feats.get(d, {}).get('team_trend', 0) * 0.6)
        if track in ('damp', 'wet'):                                 # :277-281
            for d in drivers:
                base_pace[d] = base_pace[d] - (feats.get(d, {}).get('wet_performance', 0) * 0.5)
        return dict(config=config, drivers=drivers, grid_probs=quali_probs, base_pace=base_pace, tire_deg=tire_deg,
                    driver_variance=variance, driver_dnf_rates=dnf, track_condition=track, weather=weather)

    def predict_weekend(self, season: int, race: str, fixture: dict | str, grid_penalties=None, circuit_info=None,
                        prediction_point: str = 'fp2', actual_grid=None, n_simulations: int = 10000,
                        seed: int | None = None, matchups: bool = False, trace: bool = False, gaps=None,
                        conditions=None, tyres: bool = False, moves: bool = False, pit_window=None,
                        pace_uncertainty=None) -> dict:
        """Pole / win / podium probabilities for one weekend (:99-319), Monte Carlo on the GPU.

        matchups=True (not in the reference): the race runs through RaceSimulator.run_matchups -- the same simulations,
        so every key keeps its value -- and the result gains 'head_to_head' ({a: {b: P(a ahead of b)}}),
        'teammate_battles' (MatchupResult.teammate_battles over the race config's teams) and 'likely_podiums' (the
        MATCHUP_PODIUMS most likely ordered podiums, [{'podium': [P1, P2, P3], 'probability': p}]).

        trace=True (not in the reference): the race also runs through RaceSimulator.run_trace -- again the same
        simulations -- and the result gains the keys of trace_keys: 'leader_by_lap', 'expected_laps_led',
        'pit_stop_distribution', 'fastest_lap_probabilities' and 'race_event_probabilities'.

        gaps=True, or {'edges': [...], 'pairs': [(a, b), ...]} (not in the reference): the race also runs through
        RaceSimulator.run_gaps -- the same simulations once more -- and the result gains 'gaps', the block gap_keys
        builds: the winning-margin distribution, each driver's finishing-gap distribution and the requested pairs.

        conditions={name: text} (not in the reference; the grammar is in conditions.py): the race also runs through
        RaceSimulator.run_conditions -- the same simulations -- and the result gains 'conditions', the block
        condition_keys builds: per name the probability, its standard error and the win / podium odds given the
        condition beside the unconditional ones.

        tyres=True (not in the reference): the race also runs through RaceSimulator.run_stints -- the same simulations --
        and the result gains 'tyres', the block tyre_keys builds: per driver the stop-count odds, the first-stop window,
        the most likely compound sequence and the win odds by stop count.

        moves=True (not in the reference): the race also runs through RaceSimulator.run_moves -- the same simulations --
        and the result gains 'moves', the block move_keys builds: per driver the expected places gained, the expected
        start gain and the passes made and lost, and for the race the expected on-track passes with their 10-90 % range
        and the commonest (a, b) pairs.

        pit_window=[(driver, loss in seconds or None: the config's pit_loss), ...], or {'windows': [...], 'edges': [...]}
        (not in the reference): the race also runs through RaceSimulator.run_pit_windows -- the same simulations,
        nothing re-simulated -- and the result gains 'pit_window', the block pit_window_keys builds: per window and lap
        the odds of a free stop, the rejoin position, the likeliest car ahead and the odds of clear air at rejoin.

        pace_uncertainty={'own': sigma or {driver: sigma}, 'team': sigma or {team: sigma}, 'edges': [...]} (not in the
        reference; seconds a lap, either of 'own' and 'team' may be left out): the race also runs through
        RaceSimulator.run_priors -- the same simulations as the forecast, and beside them the same simulations under a
        pace error drawn per driver (own) and per team of the race config's driver_teams (shared) -- and the result gains
        'pace_uncertainty', the block pace_uncertainty_keys builds: the odds under the draws beside the forecast's, and
        per driver the win odds and expected points by bin of its own drawn error.  There are no default sigmas, and
        prediction_point sets none: nobody has measured what an FP1 pace error is."""
        fixture = _open_fixture(fixture, season, race)
        inp = self.simulator_inputs(fixture, race, grid_penalties, circuit_info, prediction_point, actual_grid)
        sim = RaceSimulator(inp['config'], device=self.device)
        if pace_uncertainty:
            seed = sim._resolve_seed(seed)
            if self.device_front_end and not (actual_grid and prediction_point in ('quali', 'sprint')):
                raise ValueError('pace_uncertainty runs from the host grid matrix: device_front_end must be off')
            res = self.predict_weekend(season, race, fixture, grid_penalties, circuit_info, prediction_point, actual_grid,
                                       n_simulations, seed, matchups, trace, gaps, conditions, tyres, moves, pit_window)
            res['pace_uncertainty'] = self._pace_uncertainty(sim, inp, pace_uncertainty, n_simulations, seed,
                                                             grid_probs=inp['grid_probs'])
            return res
        if self.device_front_end and not (actual_grid and prediction_point in ('quali', 'sprint')):
            # same inputs, the matrix built on the device from the ratings (no host matrix crosses PCIe)
            ratings = {d: self.elo_system.ratings.get(d, {}).get('quali', self.elo_system.initial) for d in inp['drivers']}
            if matchups or trace or gaps or conditions or tyres or moves or pit_window:
                # the same matrix, read back from the device front end and handed to the matchups / trace / gaps run
                grid = sim.grid_probs_on_device(inp['drivers'], ratings, fixture.get('quali_features', {}),
                                                grid_penalties or {})
                return self._with_counts(sim, inp, grid, n_simulations, seed, prediction_point, actual_grid, matchups,
                                         trace, gaps, conditions, tyres, moves, pit_window)
            race_probs, grid = sim.run_from_ratings(
                n_simulations, inp['drivers'], ratings, fixture.get('quali_features', {}), grid_penalties or {},
                inp['base_pace'], inp['tire_deg'], inp['driver_variance'], inp['driver_dnf_rates'], seed=seed,
                track_condition=inp['track_condition'])
            return pack_result(inp['drivers'], grid, race_probs, inp['weather'], prediction_point, actual_grid)
        if matchups or trace or gaps or conditions or tyres or moves or pit_window:
            return self._with_counts(sim, inp, inp['grid_probs'], n_simulations, seed, prediction_point, actual_grid,
                                     matchups, trace, gaps, conditions, tyres, moves, pit_window)
        race_probs = sim.run_monte_carlo(
            n_simulations=n_simulations, grid_probs=inp['grid_probs'], base_pace=inp['base_pace'],
            tire_deg=inp['tire_deg'], driver_variance=inp['driver_variance'],
            driver_dnf_rates=inp['driver_dnf_rates'], seed=seed, track_condition=inp['track_condition'])
        return pack_result(inp['drivers'], inp['grid_probs'], race_probs, inp['weather'], prediction_point, actual_grid)

    def predict_from_state(self, season: int, race: str, fixture: dict | str, state, n_simulations: int = 100000,
                           seed: int | None = None, gaps=None, conditions=None, tyres: bool = False,
                           moves: bool = False, pit_window=None, pace_uncertainty=None):
        """In-race odds (not in the reference): the weekend's race inputs (simulator_inputs, as predict_weekend builds
        them) run from a mid-race RaceState of the fixture's drivers -- or from each of a list of them, with common
        random numbers -- through RaceSimulator.run_from_state.  Returns, per state, {'lap', 'win_probabilities', 'podium_probabilities',
        'points_probabilities' (top 10), 'full_distributions'}: one dict, or a list for a list of states.  gaps (as in
        predict_weekend): every state's dict gains 'gaps' from RaceSimulator.run_gaps on that state, same simulations.
        conditions (as in predict_weekend): every state's dict gains 'conditions' from RaceSimulator.run_conditions on
        that state, same simulations; race events count from the state's lap on.  tyres (as in predict_weekend): every
        state's dict gains 'tyres' from RaceSimulator.run_stints on that state, same simulations; stops count from the
        state's lap on.  moves (as in predict_weekend): every state's dict gains 'moves' from RaceSimulator.run_moves on
        that state, same simulations; passes count from the state's lap on and there is no start gain.  pit_window (as
        in predict_weekend): every state's dict gains 'pit_window' from RaceSimulator.run_pit_windows on that state, same
        simulations; the laps after the state's are recorded.  pace_uncertainty (as in predict_weekend): every state's
        dict gains 'pace_uncertainty' from RaceSimulator.run_priors on that state; the drawn errors apply to the laps after
        the state's."""
        fixture = _open_fixture(fixture, season, race)
        single = not isinstance(state, (list, tuple))
        states = [state] if single else list(state)
        inp = self.simulator_inputs(fixture, race)
        sim = RaceSimulator(inp['config'], device=self.device)
        seed = sim._resolve_seed(seed) if gaps or conditions or tyres or moves or pit_window or pace_uncertainty else seed
        # the driver order of predict_weekend's run: a state that run's simulation i reached continues as simulation i
        probs = sim.run_from_state(n_simulations, states, inp['base_pace'], inp['tire_deg'], inp['driver_variance'],
                                   inp['driver_dnf_rates'], seed=seed, track_condition=inp['track_condition'],
                                   drivers=list(inp['grid_probs']))
        drivers = sim.last_drivers
        out = []
        for st, rp in zip(states, probs):
            top = lambda k: {d: sum(rp.get(d, {}).get(p, 0) for p in range(1, k + 1)) for d in drivers}
            out.append({'lap': int(st.lap), 'win_probabilities': top(1), 'podium_probabilities': top(3),
                        'points_probabilities': top(10), 'full_distributions': rp})
        if gaps:
            for st, res in zip(states, out):
                g = sim.run_gaps(n_simulations, None, inp['base_pace'], inp['tire_deg'], inp['driver_variance'],
                                 inp['driver_dnf_rates'], state=st, seed=seed, track_condition=inp['track_condition'],
                                 drivers=list(inp['grid_probs']), **gap_options(gaps))
                res['gaps'] = gap_keys(g)
        if conditions:
            for st, res in zip(states, out):
                c = sim.run_conditions(n_simulations, conditions, None, inp['base_pace'], inp['tire_deg'],
                                       inp['driver_variance'], inp['driver_dnf_rates'], state=st, seed=seed,
                                       track_condition=inp['track_condition'], drivers=list(inp['grid_probs']))
                res['conditions'] = condition_keys(c)
        if tyres:
            for st, res in zip(states, out):
                t = sim.run_stints(n_simulations, None, inp['base_pace'], inp['tire_deg'], inp['driver_variance'],
                                   inp['driver_dnf_rates'], state=st, seed=seed, track_condition=inp['track_condition'],
                                   drivers=list(inp['grid_probs']))
                res['tyres'] = tyre_keys(t)
        if moves:
            for st, res in zip(states, out):
                mv = sim.run_moves(n_simulations, None, inp['base_pace'], inp['tire_deg'], inp['driver_variance'],
                                   inp['driver_dnf_rates'], state=st, seed=seed, track_condition=inp['track_condition'],
                                   drivers=list(inp['grid_probs']))
                res['moves'] = move_keys(mv)
        if pit_window:
            for st, res in zip(states, out):
                pw = sim.run_pit_windows(n_simulations, None, inp['base_pace'], inp['tire_deg'], inp['driver_variance'],
                                         inp['driver_dnf_rates'], state=st, seed=seed,
                                         track_condition=inp['track_condition'], drivers=list(inp['grid_probs']),
                                         **pit_window_options(pit_window, inp['config'].pit_loss))
                res['pit_window'] = pit_window_keys(pw, inp['config'].dirty_air_threshold)
        if pace_uncertainty:
            for st, res in zip(states, out):
                res['pace_uncertainty'] = self._pace_uncertainty(sim, inp, pace_uncertainty, n_simulations, seed, state=st)
        return out[0] if single else out

    @staticmethod
    def _pace_uncertainty(sim, inp, argument, n_simulations, seed, grid_probs=None, state=None) -> dict:
        """The 'pace_uncertainty' block: RaceSimulator.run_priors on the weekend's race inputs with the scenarios
        'forecast' (no prior) and 'uncertain' (the argument's priors), from the grid or from `state`."""
        drivers = list(inp['grid_probs'])
        priors, edges = pace_uncertainty_options(argument, drivers, inp['config'].driver_teams)
        r = sim.run_priors(n_simulations, {'forecast': [], 'uncertain': priors}, edges, None, inp['base_pace'],
                           inp['tire_deg'], inp['driver_variance'], inp['driver_dnf_rates'], grid_probs=grid_probs,
                           state=state, seed=seed, track_condition=inp['track_condition'], drivers=drivers)
        return pace_uncertainty_keys(r)

    def _scenario_run(self, season, race, fixture, state, seed, prediction_point, allow_single_compound):
        """What the seven scenario methods below share -> (simulator, the keyword arguments every run_* takes after its
        scenarios): the weekend's race inputs as predict_weekend builds them, drawn from the grid unless a mid-race
        `state` is given, in predict_weekend's driver order."""
        inp = self.simulator_inputs(_open_fixture(fixture, season, race), race, prediction_point=prediction_point)
        sim = RaceSimulator(inp['config'], device=self.device)
        return sim, dict(base_pace=inp['base_pace'], tire_deg=inp['tire_deg'], driver_variance=inp['driver_variance'],
                         driver_dnf_rates=inp['driver_dnf_rates'], grid_probs=inp['grid_probs'] if state is None else None,
                         state=state, seed=seed, track_condition=inp['track_condition'], drivers=list(inp['grid_probs']),
                         allow_single_compound=allow_single_compound)

    def predict_strategies(self, season: int, race: str, fixture: dict | str, strategies: dict, state=None,
                           n_simulations: int = 100000, seed: int | None = None, prediction_point: str = 'fp2',
                           allow_single_compound: bool = False):
        """Pit-strategy comparison (not in the reference): the weekend's race inputs (simulator_inputs, as
        predict_weekend builds them) run under each scenario of `strategies` ({name: [PitPlan, ...]}) through
        RaceSimulator.run_strategies -- from the grid, or from a mid-race RaceState -- with common random numbers.  The
        driver order is predict_weekend's, so an empty scenario reproduces predict_weekend's (or predict_from_state's)
        race for the same seed.  Returns the StrategyResult."""
        sim, common = self._scenario_run(season, race, fixture, state, seed, prediction_point, allow_single_compound)
        return sim.run_strategies(n_simulations, strategies, **common)

    def predict_penalties(self, season: int, race: str, fixture: dict | str, penalties: dict, strategies: dict | None = None,
                          state=None, n_simulations: int = 100000, seed: int | None = None,
                          prediction_point: str = 'fp2', allow_single_compound: bool = False):
        """Time penalties (not in the reference): predict_strategies' race run through RaceSimulator.run_penalties under
        each scenario of `penalties` ({name: [TimePenalty, ...]}) and `strategies` ({name: [PitPlan, ...]} or None).  A
        scenario without penalties or plans reproduces predict_weekend's (or predict_from_state's) race for the same
        seed.  Returns the PenaltyResult."""
        sim, common = self._scenario_run(season, race, fixture, state, seed, prediction_point, allow_single_compound)
        return sim.run_penalties(n_simulations, penalties, strategies, **common)

    def predict_events(self, season: int, race: str, fixture: dict | str, events: dict, strategies: dict | None = None,
                       state=None, n_simulations: int = 100000, seed: int | None = None,
                       prediction_point: str = 'fp2', allow_single_compound: bool = False):
        """Event scenarios (not in the reference): predict_strategies' race run through RaceSimulator.run_events under
        each scenario of `events` ({name: [RaceEvent, ...]}) and `strategies` ({name: [PitPlan, ...]} or None).  A
        scenario without overrides or plans reproduces predict_weekend's (or predict_from_state's) race for the same
        seed.  Returns the EventResult."""
        sim, common = self._scenario_run(season, race, fixture, state, seed, prediction_point, allow_single_compound)
        return sim.run_events(n_simulations, events, strategies, **common)

    def predict_paces(self, season: int, race: str, fixture: dict | str, paces: dict, strategies: dict | None = None,
                      state=None, n_simulations: int = 100000, seed: int | None = None,
                      prediction_point: str = 'fp2', allow_single_compound: bool = False):
        """Pace scenarios (not in the reference): predict_strategies' race run through RaceSimulator.run_paces under each
        scenario of `paces` ({name: [PaceOffset, ...]}) and `strategies` ({name: [PitPlan, ...]} or None).  A scenario
        without offsets or plans reproduces predict_weekend's (or predict_from_state's) race for the same seed.  Returns
        the PaceResult."""
        sim, common = self._scenario_run(season, race, fixture, state, seed, prediction_point, allow_single_compound)
        return sim.run_paces(n_simulations, paces, strategies, **common)

    def predict_weather(self, season: int, race: str, fixture: dict | str, changes: dict, strategies: dict | None = None,
                        model=None, state=None, n_simulations: int = 100000, seed: int | None = None,
                        prediction_point: str = 'fp2', allow_single_compound: bool = False):
        """Weather scenarios (not in the reference): predict_strategies' race run through RaceSimulator.run_weather under
        each scenario of `changes` ({name: [TrackChange, ...]}) and `strategies` ({name: [PitPlan, ...]} or None), with
        `model` (a WeatherModel, None: the project's default table).  Returns the WeatherResult."""
        sim, common = self._scenario_run(season, race, fixture, state, seed, prediction_point, allow_single_compound)
        return sim.run_weather(n_simulations, changes, strategies, model, **common)

    def predict_grids(self, season: int, race: str, fixture: dict | str, edits: dict, strategies: dict | None = None,
                      n_simulations: int = 100000, seed: int | None = None, prediction_point: str = 'fp2',
                      allow_single_compound: bool = False):
        """Grid scenarios (not in the reference, whose adjust_for_penalties smears a driver's grid distribution before
        the run): predict_strategies' race run through RaceSimulator.run_grids under each scenario of `edits` ({name:
        [GridEdit, ...]}) and `strategies` ({name: [PitPlan, ...]} or None), paired by simulation.  A scenario without
        edits or plans reproduces predict_weekend's race for the same seed.  Returns the GridResult."""
        sim, common = self._scenario_run(season, race, fixture, None, seed, prediction_point, allow_single_compound)
        return sim.run_grids(n_simulations, edits, strategies, **common)

    def predict_combined(self, season: int, race: str, fixture: dict | str, scenarios: dict, state=None,
                         n_simulations: int = 100000, seed: int | None = None, prediction_point: str = 'fp2',
                         allow_single_compound: bool = False):
        """Combined what-if scenarios (not in the reference): predict_strategies' race run through
        RaceSimulator.run_combined under each scenario of `scenarios` ({name: {'plans': [PitPlan, ...], 'penalties':
        [TimePenalty, ...], 'events': [RaceEvent, ...], 'paces': [PaceOffset, ...]}}).  An empty scenario reproduces
        predict_weekend's (or predict_from_state's) race for the same seed.  Returns the CombinedResult."""
        sim, common = self._scenario_run(season, race, fixture, state, seed, prediction_point, allow_single_compound)
        return sim.run_combined(n_simulations, scenarios, **common)

    @staticmethod
    def _with_counts(sim, inp, grid, n_simulations, seed, prediction_point, actual_grid, matchups, trace,
                     gaps=None, conditions=None, tyres=False, moves=False, pit_window=None) -> dict:
        """predict_weekend's result from run_matchups, run_trace, run_gaps, run_conditions, run_stints, run_moves and / or
        run_pit_windows calls on `grid` (the same simulations: one seed for all), with their keys added."""
        args = (n_simulations, grid, inp['base_pace'], inp['tire_deg'], inp['driver_variance'], inp['driver_dnf_rates'])
        seed = sim._resolve_seed(seed)
        res = None
        if matchups:
            m = sim.run_matchups(*args, seed=seed, track_condition=inp['track_condition'])
            res = pack_result(inp['drivers'], grid, m.position_probabilities, inp['weather'], prediction_point, actual_grid)
            res.update(matchup_keys(m, inp['config'].driver_teams))
        if trace:
            t = sim.run_trace(*args, seed=seed, track_condition=inp['track_condition'])
            if res is None:
                res = pack_result(inp['drivers'], grid, t.position_probabilities, inp['weather'], prediction_point,
                                  actual_grid)
            res.update(trace_keys(t))
        if gaps:
            g = sim.run_gaps(*args, seed=seed, track_condition=inp['track_condition'], **gap_options(gaps))
            if res is None:
                res = pack_result(inp['drivers'], grid, g.position_probabilities, inp['weather'], prediction_point,
                                  actual_grid)
            res['gaps'] = gap_keys(g)
        if conditions:
            c = sim.run_conditions(n_simulations, conditions, grid, inp['base_pace'], inp['tire_deg'],
                                   inp['driver_variance'], inp['driver_dnf_rates'], seed=seed,
                                   track_condition=inp['track_condition'])
            if res is None:
                res = pack_result(inp['drivers'], grid, c.position_probabilities(), inp['weather'], prediction_point,
                                  actual_grid)
            res['conditions'] = condition_keys(c)
        if tyres:
            t = sim.run_stints(*args, seed=seed, track_condition=inp['track_condition'])
            if res is None:
                res = pack_result(inp['drivers'], grid, t.position_probabilities(), inp['weather'], prediction_point,
                                  actual_grid)
            res['tyres'] = tyre_keys(t)
        if moves:
            mv = sim.run_moves(*args, seed=seed, track_condition=inp['track_condition'])
            if res is None:
                res = pack_result(inp['drivers'], grid, mv.position_probabilities(), inp['weather'], prediction_point,
                                  actual_grid)
            res['moves'] = move_keys(mv)
        if pit_window:
            pw = sim.run_pit_windows(*args, seed=seed, track_condition=inp['track_condition'],
                                     **pit_window_options(pit_window, inp['config'].pit_loss))
            if res is None:
                res = pack_result(inp['drivers'], grid, pw.position_probabilities(), inp['weather'], prediction_point,
                                  actual_grid)
            res['pit_window'] = pit_window_keys(pw, inp['config'].dirty_air_threshold)
        return res


MATCHUP_PODIUMS = 10         # ordered podiums listed by predict_weekend(matchups=True)


def matchup_keys(m, driver_teams) -> dict:
    """The keys predict_weekend(matchups=True) adds, JSON-safe, from a MatchupResult."""
    podiums = m.most_likely_podiums(MATCHUP_PODIUMS) if m.podium is not None else []
    return {
        'head_to_head': m.ahead_probabilities,
        'teammate_battles': m.teammate_battles(driver_teams),
        'likely_podiums': [{'podium': list(p), 'probability': q} for p, q in podiums],
    }


def trace_keys(t) -> dict:
    """The keys predict_weekend(trace=True) adds, JSON-safe, from a TraceResult: per driver, P(leading after each lap),
    expected laps led, the pit-stop distribution up to the largest count any simulation reached, P(fastest lap); and
    per race event P(at least one) and the expected number."""
    used = int(np.max(np.nonzero(t.stops.sum(axis=0))[0])) + 1 if t.stops.any() else 1
    return {
        'leader_by_lap': {d: [float(x) for x in p] for d, p in t.leader_probabilities.items()},
        'expected_laps_led': t.expected_laps_led,
        'pit_stop_distribution': {d: [float(x) for x in p[:used]] for d, p in t.pit_stop_distribution.items()},
        'expected_pit_stops': t.expected_pit_stops,
        'fastest_lap_probabilities': t.fastest_lap_probabilities,
        'race_event_probabilities': t.event_probabilities,
    }


def condition_keys(c) -> dict:
    """The 'conditions' block predict_weekend(conditions=...) / predict_from_state(conditions=...) add, JSON-safe, from a
    ConditionResult: {name: {'probability', 'standard_error', 'count', 'win': {driver: {'given', 'unconditional'}},
    'podium': the same}}; 'given' is None where no simulation met the condition."""
    return c.summary()


def tyre_keys(t) -> dict:
    """The 'tyres' block predict_weekend(tyres=True) / predict_from_state(tyres=True) add, JSON-safe, from a StintResult:
    {'first_lap', 'drivers': {driver: {'stops': [P(0), P(1), P(2), P(3), P(4 or more)], 'first_stop_window': [lap at the
    10 % quantile, lap at the 90 % quantile] among the simulations that stop or None, 'strategy': {'sequence',
    'probability'} the most likely compound sequence, 'win_by_stops': [P(win | s stops)] with None where no simulation
    makes s stops}}}."""
    stops = t.stop_count_probabilities()
    out = {}
    for d in t.drivers:
        window = t.stop_window(d)
        best = t.strategy_probabilities(d)[:1]
        out[d] = {
            'stops': stops[d],
            'first_stop_window': list(window) if window else None,
            'strategy': {'sequence': best[0][0], 'probability': best[0][1]} if best else None,
            'win_by_stops': [t.win_probability_given_stops(d, s) for s in range(t.stops_pos.shape[1])],
        }
    return {'first_lap': t.first_lap, 'drivers': out}


def move_keys(mv, pairs=5) -> dict:
    """The 'moves' block predict_weekend(moves=True) / predict_from_state(moves=True) add, JSON-safe, from a MoveResult:
    {'first_lap', 'drivers': {driver: {'places_gained' E[grid slot - classified position], 'start_gain' E[slot -
    position after lap 1 | running] or None (None from a state), 'passes': {kind name: expected per race}}},
    'race_passes': {'expected', 'p10', 'p90'} on track, 'pairs': [{'a', 'b', 'per_race'}] the commonest (a, b) with a
    taking a place from b on track}.  A pass is the model's order change between two lap ends."""
    gained, passes = mv.expected_positions_gained(), mv.expected_passes()
    start = mv.expected_start_gain() if mv.from_grid else {}
    return {'first_lap': mv.first_lap,
            'drivers': {d: {'places_gained': gained[d], 'start_gain': start.get(d), 'passes': passes[d]} for d in mv.drivers},
            'race_passes': {'expected': mv.expected_race_passes(), 'p10': mv.race_passes_quantile(0.1),
                            'p90': mv.race_passes_quantile(0.9)},
            'pairs': [{'a': a, 'b': b, 'per_race': x} for a, b, x in mv.most_frequent_passes(pairs)]}


def gap_options(gaps) -> dict:
    """run_gaps's edges / pairs from predict_weekend's gaps argument: True, or {'edges': [...], 'pairs': [(a, b), ...]}."""
    if gaps is True:
        return {}
    unknown = set(gaps) - {'edges', 'pairs'}
    if unknown:
        raise ValueError(f'gaps: unknown keys {sorted(unknown)} (edges, pairs)')
    out = {}
    if gaps.get('edges') is not None:
        out['edges'] = [float(x) for x in gaps['edges']]
    if gaps.get('pairs'):
        out['pairs'] = [(str(a), str(b)) for a, b in gaps['pairs']]
    return out


def pit_window_options(pit_window, pit_loss) -> dict:
    """run_pit_windows's windows / edges from predict_weekend's pit_window argument: [(driver, loss or None), ...], or
    {'windows': [...], 'edges': [...]}.  None stands for `pit_loss`; a window given twice is kept once."""
    if not isinstance(pit_window, dict):
        pit_window = {'windows': pit_window}
    unknown = set(pit_window) - {'windows', 'edges'}
    if unknown:
        raise ValueError(f'pit_window: unknown keys {sorted(unknown)} (windows, edges)')
    windows = []
    for d, loss in pit_window.get('windows') or ():
        w = (str(d), float(pit_loss if loss is None else loss))
        if w not in windows:
            windows.append(w)
    out = {'windows': windows}
    if pit_window.get('edges') is not None:
        out['edges'] = [float(x) for x in pit_window['edges']]
    return out


def pit_window_keys(pw, clear_air_seconds=2.0) -> dict:
    """The 'pit_window' block predict_weekend(pit_window=...) / predict_from_state(pit_window=...) add, JSON-safe, from a
    PitWindowResult: the edges, the first recorded lap, the edge nearest to `clear_air_seconds` (the model's
    dirty_air_threshold; the counts answer at edges only) and per window, by lap (index lap - 1; None where the lap is
    not recorded or the driver never runs), all given that the driver is running: 'free_stop' P(no place lost),
    'expected_rejoin_position' and 'median_rejoin_position' (1-based), 'clear_air' P(car ahead at least that edge up
    the road, or none), 'safe_from_behind' likewise for the car behind, 'likeliest_ahead' [driver or 'in the lead',
    probability]; and 'running' P(running), 'open_laps' the laps with P(free stop) >= 0.5."""
    edge = min(pw.edges, key=lambda x: (abs(x - clear_air_seconds), x))           # (as cli._nearest_edges picks)
    laps = range(1, pw.total_laps + 1)
    recorded = lambda lap: lap >= pw.first_lap
    safe = lambda xs: [None if x is None or x != x else float(x) for x in xs]
    rows = []
    for w, (d, loss) in enumerate(pw.windows):
        ahead = [(pw.rejoins_behind(w, lap, 1) or [None])[0] if recorded(lap) else None for lap in laps]
        rows.append({
            'driver': d, 'loss': loss, 'running': safe(pw.running_probability(w)),
            'free_stop': safe(pw.free_stop_probability(w)),
            'expected_rejoin_position': safe(pw.expected_rejoin_position(w)),
            'median_rejoin_position': [pw.median_rejoin_position(w, lap) if recorded(lap) else None for lap in laps],
            'clear_air': safe(pw.clear_air_probability(w, edge)),
            'safe_from_behind': safe(pw.safe_from_behind_probability(w, edge)),
            'likeliest_ahead': [None if a is None else [a[0], a[1]] for a in ahead],
            'open_laps': pw.open_laps(w)})
    return {'edges': list(pw.edges), 'first_lap': pw.first_lap, 'total_laps': pw.total_laps, 'clear_air_seconds': edge,
            'windows': rows}


DEFAULT_PACE_EDGES = (-0.3, -0.1, 0.0, 0.1, 0.3)      # seconds a lap: the by-draw table's bins when none are given


def pace_uncertainty_options(argument, drivers, driver_teams):
    """run_priors' priors and edges from predict_weekend's pace_uncertainty argument {'own': sigma or {driver: sigma},
    'team': sigma or {team: sigma}, 'edges': [...]}: one own prior per driver that has a sigma, one group per team of
    `driver_teams` that has a sigma and a driver in the race."""
    from .simulation import PacePrior
    if not isinstance(argument, dict) or set(argument) - {'own', 'team', 'edges'}:
        raise ValueError("pace_uncertainty: a dict with any of the keys 'own', 'team', 'edges'")
    own, team = argument.get('own'), argument.get('team')
    if own is None and team is None:
        raise ValueError("pace_uncertainty: give 'own', 'team' or both (there are no default sigmas)")
    priors = []
    if own is not None:
        if isinstance(own, dict):
            unknown = [d for d in own if d not in drivers]
            if unknown:
                raise ValueError(f'pace_uncertainty: own: {unknown} not among the drivers')
        priors += [PacePrior.driver(d, own[d] if isinstance(own, dict) else own) for d in drivers
                   if not isinstance(own, dict) or d in own]
    if team is not None:
        members = {}
        for d in drivers:
            members.setdefault(driver_teams.get(d, 'Unknown'), []).append(d)
        if isinstance(team, dict):
            unknown = [t for t in team if t not in members]
            if unknown:
                raise ValueError(f'pace_uncertainty: team: {unknown} not among the teams {sorted(members)}')
        priors += [PacePrior.group(ds, team[t] if isinstance(team, dict) else team) for t, ds in members.items()
                   if not isinstance(team, dict) or t in team]
    edges = argument.get('edges')
    return priors, list(DEFAULT_PACE_EDGES if edges is None else edges)


def pace_uncertainty_keys(r) -> dict:
    """The 'pace_uncertainty' block, JSON-safe, from a PriorResult with the scenarios 'forecast' and 'uncertain': the
    edges and each bin's bounds (None: open), per driver the win, podium and points odds and the expected points under
    both, the paired comparison, and by bin of the driver's own drawn error the share of simulations, the win odds and
    the expected points (None for an empty bin)."""
    num = lambda x: None if x is None or x != x or x in (float('inf'), float('-inf')) else float(x)
    B = len(r.edges) + 1
    out = {'n_simulations': int(r.n_simulations), 'edges': [float(e) for e in r.edges],
           'bins': [[num(v) for v in r.bin_bounds(b)] for b in range(B)], 'drivers': {}}
    points = {s: r.expected_points(s) for s in r.names}
    for d in r.drivers:
        i = r.drivers.index(d)
        odds = lambda s: {'win': float(r._p(s)[i, 0]), 'podium': float(r._p(s)[i, :3].sum()),
                          'points': float(r._p(s)[i, :10].sum()), 'expected_points': points[s][d]}
        c = r.compare('uncertain', d)
        out['drivers'][d] = {
            'forecast': odds('forecast'), 'uncertain': odds('uncertain'),
            'paired': {k: c[k] for k in ('p_better', 'p_same', 'p_worse', 'mean_gain', 'se')},
            'by_draw': {'share': [float(v) for v in r.draw_probabilities('uncertain', d)],
                        'win': [num(v) for v in r.win_probability_by_draw('uncertain', d)],
                        'expected_points': [num(v) for v in r.expected_points_by_draw('uncertain', d)]}}
    return out


def gap_keys(g) -> dict:
    """The 'gaps' block predict_weekend(gaps=...) / predict_from_state(gaps=...) add, JSON-safe, from a GapResult: the
    edges; the winning-margin distribution ([B + 1]: the bins, then P(fewer than two finish)); per driver the
    finishing-gap distribution ([B + 1]: the bins, then P(retired)) and P(within each edge of the leader at the flag);
    per pair P(a ahead), P(b ahead), P(either out) at the flag and P(|gap| < edge) by lap for every edge."""
    fl = lambda a: [float(x) for x in a]
    return {
        'edges': list(g.edges),
        'first_lap': g.first_lap,
        'winning_margin': fl(g.winning_margin_distribution),
        'finishing_gap': {d: fl(g.gap_distribution(d)) for d in g.drivers},
        'within_at_flag': {d: {str(e): g.within(d, e) for e in g.edges} for d in g.drivers},
        'pairs': [dict(a=a, b=b, **g.pair_summary(a, b),
                       within_by_lap={str(e): fl(g.pair_within_by_lap(a, b, e)) for e in g.edges})
                  for a, b in g.pairs],
    }


def pack_result(drivers, quali_probs, race_probs, weather, prediction_point, actual_grid) -> dict:
    """The result dict of predict_weekend (:302-319)."""
    n = max(1, len(drivers))
    return {
        'pole_probabilities': {d: quali_probs[d][0] if quali_probs.get(d) else 1.0 / n for d in drivers},
        'win_probabilities': {d: race_probs.get(d, {}).get(1, 0) for d in drivers},
        'podium_probabilities': {d: sum(race_probs.get(d, {}).get(p, 0) for p in (1, 2, 3)) for d in drivers},
        'full_distributions': race_probs,
        'weather': weather,
        'prediction_point': prediction_point,
        'confidence': CONFIDENCE.get(prediction_point, 'moderate'),
        'grid_is_actual': actual_grid is not None and prediction_point in ('quali', 'sprint'),
    }
