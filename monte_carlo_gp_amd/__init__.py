"""MI355X-native Monte Carlo race-simulation engine (hot path of dan-lee-gh/monte-carlo-gp).

Public surface mirrors reference src/simulation.py: CarState, RaceConfig, RaceSimulator; run_monte_carlo_batch runs several
races in one launch; RaceSimulator.run_matchups counts head-to-heads and podiums of one race (MatchupResult);
run_championship simulates the drivers' and constructors' standings over a calendar of races;
RaceSimulator.run_from_state simulates the rest of a race from a mid-race RaceState; RaceSimulator.run_trace counts what
happened lap by lap (TraceResult: lap chart, laps led, pit stops, fastest lap, race events);
RaceSimulator.run_strategies compares pit strategies (PitPlan, pit_window, StrategyResult); RaceSimulator.run_gaps counts
the race's time gaps (GapResult: gap to the leader by lap, winning margin, gaps between named drivers);
RaceSimulator.run_pit_windows counts where a car would rejoin if it stopped at the end of a lap (PitWindowResult: rejoin position,
places lost, car ahead and gaps by lap, nothing re-simulated; the command is python -m monte_carlo_gp_amd.pit_window);
RaceSimulator.run_penalties adds time penalties to the scenarios (TimePenalty, PenaltyResult: served in the pits or at the flag);
RaceSimulator.run_events sets the race's events on chosen laps (RaceEvent, EventResult: a safety car on lap 31, a green rest of the race);
RaceSimulator.run_paces adds lap-time offsets to the scenarios (PaceOffset, PaceResult: damage until the next stop, an engine mode for ten laps);
RaceSimulator.run_combined holds plans, penalties, events and offsets in one scenario (CombinedResult: a safety car on lap 31, a penalty served under it);
RaceSimulator.run_weather changes the track condition by lap (TrackChange, WeatherModel, WeatherResult: rain from lap 30, who gains by boxing at once);
RaceSimulator.run_grids edits the starting grid (GridEdit, GridResult: a ten-place drop, a pit-lane start, a front row fixed by qualifying);
RaceSimulator.run_priors draws a pace error per driver and simulation (PacePrior, PriorResult: how sure are these odds when the pace figures are FP1 estimates; what a tenth is worth);
RaceSimulator.run_stints counts the model's tyre stints (StintResult: stop laps, compound sequences, odds by stop count);
RaceSimulator.run_moves counts how the field moves (MoveResult: grid-to-finish odds, start gains, passes by driver, lap and pair);
RaceSimulator.run_conditions counts combinations and conditional odds (conditions.parse, Condition, ConditionResult).
The compute path is the HIP library libmcgp_hip.so (C ABI: include/mcgp.h); there is no
CPU fallback.
"""
from .simulation import (DEFAULT_GAP_EDGES, CarState, ChampionshipResult, CombinedResult, EventResult, GapResult, GridEdit, GridResult, MatchupResult,  # noqa: F401
                         MoveResult, PaceOffset, PacePrior, PaceResult, PenaltyResult, PitPlan, PitWindowResult, PriorResult, RaceConfig, RaceEvent, RaceSimulator, RaceState, StintResult, StrategyResult,
                         TimePenalty, TraceResult, TrackChange, WeatherModel, WeatherResult,
                         decode_stints, encode_stints, histogram_to_probs, pit_window, run_championship,
                         run_monte_carlo_batch)
from .conditions import Condition, ConditionResult  # noqa: F401
from . import conditions, config  # noqa: F401

__all__ = ['DEFAULT_GAP_EDGES', 'CarState', 'ChampionshipResult', 'CombinedResult', 'Condition', 'ConditionResult', 'EventResult', 'GapResult', 'GridEdit', 'GridResult', 'MatchupResult', 'MoveResult', 'PaceOffset', 'PacePrior', 'PaceResult', 'PenaltyResult', 'PitPlan', 'PitWindowResult', 'PriorResult', 'RaceConfig', 'RaceEvent',
           'RaceSimulator', 'RaceState', 'StintResult', 'StrategyResult', 'TimePenalty', 'TraceResult', 'TrackChange', 'WeatherModel', 'WeatherResult', 'decode_stints', 'encode_stints',
           'histogram_to_probs', 'pit_window',
           'run_championship', 'run_monte_carlo_batch', 'conditions', 'config']
