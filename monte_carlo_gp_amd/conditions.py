"""Conditions for RaceSimulator.run_conditions (include/mcgp.h: mcgp_run_conditions): the text form, its parser and the
result.  A condition is a conjunction of up to 8 atoms; an atom compares one integer fact of a finished simulation with a
range.  The device evaluates them inside every simulation; nothing here simulates or counts.

Grammar (one condition per string):

    condition := atom ('&' atom)*
    atom      := ['!'] subject op value | ['!'] subject 'in' LO '..' HI | ['!'] shorthand
    subject   := D.pos | D.grid | D.out | D.gain | D.ahead_of.E | finishers | red | sc | vsc
    op        := = | != | < | <= | > | >=
    shorthand := D.wins | D.podium | D.points | D.pole | D.dnf | D.finishes | D.beats.E

D, E are driver names.  D.pos: classified position (1..n); D.grid: grid slot (1..n); D.out: the lap of retirement, 0 when
running at the flag; D.gain: grid slot - position; D.ahead_of.E: E's position - D's (> 0: D ahead); finishers: cars
running at the flag; red / sc / vsc: laps with a red flag / safety car / virtual safety car.  D.points is pos <= 10."""
from __future__ import annotations

import ctypes as C
import math
import re
from dataclasses import dataclass

import numpy as np

from . import _native as N

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
VALUE_LIMIT = 10 ** 9                 # |value| a text may state: leaves room for the +-1 of < and >

_DRIVER_FACTS = {'pos': N.FACT_POSITION, 'grid': N.FACT_GRID, 'out': N.FACT_RETIRED_LAP, 'gain': N.FACT_GAINED}
_RACE_FACTS = {'finishers': N.FACT_FINISHERS, 'red': N.FACT_RED_FLAGS, 'sc': N.FACT_SAFETY_CARS, 'vsc': N.FACT_VSCS}
# shorthand -> (fact, lo, hi)
_SHORTHANDS = {'wins': (N.FACT_POSITION, 1, 1), 'podium': (N.FACT_POSITION, 1, 3), 'points': (N.FACT_POSITION, 1, 10),
               'pole': (N.FACT_GRID, 1, 1), 'dnf': (N.FACT_RETIRED_LAP, 1, INT_MAX), 'finishes': (N.FACT_RETIRED_LAP, 0, 0)}
_COMPARISON = re.compile(r'^(?P<subject>[^\s=<>!]+)\s*(?P<op><=|>=|!=|=|<|>)\s*(?P<value>.*)$')
_RANGE = re.compile(r'^(?P<subject>\S+)\s+in\s+(?P<lo>\S+?)\s*\.\.\s*(?P<hi>\S+)$')


@dataclass(frozen=True)
class Atom:
    fact: int
    a: int = 0
    b: int = 0
    lo: int = INT_MIN
    hi: int = INT_MAX
    negate: bool = False


@dataclass(frozen=True)
class Condition:
    """A parsed condition: its atoms (driver indices in the order of the `drivers` it was parsed against) and text."""
    atoms: tuple
    text: str = ''

    def c_struct(self) -> 'N.McgpCondition':
        c = N.McgpCondition()
        c.n_atoms = len(self.atoms)
        for k, at in enumerate(self.atoms):
            c.atom[k] = N.McgpConditionAtom(at.fact, at.a, at.b, at.lo, at.hi, int(at.negate))
        return c


def _fail(text, token, why):
    raise ValueError(f'condition {text!r}: {token!r}: {why}')


def _int(text, token):
    if not re.fullmatch(r'[+-]?\d+', token):
        _fail(text, token, 'not an integer')
    v = int(token)
    if abs(v) > VALUE_LIMIT:
        _fail(text, token, f'beyond +-{VALUE_LIMIT}')
    return v


def _driver(text, name, index):
    if name not in index:
        _fail(text, name, 'not among the drivers')
    return index[name]


def _subject(text, subject, index):
    """(fact, a, b) of a comparable subject."""
    if subject in _RACE_FACTS:
        return _RACE_FACTS[subject], 0, 0
    parts = subject.split('.')
    if len(parts) == 2 and parts[1] in _DRIVER_FACTS:
        return _DRIVER_FACTS[parts[1]], _driver(text, parts[0], index), 0
    if len(parts) == 3 and parts[1] == 'ahead_of':
        a, b = _driver(text, parts[0], index), _driver(text, parts[2], index)
        if a == b:
            _fail(text, subject, 'needs two different drivers')
        return N.FACT_AHEAD_BY, a, b
    if len(parts) == 2 and parts[1] in _SHORTHANDS or len(parts) == 3 and parts[1] == 'beats':
        _fail(text, subject, 'is a yes/no shorthand and takes no comparison')
    _fail(text, subject, 'unknown subject (D.pos, D.grid, D.out, D.gain, D.ahead_of.E, finishers, red, sc, vsc)')


def _atom(text, token, index):
    body = token.strip()
    negate = body.startswith('!') and not body.startswith('!=')
    if negate:
        body = body[1:].strip()
    if not body:
        _fail(text, token, 'empty atom')
    m = _RANGE.match(body)
    if m:
        fact, a, b = _subject(text, m['subject'], index)
        lo, hi = _int(text, m['lo']), _int(text, m['hi'])
        if lo > hi:
            _fail(text, body, 'the range is empty (LO above HI)')
        return Atom(fact, a, b, lo, hi, negate)
    m = _COMPARISON.match(body)
    if m:
        fact, a, b = _subject(text, m['subject'], index)
        v = _int(text, m['value'].strip())
        op = m['op']
        lo, hi = {'=': (v, v), '!=': (v, v), '<': (INT_MIN, v - 1), '<=': (INT_MIN, v), '>': (v + 1, INT_MAX),
                  '>=': (v, INT_MAX)}[op]
        return Atom(fact, a, b, lo, hi, negate != (op == '!='))
    if re.search(r'\s', body):
        _fail(text, body, 'expected SUBJECT OP VALUE, SUBJECT in LO..HI or a shorthand')
    parts = body.split('.')
    if len(parts) == 2 and parts[1] in _SHORTHANDS:
        fact, lo, hi = _SHORTHANDS[parts[1]]
        return Atom(fact, _driver(text, parts[0], index), 0, lo, hi, negate)
    if len(parts) == 3 and parts[1] == 'beats':
        a, b = _driver(text, parts[0], index), _driver(text, parts[2], index)
        if a == b:
            _fail(text, body, 'needs two different drivers')
        return Atom(N.FACT_AHEAD_BY, a, b, 1, INT_MAX, negate)
    if body in _RACE_FACTS or len(parts) == 2 and parts[1] in _DRIVER_FACTS or len(parts) == 3 and parts[1] == 'ahead_of':
        _fail(text, body, 'needs a comparison (=, !=, <, <=, >, >=, in LO..HI)')
    _fail(text, body, 'unknown shorthand (D.wins, D.podium, D.points, D.pole, D.dnf, D.finishes, D.beats.E)')


def parse(text: str, drivers) -> Condition:
    """One condition string -> Condition against `drivers` (names in driver-index order).  ValueError names the text and
    the offending token; an unknown driver is an error."""
    if isinstance(text, Condition):
        return text
    if not isinstance(text, str):
        raise ValueError(f'a condition is a string or a Condition, got {type(text).__name__}')
    index = {str(d): i for i, d in enumerate(drivers)}
    if not text.strip():
        raise ValueError(f'condition {text!r}: empty (every simulation meets it: give Condition(()) if that is meant)')
    atoms = tuple(_atom(text, tok, index) for tok in text.split('&'))
    if len(atoms) > N.MAX_CONDITION_ATOMS:
        raise ValueError(f'condition {text!r}: {len(atoms)} atoms, at most {N.MAX_CONDITION_ATOMS}')
    return Condition(atoms, text.strip())


def parse_all(conditions, drivers) -> dict:
    """{name: string | Condition} -> {name: Condition}, 1 to 64 of them."""
    if not isinstance(conditions, dict):
        raise ValueError('conditions: a dict name -> condition string (or Condition)')
    if not 1 <= len(conditions) <= N.MAX_CONDITIONS:
        raise ValueError(f'conditions: 1 to {N.MAX_CONDITIONS}, got {len(conditions)}')
    out = {}
    for name, c in conditions.items():
        c = parse(c, drivers)
        if len(c.atoms) > N.MAX_CONDITION_ATOMS:
            raise ValueError(f'condition {name!r}: {len(c.atoms)} atoms, at most {N.MAX_CONDITION_ATOMS}')
        out[str(name)] = c
    return out


def c_array(parsed):
    """The mcgp_condition array of parse_all's result, in its order."""
    return (N.McgpCondition * len(parsed))(*[c.c_struct() for c in parsed.values()])


@dataclass
class ConditionResult:
    """Counts of RaceSimulator.run_conditions.  hist [n][n]: every simulation's [driver][position - 1]; counts {name: the
    simulations that met the condition}; cond_hist [C][n][n]: the position histogram among those, in the order of names,
    or None when the run did not collect them (then only probabilities and counts are available)."""
    drivers: list
    names: list
    n_simulations: int
    hist: np.ndarray
    counts: dict
    cond_hist: 'np.ndarray | None'

    def _count(self, name):
        if name not in self.counts:
            raise KeyError(f'no condition named {name!r}; have {self.names}')
        return int(self.counts[name])

    def probability(self, name) -> float:
        """P(condition)."""
        c = self._count(name)
        return c / self.n_simulations if self.n_simulations else 0.0

    def standard_error(self, name) -> float:
        """Binomial standard error of probability(name)."""
        if not self.n_simulations:
            return 0.0
        p = self.probability(name)
        return math.sqrt(p * (1.0 - p) / self.n_simulations)

    def _given(self, name):
        c = self._count(name)
        if self.cond_hist is None:
            raise ValueError(f'condition {name!r}: the conditional histograms were not collected (histograms=False)')
        if c == 0:
            raise ValueError(f'condition {name!r} was met in none of {self.n_simulations} simulations: no conditional odds')
        return self.cond_hist[self.names.index(name)], c

    def position_probabilities(self, name=None) -> dict:
        """{driver: {position: probability}} given the condition; None: the unconditional result."""
        from .simulation import histogram_to_probs
        if name is None:
            return histogram_to_probs(self.hist, self.drivers, self.n_simulations) if self.n_simulations else \
                {d: {} for d in self.drivers}
        h, c = self._given(name)
        return histogram_to_probs(h, self.drivers, c)

    def _driver(self, driver):
        if driver not in self.drivers:
            raise KeyError(f'no driver {driver!r}')
        return self.drivers.index(driver)

    def win_probability(self, name, driver) -> float:
        """P(driver wins | condition); name None: unconditional."""
        d = self._driver(driver)
        if name is None:
            return int(self.hist[d, 0]) / self.n_simulations if self.n_simulations else 0.0
        h, c = self._given(name)
        return int(h[d, 0]) / c

    def podium_probability(self, name, driver) -> float:
        """P(driver in the first three | condition); name None: unconditional."""
        d = self._driver(driver)
        if name is None:
            return int(self.hist[d, :3].sum()) / self.n_simulations if self.n_simulations else 0.0
        h, c = self._given(name)
        return int(h[d, :3].sum()) / c

    def summary(self) -> dict:
        """{name: probability, standard_error, count, and per driver the win / podium odds given the condition beside the
        unconditional ones (None where the condition was never met or no histograms were collected)}."""
        out = {}
        for name in self.names:
            met = self._count(name) > 0 and self.cond_hist is not None
            out[name] = {
                'probability': self.probability(name), 'standard_error': self.standard_error(name),
                'count': self._count(name),
                'win': {d: {'given': self.win_probability(name, d) if met else None,
                            'unconditional': self.win_probability(None, d)} for d in self.drivers},
                'podium': {d: {'given': self.podium_probability(name, d) if met else None,
                               'unconditional': self.podium_probability(None, d)} for d in self.drivers},
            }
        return out
