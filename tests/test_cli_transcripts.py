"""The command line against its recorded transcripts (tests/golden/cli/, recorded by cli_cases.record from the commit before
the commands were folded into one driver): for every case the exit status, stdout, stderr and the --json document are
equal to the record, and every subcommand's arguments are the recorded ones, option by option.  No device needed: the
predictor is cli_cases.StandInPredictor."""
import json
import os

import pytest

import cli_cases
from monte_carlo_gp_amd import cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cli')


def _golden(command):
    with open(cli_cases.golden_path(GOLDEN, command)) as f:
        return json.load(f)


@pytest.mark.parametrize('command', list(cli_cases.CASES))
def test_transcripts(command, tmp_path):
    golden = _golden(command)
    assert list(golden) == list(cli_cases.CASES[command])
    for name, argv in cli_cases.CASES[command].items():
        got = cli_cases.run_case(cli, command, argv, str(tmp_path))
        for key in ('status', 'stderr', 'stdout', 'json'):
            assert got[key] == golden[name][key], (command, name, key)


def test_every_what_if_command_has_every_kind_of_case():
    for command in ('strategy', 'penalty', 'events', 'pace', 'weather', 'grid', 'what-if'):
        golden = _golden(command)
        statuses = {name: rec['status'] for name, rec in golden.items()}
        assert statuses['full'] == 0 and golden['full']['json'] is not None
        assert statuses['not offline'] == statuses['nothing given'] == statuses['refused by the library'] == 2
        assert golden['refused by the library']['stderr'] == 'error: the library refused these scenarios\n'
        assert 'state' in golden or command == 'grid'
    for command in ('pace', 'what-if'):
        assert 'offset carried' in _golden(command)['full']['stdout']
    assert 'penalty served at a stop' in _golden('what-if')['full']['stdout']


def test_parser_shape():
    """Every subcommand's options, in the order --help lists them: flag strings, dest, type, default, nargs, required,
    choices, metavar, help text and action class."""
    golden, got = _golden('parser'), json.loads(json.dumps(cli_cases.parser_shape(cli)))
    assert list(got) == list(golden)
    for command in golden:
        assert got[command] == golden[command], command
    assert '--state' not in [s for a in got['grid'] for s in a['option_strings']]
