"""The launch ladder of the pitch tracker's Viterbi stage (shennong_amd/csrc/pitch_route.h), on the CPU.

tests/tools/pitch_route_dump.cpp is compiled against pitch_route.h alone - host code, no device and no library - and
prints, for every combination of state count, batch size and the two knobs below, which of the three Viterbi forms
runs, with how many waves, which register-slice count the by-state form takes, the dynamic LDS and whether the route
refuses.  Every line is compared with the ladder and the LDS formulas as THIS file states them (from the launcher the
header replaced), not with a recording of the program's output."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'shennong_amd', 'csrc')

STATES = (1, 127, 128, 129, 417, 448, 449, 461, 512, 513, 521, 1400, 1600)
UTTS = (1, 768, 769, 1280, 1281, 100000)
TEAM_KNOBS = (None, '1', '2', '3', '4')
FLAT_KNOBS = (None, '0', '1')

BY_STATE, TEAM, FLAT = 0, 1, 2
FWD_PAD, QUEUE_FLOATS, WAVES = 36, 128 * 4, 8
LDS_LIMIT = 160 * 1024


def _compiler():
    for candidate in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


def _atoi(text):
    """C's atoi on the strings the knobs see: leading digits, 0 if there are none"""
    digits = ''.join(itertools.takewhile(str.isdigit, text))
    return int(digits) if digits else 0


def _knobs(team, flat):
    """(forced team size or 0, flat form allowed)"""
    return (_atoi(team) if team is not None else 0), not (flat is not None and flat[:1] == '0')


def _state_lds(s4):
    return 4 * (s4 + WAVES * (3 * s4 + FWD_PAD + QUEUE_FLOATS))


def _route(S, n_utts, team_knob, flat_knob):
    """(form, waves, nk, lds bytes, refused): the ladder, from the state count and the batch size"""
    forced, flat_allowed = _knobs(team_knob, flat_knob)
    s4 = (S + 3) & ~3
    team = forced if forced in (1, 2, 4) else 4 if n_utts <= 768 else 2 if n_utts <= 1280 else 1
    if S > 512 or S < 128:
        team = 1
    if team > 1:
        return TEAM, team, -1, 4 * (4 * s4 + FWD_PAD + team * (QUEUE_FLOATS + 1)), False
    if 128 < S <= 448 and flat_allowed:
        wave_bytes = (448 + 32) * 8 + (448 + FWD_PAD) * 4 + 448 * 4
        return FLAT, WAVES, -1, ((s4 * 4 + 15) & ~15) + WAVES * wave_bytes, False
    lds = _state_lds(s4)
    return BY_STATE, WAVES, 7 if S <= 448 else 8 if S <= 512 else 0, lds, lds > LDS_LIMIT


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    hipcc = _compiler()
    if hipcc is None:
        pytest.skip('no hipcc to compile tests/tools/pitch_route_dump.cpp with')
    tmp = tmp_path_factory.mktemp('pitch_route')
    program = str(tmp / 'pitch_route_dump')
    subprocess.run([hipcc, '-O1', '-std=c++17', '-Wall', '-I', CSRC, '-o', program,
                    os.path.join(ROOT, 'tests', 'tools', 'pitch_route_dump.cpp')], check=True, cwd=str(tmp))
    lines = subprocess.run([program], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
    fields = [dict(item.split('=', 1) for item in line.split()[1:] if '=' in item) for line in lines]
    return [(line.split()[0], f) for line, f in zip(lines, fields)]


def test_route_is_the_ladder(dump):
    got = [f for kind, f in dump if kind == 'route']
    cases = list(itertools.product(STATES, UTTS, TEAM_KNOBS, FLAT_KNOBS))
    assert len(got) == len(cases)
    seen = set()
    for f, (S, n, team, flat) in zip(got, cases):
        assert (int(f['S']), int(f['n']), f['team'], f['flat']) == (S, n, team or '-', flat or '-')
        want = _route(S, n, team, flat)
        have = (int(f['form']), int(f['waves']), int(f['nk']), int(f['lds']), f['refusal'] == '1')
        assert have == want, 'S=%d n=%d team=%s flat=%s' % (S, n, team, flat)
        form, waves, nk, lds, refused = have
        seen.add((form, waves, nk))
        # only the by-state form refuses, and nothing that runs asks for more LDS than a workgroup can have
        assert not refused or form == BY_STATE
        assert refused or lds <= LDS_LIMIT
        assert refused == (S == 1600)
    # every form, both team sizes and every register-slice count of the by-state form
    assert seen == {(TEAM, 2, -1), (TEAM, 4, -1), (FLAT, WAVES, -1), (BY_STATE, WAVES, 7), (BY_STATE, WAVES, 8),
                    (BY_STATE, WAVES, 0)}


def test_route_refusal_threshold(dump):
    """100 S4 + 17 536 bytes against 160 KB: 1 460 states are the last that fit, 1 461 (S4 = 1 464) the first refused"""
    limit = [f for kind, f in dump if kind == 'limit']
    assert len(limit) == 1
    first = next(S for S in range(513, 4000) if _state_lds((S + 3) & ~3) > LDS_LIMIT)
    assert first == 1461
    assert _state_lds((first - 1 + 3) & ~3) <= LDS_LIMIT < _state_lds((first + 3) & ~3)
    assert int(limit[0]['state']) == first
    assert int(limit[0]['last_lds']) == _state_lds((first - 1 + 3) & ~3)
    assert int(limit[0]['first_lds']) == _state_lds((first + 3) & ~3)


def test_knob_parser(dump):
    """only 1, 2 and 4 force a team (the route drops the rest), only a first character '0' turns the flat form off"""
    got = {(f['in_team'], f['in_flat']): (int(f['team']), int(f['flat']), int(f['trace'])) for kind, f in dump
           if kind == 'knobs'}
    assert got == {('3', '0x'): (3, 0, 2), ('', '1'): (0, 1, 2), ('0', ''): (0, 1, 2), ('4', '0'): (4, 0, 2),
                   ('2', '00'): (2, 0, 2), ('1', '10'): (1, 1, 2)}
    for (team, flat), (team_out, flat_out, _) in got.items():
        assert (team_out, bool(flat_out)) == _knobs(team, flat)
