"""Every form of the pitch tracker's Viterbi stage at its state-count and batch seams (tests/pitch_state_cases.py;
tests/test_pitch_state_cases.py checks the table on the CPU): the by-state kernel in its three instantiations, the
teams of two and four waves and the lane-per-candidate kernel, at the state counts where their level formulas, their
register slices and the route change, on batches of 1, 7, 8, 9 and 17 ragged utterances of 1 .. 129 and 501 frames
(voiced, digital silence, noise, a glide over the whole pitch range, the RecomputeBacktraces corner) and on the 17
with ten zero-frame utterances among them; and with penalty_factor = 0 on silence, where every candidate ties.

Every frame of every utterance - Viterbi state, pitch and POV NCCF - is the oracle's, bit for bit, and the forms that
run at a state count return the same bytes: there is no tolerance here.  A zero-frame utterance comes back empty.

Reused memory: every test starts from LDS full of NaN patterns and a device pool that hands buffers out poisoned (the
`gpu` fixture), and each run is repeated after LDS was filled again and a batch of noise went through the same form at
ANOTHER state count: the FLT_MAX padding behind the forward costs (kFwdPad) and the tail of the S4 rounding are
written by every call, not inherited.

The long-window queue of refine_levels: from 1369 states on the first frame of every utterance, and every frame of
digital silence, fills a wave's queue to its 128 entries in the second pass of level 3 and makes it work the queue
off in the middle of the level (tests/test_pitch_state_cases.py test_first_frame_fills_the_queue); the runs at 1369
and 1460 states take that branch, the run at 1368 stops one state short of it.  Levels 4 and 5 never come near (the
largest count of long windows seen in one frame: 51, level 5, 1460 states, noise).

The plan records one name, 'pitch', for the whole call, not the Viterbi kernel that ran: which form a run takes is
checked on the CPU (tests/test_pitch_state_cases.py test_every_run_takes_the_route_it_expects against the ladder of
tests/test_pitch_route.py)."""
import numpy as np
import pytest

import pitch_state_cases as pc
from shennong_amd import Audio, _backend
from shennong_amd.processor import KaldiPitchProcessor
from test_parity_gpu import _pitch_close

pytestmark = pytest.mark.gpu

_OUTPUTS = {}       # (S, run, batch) -> the matrices of that run, computed once per process


def _processor(S, **more):
    return KaldiPitchProcessor(**pc.options_kwargs(S, **more))


def set_knobs(setenv, delenv, team, flat):
    for name, value in (('SNF_PITCH_TEAM', team), ('SNF_PITCH_FLAT', flat)):
        if value is None:
            delenv(name)
        else:
            setenv(name, value)


def run_form(S, run, waves, setenv, delenv, **more):
    """the matrices of `waves` at S states under the knobs of `run` (copies: the plan's result block is reused)"""
    team, flat = pc.forms_at(S)[run][:2]
    set_knobs(setenv, delenv, team, flat)
    feats = _processor(S, **more)._process_batch([Audio(w, pc.SAMPLE_RATE, validate=False) for w in waves])
    return [np.array(f.data, copy=True) for f in feats]


def outputs(S, run, batch, setenv, delenv):
    key = (S, run, batch)
    if key not in _OUTPUTS:
        if batch == 'ties':
            _OUTPUTS[key] = run_form(S, run, pc.tie_waves(), setenv, delenv, penalty_factor=pc.TIE_PENALTY)
        else:
            _OUTPUTS[key] = run_form(S, run, pc.waves_of(batch), setenv, delenv)
    return _OUTPUTS[key]


def compare(got, want):
    """(frames, frames that differ from the oracle) of one utterance; shapes must agree"""
    if want.size == 0:
        assert got.size == 0, got.shape
        return 0, 0
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    return want.shape[0], int(np.any(got.view(np.uint32) != want.view(np.uint32), axis=1).sum())


def other_state_count(S):
    """a count of the table that another plan runs between the two runs of a test: more states than S where there
    are more (the words behind state S - 1 then held another run's costs), the same form where it exists there"""
    return 512 if S < 512 else 641 if S < 641 else 513


def _knob_setters(monkeypatch):
    return monkeypatch.setenv, lambda name: monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize('S, run', pc.GPU_CASES, ids=['%d-%s' % case for case in pc.GPU_CASES])
def test_pitch_seam(gpu, monkeypatch, S, run):
    setenv, delenv = _knob_setters(monkeypatch)
    for batch in pc.BATCHES:
        gots, wants = outputs(S, run, batch, setenv, delenv), pc.wanted_of(S, batch)
        assert len(gots) == len(wants) == len(pc.batch(batch))
        for u, (got, want) in enumerate(zip(gots, wants)):
            if want.size == 0:      # a zero-frame utterance: Kaldi's empty matrix
                assert got.shape == (0, 0), (batch, u)
            else:
                _pitch_close(got, want)
        # ... and the bytes of the by-state run of this state count (the same kernel where the route ignores the knob)
        if run != 'state':
            for got, ref in zip(gots, outputs(S, 'state', batch, setenv, delenv)):
                assert got.tobytes() == ref.tobytes(), batch
    # the neighbours of the zero-frame utterances have the rows they have in the batch without holes
    whole, holes = outputs(S, run, 'n17', setenv, delenv), outputs(S, run, 'holes', setenv, delenv)
    for u, index in enumerate(pc.batch('holes')):
        assert index < 0 or holes[u].tobytes() == whole[u].tobytes()
    # again, after LDS was filled with NaN patterns and the same knobs ran noise at another state count
    gpu.check(gpu.lib().snf_debug_fill_lds(0xFFFFFFFF))
    other = other_state_count(S)
    set_knobs(setenv, delenv, *pc.forms_at(S)[run][:2])
    between = _processor(other)._process_batch(
        [Audio(pc.noise(pc.FRAMES_TO_SAMPLES[frames], 200 + frames), pc.SAMPLE_RATE, validate=False)
         for frames in (129, 65, 64, 2, 128, 63, 1, 129, 64)])
    assert [f.data.shape[0] for f in between] == [129, 65, 64, 2, 128, 63, 1, 129, 64]
    again = run_form(S, run, pc.waves_of('holes'), setenv, delenv)
    for got, first in zip(again, holes):
        assert got.shape == first.shape and got.tobytes() == first.tobytes()


@pytest.mark.parametrize('S, run', pc.TIE_CASES, ids=['%d-%s' % case for case in pc.TIE_CASES])
def test_pitch_ties(gpu, monkeypatch, S, run):
    """penalty_factor = 0 on seventeen utterances of digital silence, three of them without a frame: a step costs
    nothing and all forward costs are equal, so every candidate of every state ties and the lowest index has to win
    wherever two partial results meet - state 0 in every frame (tests/pitch_state_cases.py TIE_S).

    Silence only.  With penalty_factor = 0 on other signals the forward costs tie in part, and there Kaldi's search
    keeps another of the tied minima than the first (tests/test_pitch_state_cases.py
    test_kaldi_search_on_partial_ties): seen once, at 641 states on the 501-frame utterance of the recompute corner,
    where 6 frames of the by-state kernel lie one state from the oracle's."""
    setenv, delenv = _knob_setters(monkeypatch)
    gots, wants = outputs(S, run, 'ties', setenv, delenv), pc.tie_wanted(S)
    assert len(gots) == len(wants) == len(pc.TIE_FRAMES)
    for got, want in zip(gots, wants):
        if want.size == 0:
            assert got.shape == (0, 0)
        else:
            _pitch_close(got, want)
    if run != 'state':
        for got, ref in zip(gots, outputs(S, 'state', 'ties', setenv, delenv)):
            assert got.tobytes() == ref.tobytes()


def test_pitch_state_space_beyond_lds_is_refused(gpu, monkeypatch):
    """1461 states: the by-state form would need more than the 160 KiB of a workgroup.  The host refuses the call -
    with the route's message, before anything is launched -, the plan answers the next call the same way, and the
    process goes on: the largest state space that fits runs right behind it."""
    setenv, delenv = _knob_setters(monkeypatch)
    waves = pc.waves_of('n9')
    refused = _processor(pc.REFUSED_S)
    for team in ('1', '4', None):       # (a team does not run above 512 states: the knob changes nothing)
        set_knobs(setenv, delenv, team, None)
        for _ in range(2):
            with pytest.raises(RuntimeError, match='pitch state space does not fit in LDS'):
                refused._process_batch([Audio(w, pc.SAMPLE_RATE, validate=False) for w in waves])
    # a call without a frame is no work at all, on that plan too
    empty = refused._process_batch([Audio(pc.too_short(3), pc.SAMPLE_RATE, validate=False)])
    assert empty[0].data.size == 0
    S = pc.LDS_LIMIT_S
    for got, want in zip(run_form(S, 'state', waves, setenv, delenv), pc.wanted_of(S, 'n9')):
        _pitch_close(got, want)
