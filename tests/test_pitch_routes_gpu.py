"""The route of the pitch tracker that no other test takes: fewer than 128 Viterbi states.

shennong_amd/csrc/pitch_route.h sends such a state space to pitch_viterbi_kernel whatever the batch size and the
knobs say (a team of waves and the lane-per-candidate kernel both start at 128 states), where it runs
viterbi_forward<7> (kernels_pitch_viterbi.hip) with ONE level-1 state: level 2 has no state at all and most of a
lane's seven register slices work on the last state again."""
import numpy as np
import pytest

from oracle import oracle as orc
from shennong_amd import Audio
from shennong_amd.processor import KaldiPitchProcessor

pytestmark = pytest.mark.gpu

OPTS = dict(min_f0=100, max_f0=300, delta_pitch=0.01)   # 111 states


def test_pitch_below_128_states(gpu, synth_waves, monkeypatch):
    proc = KaldiPitchProcessor(**OPTS)
    lags, _, _ = orc.pitch_lags(proc._options)
    assert 2 <= lags.shape[0] <= 127
    waves = list(synth_waves)[:3]
    want = [orc.pitch(proc._options, w) for w in waves]
    monkeypatch.delenv('SNF_PITCH_TEAM', raising=False)
    monkeypatch.delenv('SNF_PITCH_FLAT', raising=False)
    outs = [o.data for o in proc._process_batch([Audio(w, 16000) for w in waves])]
    for o, w in zip(outs, want):
        # every frame - Viterbi state, pitch and POV NCCF - is bit-identical to the oracle (test_pitch_option_paths)
        assert o.shape == w.shape
        np.testing.assert_array_equal(o[:, 1], w[:, 1])
        np.testing.assert_array_equal(o[:, 0], w[:, 0])
    # a forced team size is not honoured below 128 states: the same kernel, the same bytes
    monkeypatch.setenv('SNF_PITCH_TEAM', '4')
    again = [o.data for o in proc._process_batch([Audio(w, 16000) for w in waves])]
    for o, a in zip(outs, again):
        assert o.tobytes() == a.tobytes()
