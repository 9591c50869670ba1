"""CREPE pitch as a pipeline entry: ``extract_features`` and ``extract_features_streamed`` against the composition
of the public processors, on seeded synthetic weights (the smallest capacity of tests/test_crepe.py).

The pipeline keeps the whole pitch path on the device - the rows are resampled by ``snf_crepe_rows`` (1e-13 from
scipy) and converted by ``snf_crepe_voicing_convert`` (one float32 ulp from the host functions) - while the public
processors download after the decoder and finish on the host: the pitch columns are compared at the tolerance
tests/test_parity_gpu.py::test_pitch_post allows KaldiPitchPostProcessor against the oracle (``assert_close`` with
rtol 1e-4 and the 'pitch_post' absolute term of tests/conftest.py), everything else bit for bit.

Every step on the device runs under its own time limit (the guard of tests/test_crepe_gpu.py)."""

import numpy as np
import pytest

from conftest import assert_close
from shennong_amd import Audio, Utterances, pipeline, synth
from shennong_amd.utils import dict_equal
from test_crepe import END_TO_END_CAPACITIES, write_weights
from test_crepe_gpu import on_device

pytestmark = pytest.mark.gpu
CAPACITY, SEED = END_TO_END_CAPACITIES[0]


def corpus():
    """Three utterances of 0.3 to 1.0 s: 16 kHz, 8 kHz, 16 kHz (odd lengths)"""
    waves = [(synth.utterances(31, 1, 8321, 16000)[0], 16000), (synth.utterances(32, 1, 4815, 8000)[0], 8000),
             (synth.utterances(33, 1, 15999, 16000)[0], 16000)]
    return [(f'u{i}', Audio(w, rate)) for i, (w, rate) in enumerate(waves)]


def crepe_config(viterbi=True, center=True, cmvn=False):
    config = pipeline.get_default_config('mfcc', with_delta=True, with_cmvn=cmvn)
    config['mfcc']['dither'] = 0
    if cmvn:
        config['cmvn']['by_speaker'] = False
    config['pitch'] = pipeline.get_crepe_pitch_config()
    config['pitch'].update(model_capacity=CAPACITY, viterbi=viterbi, center=center)
    config['pitch']['postprocessing']['delta_pitch_noise_stddev'] = 0
    return config


def composition(config, audio):
    """MfccProcessor -> delta, CrepePitchProcessor.process (the device resampler for audio that is not at
    16 kHz) -> CrepePitchPostProcessor.process, Features.concatenate(tolerance=2)"""
    from shennong_amd.postprocessor import DeltaPostProcessor
    from shennong_amd.processor import CrepePitchPostProcessor, CrepePitchProcessor, MfccProcessor
    mfcc = MfccProcessor(**config['mfcc'])
    mfcc.sample_rate = audio.sample_rate
    feats = DeltaPostProcessor(**config['delta']).process(mfcc.process(audio))
    params = {k: v for k, v in config['pitch'].items() if k not in ('processor', 'postprocessing')}
    tracker = CrepePitchProcessor(frame_shift=mfcc.frame_shift, frame_length=mfcc.frame_length, **params)
    if audio.sample_rate != 16000:
        tracker.resample = 'kaldi'
    pitch = CrepePitchPostProcessor(**config['pitch']['postprocessing']).process(tracker.process(audio))
    return feats.concatenate(pitch, tolerance=2)


def install_weights(directory, monkeypatch, viterbi=True):
    """The seeded weights.  Without the smoothing their argmax jumps between 115 and 1 700 Hz from frame to frame
    and the Fourier resampling of such rows rings below zero - 'Not all pitch values are positive' on the host path
    and here alike -, so the cases without smoothing get a hill on the classifier's bias (6 at bin 180, 8 bins wide)
    that keeps the argmax within a few bins; the confidence is then 0.997 and the clamp has rows to act on."""
    import crepe_f64 as f64
    monkeypatch.setenv('SHENNONG_AMD_CREPE_DIR', str(directory))
    replace = {}
    if not viterbi:
        hill = 6.0 * np.exp(-0.5 * ((np.arange(f64.BINS) - 180) / 8.0) ** 2)
        replace['classifier/bias'] = f64.make_weights(CAPACITY, SEED)['classifier/bias'] + hill
    write_weights(directory, CAPACITY, SEED, **replace)


@pytest.mark.parametrize('viterbi', [True, False])
@pytest.mark.parametrize('center', [True, False])
def test_extract_features_is_the_composition(gpu, tmp_path, monkeypatch, viterbi, center):
    """`center` True resamples the rows down (more network frames than rows), False up"""
    install_weights(tmp_path, monkeypatch, viterbi)
    config = crepe_config(viterbi, center)
    utts = corpus()
    with on_device():
        got = pipeline.extract_features(config, Utterances(utts))
        want = {name: composition(config, audio) for name, audio in utts}
    assert list(got.keys()) == [name for name, _ in utts]
    for name, audio in utts:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.shape[1] == 39 + 3 and g.dtype == w.dtype == np.float32, name
        assert np.array_equal(g.times, w.times), name
        properties = {k: v for k, v in g.properties.items() if k != 'audio'}
        assert dict_equal(properties, w.properties), name
        assert ('resample' in g.properties['crepe']) == (audio.sample_rate != 16000)
        assert np.array_equal(g.data[:, :39], w.data[:, :39]), name
        assert_close(g.data[:, 39:], w.data[:, 39:], rtol=1e-4, family='pitch_post', what=f'crepe pitch columns {name}')
        err = np.abs(g.data[:, 39:].astype(np.float64) - w.data[:, 39:])
        print('pipeline viterbi=%s center=%s %s: %d rows, pitch columns differ by at most %.3g, %.4f bit-equal' % (
            viterbi, center, name, g.shape[0], err.max(), (g.data[:, 39:] == w.data[:, 39:]).mean()))


@pytest.mark.parametrize('viterbi,center', [(True, True), (False, False)])
def test_streamed_in_two_batches_is_one_shot(gpu, tmp_path, monkeypatch, viterbi, center):
    install_weights(tmp_path, monkeypatch, viterbi)
    config = crepe_config(viterbi, center, cmvn=True)
    utts = Utterances(corpus())
    assert utts.duration() > 1.2 > max(u.duration for u in utts)
    batches = []
    with on_device():
        want = pipeline.extract_features(config, utts)
        pipeline.extract_features_streamed(config, utts, batches.append, max_batch_duration=1.2)
    assert len(batches) == 2 and sorted(len(b) for b in batches) == [1, 2]
    got = {name: feats for batch in batches for name, feats in batch.items()}
    assert sorted(got) == sorted(want.keys())
    for name in got:
        assert got[name].shape[1] == 42
        assert np.array_equal(got[name].data, want[name].data), name
        assert np.array_equal(got[name].times, want[name].times), name
        assert dict_equal(got[name].properties, want[name].properties), name


def test_by_stage_path_composes_the_public_processors(gpu, tmp_path, monkeypatch):
    """The host cross-check path with a CREPE entry: the public processors, with the device resampler for the
    8 kHz utterance like the device-resident path - the same shapes, times and properties, the other columns bit
    for bit, the pitch columns at the tolerance of the module's docstring"""
    from shennong_amd.logger import get_logger
    install_weights(tmp_path, monkeypatch)
    config = pipeline._init_config(crepe_config())
    utts = Utterances(corpus())
    with on_device():
        want = pipeline.extract_features(config, utts)
        got = pipeline._extract_features_by_stage(config, utts, None, get_logger('pipeline', 'warning'))
    assert list(got.keys()) == list(want.keys())
    for name in want.keys():
        g, w = got[name], want[name]
        assert g.shape == w.shape and np.array_equal(g.times, w.times), name
        assert dict_equal(g.properties, w.properties), name
        assert np.array_equal(g.data[:, :39], w.data[:, :39]), name
        assert_close(g.data[:, 39:], w.data[:, 39:], rtol=1e-4, family='pitch_post', what=f'by stage {name}')
    assert got['u1'].properties['crepe']['resample'] == 'kaldi'


def test_too_short_raises_before_any_launch(gpu, tmp_path, monkeypatch):
    """200 samples make a network frame but no output row: the processors' message, with the name, and nothing
    of the batch (one sample rate: one group of the pipeline) has been launched when it is raised"""
    from shennong_amd.processor import CrepePitchProcessor, pitch_crepe
    from shennong_amd import _backend
    install_weights(tmp_path, monkeypatch)
    config = crepe_config()
    utts = corpus()[::2] + [('short', Audio(synth.utterances(34, 1, 200, 16000)[0], 16000))]
    with pytest.raises(ValueError) as processors:
        with on_device():
            CrepePitchProcessor(model_capacity=CAPACITY).process_all(Utterances(utts))
    assert str(processors.value) == 'audio "short" too short: 200 samples at 16 kHz'

    def refuse(*args, **kwargs):
        raise AssertionError('a launch before the check of the lengths')
    monkeypatch.setattr(pitch_crepe.CrepeBatch, 'from_device', refuse)
    monkeypatch.setattr(_backend.Plan, 'run_device', refuse)
    with pytest.raises(ValueError) as piped:
        with on_device():
            pipeline.extract_features(config, Utterances(utts))
    assert str(piped.value) == str(processors.value)


def test_unvoiced_utterance_raises_the_processors_message(gpu, tmp_path, monkeypatch):
    """A classifier whose sigmoids are all near zero: no confidence reaches the clamp's 1e-2, no frame is voiced"""
    from shennong_amd.processor import CrepePitchPostProcessor, CrepePitchProcessor, pitch_crepe
    shapes = pitch_crepe.expected_shapes(CAPACITY)
    monkeypatch.setenv('SHENNONG_AMD_CREPE_DIR', str(tmp_path))
    write_weights(tmp_path, CAPACITY, SEED, **{'classifier/bias': np.full(shapes['classifier/bias'], -30.0),
                                               'classifier/kernel': np.zeros(shapes['classifier/kernel'])})
    config = crepe_config()
    utts = corpus()
    with on_device():
        raw = CrepePitchProcessor(model_capacity=CAPACITY).process(utts[0][1])
    assert not raw.data[:, 0].any()
    with pytest.raises(ValueError) as processors:
        CrepePitchPostProcessor().process(raw)
    with pytest.raises(ValueError) as piped:
        with on_device():
            pipeline.extract_features(config, Utterances(utts))
    assert str(piped.value) == str(processors.value) == 'No voiced frames'
