"""Bottleneck features as a pipeline entry: the configuration layer (no device needed; the weights directory is
written by ``write_weights`` of tests/test_bottleneck.py) and the corpora of tests/test_bottleneck_pipeline_gpu.py
with the conditions those tests rest on, checked here on the float64 statement's VAD (tests/bottleneck_f64.py)."""

import numpy as np
import pytest

import bottleneck_f64 as f64
from shennong_amd import Audio, Utterances, pipeline
from shennong_amd.logger import get_logger
from test_bottleneck import weights_dir, write_weights  # noqa: F401  (fixture)

HIDDEN = 96


def burst(seed, length, rate):
    """`length` samples at `rate` of speech-like bursts: a gated tone with noise over a low noise floor (what
    ``ragged_batch`` of tests/test_bottleneck_gpu.py makes at 8 kHz)"""
    rng = np.random.RandomState(seed)
    t = np.arange(length) / float(rate)
    gate = np.sin(2 * np.pi * (2.0 + 0.1 * (seed % 7)) * t + 0.3 * seed) > -0.2
    x = gate * (5000.0 * np.sin(2 * np.pi * (200.0 + 15 * (seed % 10)) * t) + 800.0 * rng.randn(length))
    return np.clip(np.round(x + 15.0 * rng.randn(length)), -32768, 32767).astype(np.int16)


def ragged(n=7):
    """`n` utterances of different lengths, 0.35 to 0.45 s at 8 kHz"""
    rng = np.random.RandomState(5)
    return [burst(i, 2800 + 113 * i + int(rng.randint(0, 50)), 8000) for i in range(n)]


def corpus():
    """Three utterances of 0.6 to 1.05 s with odd lengths: 16 kHz, 8 kHz, 16 kHz; two speakers"""
    return [('u0', Audio(burst(31, 16643, 16000), 16000), 's0'), ('u1', Audio(burst(32, 4815, 8000), 8000), 's1'),
            ('u2', Audio(burst(33, 9999, 16000), 16000), 's0')]


def silent():
    """0.5 s at 8 kHz without a voiced frame: a constant"""
    return Audio(np.full(4000, 7, dtype=np.int16), 8000)


def at_8k(audio):
    """The int16 samples at 8 kHz on the host: Kaldi's resampler as the oracle states it (cutoff 0.99 x 4 kHz, 6
    zero crossings), rounded and clipped - the device resampler's result to within a level or so"""
    if audio.sample_rate == 8000:
        return audio.data
    from oracle import oracle as orc
    out = orc.linear_resample(audio.data.astype(np.float32), audio.sample_rate, 8000, 0.99 * 4000.0, 6)
    return np.clip(np.rint(out), -32768, 32767).astype(np.int16)


def bottleneck_config(dither=0.0, **entries):
    config = {'bottleneck': pipeline.get_bottleneck_config()}
    config['bottleneck']['dither'] = dither
    config.update(entries)
    return config


def test_get_bottleneck_config(tmp_path, monkeypatch):
    """The two defaults, from the constructor's signature: no weights directory is needed to write the entry"""
    monkeypatch.setenv('SHENNONG_AMD_BOTTLENECK_DIR', str(tmp_path / 'nowhere'))
    assert pipeline.get_bottleneck_config() == {'weights': 'BabelMulti', 'dither': 0.1}
    entry = pipeline.get_bottleneck_config()
    entry['dither'] = 0
    assert pipeline.get_bottleneck_config()['dither'] == 0.1


def test_default_config_still_refuses():
    assert pipeline.valid_features() == ['spectrogram', 'filterbank', 'mfcc', 'plp']
    with pytest.raises(ValueError, match='invalid features "bottleneck"'):
        pipeline.get_default_config('bottleneck')


def test_init_config_accepts_and_logs(weights_dir, capsys):  # noqa: F811
    write_weights(weights_dir, hidden=HIDDEN)
    config = bottleneck_config(cmvn={'by_speaker': True}, delta=pipeline._processor_params('delta'))
    config['pitch'] = pipeline.get_default_config('mfcc', with_pitch='kaldi')['pitch']
    try:
        parsed = pipeline._init_config(config, log=get_logger('pipeline', 'info'))
    finally:
        get_logger('pipeline', 'warning')   # (the level and stream the other tests of the session expect)
    assert parsed['bottleneck'] == {'weights': 'BabelMulti', 'dither': 0.0}
    assert parsed['cmvn']['with_vad'] is True
    assert ('pipeline configured for bottleneck features extraction with kaldi pitch, delta, cmvn by speaker with vad'
            in capsys.readouterr().err)


@pytest.mark.parametrize('comments', [False, True])
def test_yaml_round_trip(weights_dir, comments):  # noqa: F811
    write_weights(weights_dir, hidden=HIDDEN)
    config = bottleneck_config(0.1, cmvn={'by_speaker': False, 'with_vad': False})
    text = pipeline._get_config_to_yaml(config, comments=comments)
    assert 'bottleneck:' in text and 'weights: BabelMulti' in text
    if comments:
        assert '# Amount of dithering' in text
    assert pipeline._init_config(text) == config


def test_one_and_only_one_features_entry(weights_dir):  # noqa: F811
    write_weights(weights_dir, hidden=HIDDEN)
    config = bottleneck_config()
    config['mfcc'] = pipeline.get_default_config('mfcc')['mfcc']
    with pytest.raises(ValueError) as err:
        pipeline._init_config(config)
    assert 'more than one features extraction processors are defined' in str(err.value)
    assert str(err.value).endswith(': bottleneck, mfcc')
    with pytest.raises(ValueError) as err:
        pipeline._init_config({'delta': pipeline._processor_params('delta')})
    assert 'one and only one entry of spectrogram, filterbank, mfcc, plp, bottleneck' in str(err.value)


def test_vtln_is_refused(weights_dir):  # noqa: F811
    from shennong_amd.processor.vtln import VtlnProcessor
    write_weights(weights_dir, hidden=HIDDEN)
    sentence = 'bottleneck features do not support VTLN'
    with pytest.raises(ValueError) as err:
        pipeline._init_config(bottleneck_config(vtln=VtlnProcessor().get_params()))
    assert str(err.value) == sentence
    utts = Utterances([(name, audio) for name, audio, _ in corpus()])
    with pytest.raises(ValueError) as err:
        pipeline.extract_features(bottleneck_config(), utts, warps={name: 1.0 for name in ('u0', 'u1', 'u2')})
    assert str(err.value) == sentence
    with pytest.raises(ValueError) as err:
        pipeline.extract_features_warp(bottleneck_config(), utts, 1.1)
    assert str(err.value) == sentence


def test_bad_parameters_carry_the_prefix(weights_dir, tmp_path, monkeypatch):  # noqa: F811
    write_weights(weights_dir, hidden=HIDDEN)
    config = bottleneck_config()
    config['bottleneck']['weights'] = 'bad'
    with pytest.raises(ValueError) as err:
        pipeline._init_config(config)
    assert str(err.value) == 'error in configuration: bottleneck: invalid weights "bad", choose in "BabelMulti"'
    config = bottleneck_config()
    config['bottleneck']['window'] = 'hamming'
    with pytest.raises(ValueError, match='^error in configuration: bottleneck: '):
        pipeline._init_config(config)
    empty = tmp_path / 'empty'
    empty.mkdir()
    monkeypatch.setenv('SHENNONG_AMD_BOTTLENECK_DIR', str(empty))
    with pytest.raises(RuntimeError) as err:
        pipeline._init_config(bottleneck_config())
    assert str(err.value) == 'error in configuration: bottleneck: no weights file found in {}'.format(empty)


def test_memory_estimates_count_the_bounded_scratch():
    """A bottleneck entry adds its 8 kHz copy per hour of audio and, per batch in flight, the extractor's bounded
    scratch - nothing per row for the 144-column input and the first stage, which live in that scratch"""
    seen = []

    def estimate(*args):
        seen.append(args)
        return 'sized'
    assert pipeline._sized(estimate, 'corpus', {'bottleneck': {}}) == 'sized'
    assert seen == [('corpus', 2 * 8000 * 3600, 1 << 30)]
    assert pipeline._sized(estimate, 'corpus', {'mfcc': {}}) == 'sized' and seen[1] == ('corpus',)


def test_gpu_corpus_conditions():
    """What tests/test_bottleneck_pipeline_gpu.py rests on: every utterance of its corpora has voiced frames (so
    the CMVN with VAD accumulates something and no status bit is set), away from the all-or-nothing edge, and
    the silent one has none"""
    for name, audio, _ in corpus():
        samples = at_8k(audio)
        mask = f64.vad(samples)
        print('%s: %d samples at 8 kHz, %d of %d frames voiced' % (name, samples.shape[0], mask.sum(), mask.size))
        assert mask.size == f64.num_frames(samples.shape[0]) >= 40
        assert 10 <= mask.sum() < mask.size, name
        # The CMVN weights come from the energy VAD, whose energy is dithered (one level of Gaussian noise) with
        # another draw in the pipeline than in a processor called by hand.  The by-hand chain has the pipeline's
        # bits only if no decision depends on the draw: a frame of 200 samples of standard deviation s >= 8 (the
        # noise floor here) moves by about 2 / (s sqrt(200)) + 1 / s^2 < 0.035 in log energy, a few deviations
        # included, so every frame must be at least 0.1 away from the threshold 5 + 0.5 mean(E)
        frames = np.stack([samples[80 * f:80 * f + 200] for f in range(mask.size)]).astype(np.float64)
        energy = np.log(((frames - frames.mean(axis=1, keepdims=True)) ** 2).sum(axis=1))
        margin = np.abs(energy - (5.0 + 0.5 * energy.mean())).min()
        print('%s: log energies %.2f to %.2f, nearest to the VAD threshold %.3f' % (
            name, energy.min(), energy.max(), margin))
        assert frames.std(axis=1).min() >= 8.0 and margin >= 0.1, name
    for i, samples in enumerate(ragged()):
        mask = f64.vad(samples)
        assert 10 <= mask.sum() < mask.size, i
    assert len({w.shape[0] for w in ragged()}) == 7
    assert not f64.vad(silent().data).any()
