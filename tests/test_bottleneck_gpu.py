"""BottleneckProcessor on the device, through the public class and through the C ABI, against the
reference's float64 outputs in tests/golden/reference_bottleneck.npz.

Error bound of the float32 device path, stage by stage: the test evaluates tests/bottleneck_f64.py in
float32 on the same input, takes its largest absolute error against the fixture, and allows the device 4
times that (another accumulation order in the matrix cores, a device exp, a float32 transform), never more
than the 2e-2 absolute of the reference's own comparison with the original extractor.  Measured figures are
printed; DESIGN 4.9 records them."""

import os

import numpy as np
import pytest

import bottleneck_f64 as f64
from test_bottleneck import STEM, cases, write_weights

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FACTOR, CEILING = 4.0, 2e-2


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'reference_bottleneck.npz')) as data:
        return {k: data[k] for k in data.files}


def processor_for(directory, monkeypatch, seed, hidden, context, dither=0.0):
    """A BottleneckProcessor over synthetic weights written in the published format"""
    from shennong_amd.processor import BottleneckProcessor
    os.makedirs(str(directory), exist_ok=True)
    monkeypatch.setenv('SHENNONG_AMD_BOTTLENECK_DIR', str(directory))
    write_weights(directory, 'BabelMulti', seed=seed, hidden=hidden, context=context)
    return BottleneckProcessor(weights='BabelMulti', dither=dither)


def bound(f32_value, want):
    return min(FACTOR * float(np.abs(f32_value.astype(np.float64) - want).max()), CEILING)


def ragged_batch(n, seed=5):
    """`n` utterances of different lengths (0.35 .. 1.1 s at 8 kHz) with speech-like bursts"""
    rng = np.random.RandomState(seed)
    waves = []
    for i in range(n):
        length = 2800 + 113 * i + int(rng.randint(0, 50))
        t = np.arange(length) / 8000.0
        gate = (np.sin(2 * np.pi * (2.0 + 0.1 * (i % 7)) * t + 0.3 * i) > -0.2)
        x = gate * (5000.0 * np.sin(2 * np.pi * (200.0 + 15 * i) * t) + 800.0 * rng.randn(length)) + 15.0 * rng.randn(length)
        waves.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    return waves


def test_fixture_cases(gpu, golden, tmp_path, monkeypatch):
    from shennong_amd import Audio
    from shennong_amd.processor import bottleneck
    for n in cases(golden):
        seed, hidden, context = (int(v) for v in golden['case_' + n])
        key = str(golden['signal_' + n])
        samples = golden['input_' + key]
        proc = processor_for(tmp_path / n, monkeypatch, seed, hidden, context)
        low = f64.extract(samples, f64.make_weights(seed, hidden, context), np.float32)
        # through the C ABI, stage by stage
        batch = bottleneck.BottleneckBatch([samples])
        voiced = batch.vad()
        np.testing.assert_array_equal(batch.host_mask(), golden['vad_' + key])
        assert int(voiced[0]) == int(golden['vad_' + key].sum())
        batch.fbank(0.0)
        out = batch.forward(proc._device_network(batch.device))
        stages = {'logmel': (batch.host_logmel(), golden['logmel_' + key]),
                  'bn': (batch.host_bn(), golden['bn_' + n]), 'out': (out, golden['out_' + n])}
        for stage, (got, want) in stages.items():
            assert got.shape == want.shape and got.dtype == np.float32
            err = float(np.abs(got.astype(np.float64) - want).max())
            limit = bound(low[stage], want)
            print('%s %s: device %.3g, float32 numpy %.3g, bound %.3g' % (n, stage, err, limit / FACTOR, limit))
            assert err <= limit, (n, stage, err, limit)
        # through the public class
        feats = proc.process(Audio(samples, 8000))
        assert feats.shape == golden['out_' + n].shape and feats.dtype == np.float32
        np.testing.assert_array_equal(feats.data, out)
        np.testing.assert_array_equal(feats.times, f64.times(feats.shape[0]))
        assert feats.properties == proc.get_properties()


@pytest.mark.parametrize('act', ['identity', 'sigmoid'])
def test_dense_layer(gpu, act):
    from shennong_amd.processor import bottleneck
    rng = np.random.RandomState(1)
    shapes = [(1, 1, 1), (1, 144, 500), (63, 80, 96), (63, 96, 200), (63, 400, 1500), (63, 1500, 80),
              (63, 200, 1), (63, 1, 400), (1000, 144, 1500), (1000, 1500, 1500), (1000, 500, 500),
              (1000, 400, 96), (1000, 96, 144), (1000, 200, 80)]
    for m, k, n in shapes:
        x = rng.uniform(0.0, 1.0, (m, k)).astype(np.float32)
        w = (rng.uniform(-1.0, 1.0, (k, n)) / np.sqrt(k)).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, n).astype(np.float32)
        want = x.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
        low = x @ w + b
        if act == 'sigmoid':
            want, low = f64._sigmoid(want), f64._sigmoid(low)
        got = bottleneck.dense_layer(x, w, b, act)
        assert got.shape == (m, n) and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - want).max())
        limit = bound(low, want)
        print('dense %s %dx%dx%d: device %.3g, float32 numpy %.3g' % (act, m, k, n, err, limit / FACTOR))
        assert err <= limit, (act, m, k, n, err, limit)
        # a row alone gives the bits it has in the block
        row = m // 2
        np.testing.assert_array_equal(bottleneck.dense_layer(x[row:row + 1], w, b, act)[0], got[row])


def test_dense_layer_invalid(gpu):
    L, ptr = gpu.lib(), 256
    assert L.snf_dense_layer(0, ptr, -1, 4, ptr, ptr, 4, 0, ptr, None) == -1
    assert L.snf_dense_layer(0, ptr, 4, 0, ptr, ptr, 4, 0, ptr, None) == -1
    assert L.snf_dense_layer(0, ptr, 4, 4, ptr, ptr, 4, 2, ptr, None) == -1
    assert L.snf_dense_layer(0, None, 4, 4, ptr, ptr, 4, 0, ptr, None) == -1
    assert L.snf_dense_layer(0, ptr, 4, 4, None, ptr, 4, 0, ptr, None) == -1


def test_batch_invariance(gpu, tmp_path, monkeypatch):
    from shennong_amd import Audio, Utterances
    proc = processor_for(tmp_path, monkeypatch, seed=21, hidden=200, context=5)
    waves = ragged_batch(53)
    audios = [Audio(w, 8000) for w in waves]
    assert len({w.shape[0] for w in waves}) == len(waves)
    alone = [proc.process(a).data for a in audios]
    utts = Utterances([('utt%02d' % i, a) for i, a in enumerate(audios)])
    together = proc.process_all(utts)
    assert list(together.keys()) == ['utt%02d' % i for i in range(len(waves))]
    for i, want in enumerate(alone):
        got = together['utt%02d' % i]
        assert got.shape == want.shape == (f64.num_frames(len(waves[i])), 80)
        np.testing.assert_array_equal(got.data, want)
    # one utterance first, in the middle and last in batches of another order
    probe = 17
    for position in (0, 26, 52):
        order = [i for i in range(53) if i != probe]
        order.insert(position, probe)
        feats = proc._process_batch([audios[i] for i in order])
        np.testing.assert_array_equal(feats[position].data, alone[probe])


def test_silence(gpu, tmp_path, monkeypatch):
    from shennong_amd import Audio, Utterances
    proc = processor_for(tmp_path, monkeypatch, seed=22, hidden=96, context=5)
    silence = Audio(np.zeros(8000, dtype=np.int16), 8000)
    with pytest.raises(RuntimeError) as err:
        proc.process(silence)
    assert str(err.value) == 'no voice detected in signal, failed to extract features'
    speech = Audio(ragged_batch(2)[1], 8000)
    with pytest.raises(RuntimeError) as err:
        proc.process_all(Utterances([('first', speech), ('quiet', silence)]))
    assert 'no voice detected in signal' in str(err.value) and '"quiet"' in str(err.value)
    with pytest.raises(ValueError, match='too short'):
        proc.process(Audio(np.zeros(150, dtype=np.int16), 8000))


def test_resampled_input(gpu, tmp_path, monkeypatch, audio, capsys):
    proc = processor_for(tmp_path, monkeypatch, seed=23, hidden=96, context=5)
    proc.set_logger('debug')
    signal = audio.astype(np.float32)
    assert signal.sample_rate == 16000
    feats = proc.process(signal)
    frames = f64.num_frames(signal.resample(8000).data.shape[0])
    assert feats.shape == (frames, 80) and frames == 140
    np.testing.assert_array_equal(feats.times, f64.times(frames))
    log = capsys.readouterr().err
    assert 'resampling audio from 16000Hz@32b to 8000Hz@16b' in log
    assert 'frames of speech detected (on 140 total frames)' in log


def test_dither(gpu, golden, tmp_path, monkeypatch):
    from shennong_amd import Audio
    from shennong_amd.processor import bottleneck
    samples = golden['input_wav']
    proc = processor_for(tmp_path, monkeypatch, seed=24, hidden=200, context=5, dither=0.1)
    audio = Audio(samples, 8000)
    noisy = proc.process(audio).data
    assert np.isfinite(noisy).all()
    np.testing.assert_array_equal(proc.process(audio).data, noisy)          # the noise is keyed by the utterance
    other = Audio(ragged_batch(3)[2], 8000)
    np.testing.assert_array_equal(proc._process_batch([other, audio])[1].data, noisy)
    proc.dither = 0.0
    clean = proc.process(audio).data
    assert not np.array_equal(clean, noisy)
    # the log-mel energies move by what +-0.1 LSB of uniform noise explains: the noise energy of a windowed
    # frame is dither^2 / 3 * sum(window^2) per bin before the filters; relative to frames of speech that is
    # far below 1e-3 in the log domain, and the two runs must differ somewhere
    batch = bottleneck.BottleneckBatch([samples])
    batch.fbank(0.0)
    quiet = batch.host_logmel().astype(np.float64)
    batch.fbank(0.1)
    dithered = batch.host_logmel().astype(np.float64)
    batch.fbank(0.1, seed=1)
    reseeded = batch.host_logmel().astype(np.float64)
    diff = np.abs(dithered - quiet)
    assert 0 < diff.max() < 0.05 and np.median(diff) < 1e-3
    assert not np.array_equal(reseeded, dithered)
    # ten times the dither, about ten times the change (linear regime; the median is robust)
    batch.fbank(1.0)
    louder = np.abs(batch.host_logmel().astype(np.float64) - quiet)
    ratio = np.median(louder) / max(np.median(diff), 1e-12)
    print('dither: median |d logmel| %.3g at 0.1, %.3g at 1.0 (ratio %.3g)' % (np.median(diff), np.median(louder), ratio))
    assert 1.5 < ratio < 30.0   # (10 in the linear regime; float32 rounding of the log floors the smaller one)
    assert float(np.abs(noisy - clean).max()) < 0.05
