"""linear_resample_kernel through ``snf_linear_resample`` and through the public surface that uses it.

The kernel runs the oracle's chain (oracle/kaldi_oracle.c linres_apply: one fused multiply-add per tap, taps
ascending, from 0.0f) on the oracle's weights, so every check here is equality of bits with
``oracle.linear_resample`` at ResampleWaveform's cutoff and width - no tolerance; the int16 form is that float
result rounded to nearest (ties to even) and clamped."""

import numpy as np
import pytest

from oracle import oracle as orc
from test_bottleneck_gpu import processor_for as bottleneck_for
from test_bottleneck_gpu import ragged_batch
from test_crepe_gpu import processor_for as crepe_for
from test_resample import RATE_PAIRS, cutoff

pytestmark = pytest.mark.gpu


def reference(x, rate_in, rate_out):
    return orc.linear_resample(np.asarray(x, dtype=np.float32), rate_in, rate_out, cutoff(rate_in, rate_out), 6)


def as_int16(y):
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def device_resample(waves, rate_in, rate_out, starts=None, size=None, guard=None):
    """The waves (all int16 or all float32) resampled in one call -> (list of outputs, the whole destination);
    `starts`: where every output goes in a destination of `size` samples prefilled with `guard`"""
    from shennong_amd import _backend
    dtype = np.dtype(waves[0].dtype)
    kind = _backend.RESAMPLE_KINDS[dtype]
    soff = np.zeros(len(waves) + 1, dtype=np.int64)
    np.cumsum([len(w) for w in waves], out=soff[1:])
    # (a sample in front: never an empty upload, and offsets tables that do not start at 0 are covered)
    source = _backend.upload_rows([np.zeros(1, dtype=dtype)] + list(waves), dtype)
    soff += 1
    dst = None
    if starts is not None:
        dst = _backend.DeviceBuffer(size * dtype.itemsize)
        dst.upload(np.full(size, guard, dtype=dtype))
    block, out_soff = _backend.resample_device(source, soff, rate_in, rate_out, kind, dst=dst, dst_starts=starts)
    total = size if starts is not None else int(out_soff[-1])
    whole = block.download(np.empty(total, dtype=dtype)) if total else np.empty(0, dtype=dtype)
    where = out_soff[:-1] if starts is None else starts
    return [whole[a:a + n] for a, n in zip(where, np.diff(out_soff))], whole


def lengths_for(rate_in, rate_out):
    """Input lengths of the bit-for-bit check: tiny ones, those whose output count sits just below, at and just
    above every seam of the kernel's tiling (a chunk of 256 outputs, a workgroup's run of 1024) - when
    upsampling not every count exists: the nearest that do, on both sides -, and one of three workgroups"""
    from shennong_amd import _backend
    seams = [_backend.RESAMPLE_CHUNK, 2 * _backend.RESAMPLE_CHUNK, _backend.RESAMPLE_RUN, 2 * _backend.RESAMPLE_RUN]
    assert seams == [256, 512, 1024, 2048]
    lengths = {0, 1, 2, 3, 37}

    def count(n):
        return _backend.resample_num_out(rate_in, rate_out, n)

    for seam in seams:
        n = int((seam - 1) * rate_in / rate_out)
        while n > 0 and count(n) >= seam - 1:
            n -= 1
        first = {}   # output count -> the shortest input that gives it
        while not first or max(first) <= seam:
            first.setdefault(count(n), n)
            n += 1
        below, above = max(c for c in first if c < seam), min(c for c in first if c > seam)
        if rate_out < rate_in:
            assert (below, above) == (seam - 1, seam + 1) and seam in first
        lengths |= {first[below], first[above]} | ({first[seam]} if seam in first else set())
    three = int(2.3 * _backend.RESAMPLE_RUN * rate_in / rate_out)
    assert 2 * _backend.RESAMPLE_RUN < _backend.resample_num_out(rate_in, rate_out, three) <= 3 * _backend.RESAMPLE_RUN
    return sorted(lengths | {three})


@pytest.mark.parametrize('rate_in,rate_out', RATE_PAIRS)
def test_float32_equals_oracle(gpu, rate_in, rate_out):
    rng = np.random.RandomState(rate_in % 1000 + rate_out // 1000)
    waves = [(3000.0 * rng.randn(n)).astype(np.float32) for n in lengths_for(rate_in, rate_out)]
    got, _ = device_resample(waves, rate_in, rate_out)
    for wave, out in zip(waves, got):
        want = reference(wave, rate_in, rate_out)
        assert out.dtype == np.float32 and out.shape == want.shape, (len(wave), out.shape, want.shape)
        np.testing.assert_array_equal(out, want, err_msg=f'{len(wave)} samples')


def square_wave(n=4000, period=80):
    x = np.where((np.arange(n) // (period // 2)) % 2 == 0, 32767, -32768)
    return x.astype(np.int16)


def test_int16_equals_rounded_oracle(gpu, audio, audio_8k):
    cases = [(audio.data, 16000, 8000), (audio_8k.data, 8000, 16000), (square_wave(), 16000, 8000)]
    for wave, rate_in, rate_out in cases:
        assert wave.dtype == np.int16
        want = reference(wave, rate_in, rate_out)
        got, _ = device_resample([wave], rate_in, rate_out)
        assert got[0].dtype == np.int16
        np.testing.assert_array_equal(got[0], as_int16(want))
    # the square wave's overshoot is what the clamp is for (precondition of the case above)
    assert want.max() > 32767.5 and want.min() < -32768.5
    assert got[0].max() == 32767 and got[0].min() == -32768


@pytest.mark.parametrize('rate_in,rate_out,dtype', [(16000, 8000, np.int16), (44100, 16000, np.float32),
                                                    (8000, 44100, np.int16)])
def test_batch_invariance(gpu, rate_in, rate_out, dtype):
    """53 ragged utterances: the same bits alone, in the batch and at the first, a middle and the last position,
    with destinations scattered in an order that is not the utterances' and a guard value between the slots"""
    waves = [w.astype(dtype) for w in ragged_batch(53)]
    assert len({len(w) for w in waves}) == 53
    guard = dtype(31415)
    alone = [device_resample([w], rate_in, rate_out)[0][0] for w in waves]
    rounded = (lambda y: y) if dtype is np.float32 else as_int16
    for k in (0, 17, 52):
        np.testing.assert_array_equal(alone[k], rounded(reference(waves[k], rate_in, rate_out)))

    def scattered(order):
        """slots handed out in the order of a permutation, 3 to 9 guard samples around each"""
        rng = np.random.RandomState(len(order) + order[0])
        starts, at = np.zeros(len(order), dtype=np.int64), 5
        for u in rng.permutation(len(order)):
            starts[u] = at
            at += len(alone[order[u]]) + 3 + int(rng.randint(0, 7))
        assert np.any(np.diff(starts) < 0)
        got, whole = device_resample([waves[i] for i in order], rate_in, rate_out, starts=starts, size=at, guard=guard)
        used = np.zeros(at, dtype=bool)
        for u, i in enumerate(order):
            np.testing.assert_array_equal(got[u], alone[i], err_msg=f'utterance {i} at position {u}')
            assert not used[starts[u]:starts[u] + len(alone[i])].any()
            used[starts[u]:starts[u] + len(alone[i])] = True
        assert np.all(whole[~used] == guard)

    scattered(list(range(53)))
    probe = 17
    for position in (0, 26, 52):
        order = [i for i in range(53) if i != probe]
        order.insert(position, probe)
        scattered(order)
    # contiguous destinations, the default
    got, _ = device_resample(waves, rate_in, rate_out)
    for out, want in zip(got, alone):
        np.testing.assert_array_equal(out, want)


def test_audio_resample_kaldi(gpu, audio):
    from shennong_amd import Audio
    out = audio.resample(8000, backend='kaldi')
    assert isinstance(out, Audio) and out.dtype == np.int16 and out.sample_rate == 8000 and out.nsamples == 11357
    assert audio.resample(8000).nsamples == 11356
    np.testing.assert_array_equal(out.data, as_int16(reference(audio.data, 16000, 8000)))
    signal = audio.astype(np.float32)
    out = signal.resample(8000, backend='kaldi')
    assert out.dtype == np.float32 and out.sample_rate == 8000 and out.nsamples == 11357
    np.testing.assert_array_equal(out.data, reference(signal.data, 16000, 8000))


def test_bottleneck_kaldi(gpu, tmp_path, monkeypatch, audio, audio_8k, capsys):
    from shennong_amd import Audio, Utterances
    proc = bottleneck_for(tmp_path, monkeypatch, seed=3, hidden=96, context=5)
    # the default path is today's: Audio.resample on the host, then int16
    assert proc.resample == 'scipy'
    today = proc.process(Audio(audio.resample(8000).astype(np.int16).data, 8000))
    default = proc.process(audio)
    np.testing.assert_array_equal(default.data, today.data)
    assert 'resample' not in default.properties['bottleneck']

    proc.resample = 'kaldi'
    proc.set_logger('debug')
    down = as_int16(reference(audio.data, 16000, 8000))
    want = proc.process(Audio(down, 8000))
    capsys.readouterr()
    got = proc.process(audio)
    assert 'resampling audio from 16000Hz@16b to 8000Hz@16b' in capsys.readouterr().err
    assert got.shape == want.shape == (140, 80)
    np.testing.assert_array_equal(got.data, want.data)
    np.testing.assert_array_equal(got.times, want.times)
    assert got.properties['bottleneck']['resample'] == 'kaldi'
    assert not np.array_equal(got.data, default.data)
    # float32 audio: the int16 conversion comes first
    np.testing.assert_array_equal(proc.process(audio.astype(np.float32)).data, want.data)

    # rates mixed in one batch, native-rate audio on both sides of the others
    high = Audio(audio.data, 16000).resample(44100)
    assert high.sample_rate == 44100 and high.dtype == np.int16
    signals = [('a8', audio_8k), ('b16', audio), ('c44', high), ('d8', Audio(down, 8000)), ('e16', audio)]
    alone = {name: proc.process(signal).data for name, signal in signals}
    together = proc.process_all(Utterances(signals))
    assert list(together.keys()) == [name for name, _ in signals]
    for name, _ in signals:
        np.testing.assert_array_equal(together[name].data, alone[name], err_msg=name)
    np.testing.assert_array_equal(alone['d8'], alone['b16'])
    np.testing.assert_array_equal(
        alone['c44'], proc.process(Audio(as_int16(reference(high.data, 44100, 8000)), 8000)).data)
    with pytest.raises(ValueError, match='too short: 199 samples at 8 kHz give 0 frames'):
        proc.process(Audio(np.zeros(398, dtype=np.int16), 16000))


def test_crepe_kaldi(gpu, tmp_path, monkeypatch, audio, audio_8k):
    from shennong_amd import Audio, Utterances
    proc = crepe_for(tmp_path, monkeypatch, 'tiny', 11)
    default = proc.process(audio_8k)
    today = proc.process(Audio(audio_8k.resample(16000).astype(np.int16).data, 16000))
    np.testing.assert_array_equal(default.data, today.data)
    proc.resample = 'kaldi'
    up = as_int16(reference(audio_8k.data, 8000, 16000))
    want = proc.process(Audio(up, 16000))
    got = proc.process(audio_8k)
    assert got.shape == want.shape and got.shape[1] == 2
    np.testing.assert_array_equal(got.data, want.data)
    np.testing.assert_array_equal(got.times, want.times)
    assert got.properties['crepe']['resample'] == 'kaldi'
    together = proc.process_all(Utterances([('low', audio_8k), ('native', audio)]))
    np.testing.assert_array_equal(together['low'].data, want.data)
    np.testing.assert_array_equal(together['native'].data, proc.process(audio).data)
