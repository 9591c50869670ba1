"""CrepePitchProcessor on the device, through the public classes and through the C ABI, against the float64
statement of tests/crepe_f64.py on seeded synthetic weights (no pretrained model is needed).

Error bound of the float32 device path: the test evaluates the statement in float32 numpy on the same input,
takes its largest absolute error against the float64 statement, and allows the device 4 times that - the rule
of tests/test_bottleneck_gpu.py, for the same reason: sequential multiply-add chains over k ascending on the
matrix cores against the blocked sums of the host's BLAS.  Measured figures are printed (run with -s);
profiles/crepe_errors.txt records them.

Every step on the device runs under its own time limit (`on_device`): a watchdog thread ends the whole process
when the step overruns it - also when the main thread is stuck inside a device call -, so nothing more is
started on a device that hangs.  The statements on the host (most of a test's time) are computed outside the
limit.  Nothing is retried."""

import contextlib
import faulthandler
import os

import numpy as np
import pytest

import crepe_f64 as f64
from test_crepe import END_TO_END_CAPACITIES, left_out, write_weights

pytestmark = pytest.mark.gpu
FACTOR = 4.0
TIME_LIMIT = 120   # seconds per step on the device (the first one loads the code objects)

_CACHE = {}


@contextlib.contextmanager
def on_device(seconds=TIME_LIMIT):
    """The time limit of one step that uses the device (not nested: there is one watchdog)"""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def processor_for(directory, monkeypatch, capacity, seed, **params):
    from shennong_amd.processor import CrepePitchProcessor
    monkeypatch.setenv('SHENNONG_AMD_CREPE_DIR', str(directory))
    write_weights(directory, capacity, seed)
    return CrepePitchProcessor(model_capacity=capacity, **params)


def rounded(weights):
    """The weights as the .npz file holds them (float32), for the statement"""
    return {k: v.astype(np.float32).astype(np.float64) for k, v in weights.items()}


def inputs(audio, audio_8k):
    """name -> 16 kHz int16 samples: the reference's clip, its 8 kHz version resampled, synthetic audio"""
    return {'test.wav': audio.data, 'test.8k.wav': audio_8k.resample(16000).astype(np.int16).data,
            'synthetic': f64.synthetic_signal()}


def statements(capacity, seed, name, samples, hop=160, center=True):
    """(float64 activation, float32 activation) of the statement, computed once per case"""
    key = (capacity, seed, name, hop, center)
    if key not in _CACHE:
        weights = rounded(f64.make_weights(capacity, seed))
        _CACHE[key] = (f64.activation(samples, weights, hop, center),
                       f64.activation(samples, weights, hop, center, dtype=np.float32))
    return _CACHE[key]


def device_activation(proc, samples, hop=160, center=True):
    from shennong_amd.processor import pitch_crepe
    with on_device():
        batch = pitch_crepe.CrepeBatch([samples], hop, center)
        batch.forward(pitch_crepe.device_model(proc.model_capacity, batch.device))
        return batch, batch.host_activation()


@pytest.mark.parametrize('capacity,seed', END_TO_END_CAPACITIES)
def test_activation(gpu, tmp_path, monkeypatch, audio, audio_8k, capacity, seed):
    proc = processor_for(tmp_path, monkeypatch, capacity, seed)
    for name, samples in inputs(audio, audio_8k).items():
        want, low = statements(capacity, seed, name, samples)
        _, got = device_activation(proc, samples)
        assert got.shape == want.shape == (f64.num_frames(len(samples), 160), 360) and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - want).max())
        low_err = float(np.abs(low.astype(np.float64) - want).max())
        print('activation %s %s: device %.3g, float32 numpy %.3g, bound %.3g' % (capacity, name, err, low_err, FACTOR * low_err))
        assert err <= FACTOR * low_err, (capacity, name, err, low_err)


@pytest.mark.parametrize('viterbi', [True, False])
def test_decoder_alone(gpu, audio, viterbi):
    """The statement's own float32 activation through the device decoder"""
    from shennong_amd.processor import pitch_crepe
    capacity, seed = END_TO_END_CAPACITIES[0]
    samples = audio.data
    want64, low = statements(capacity, seed, 'test.wav', samples)
    with on_device():
        batch = pitch_crepe.CrepeBatch([samples], 160, True)
        batch.set_activation(low)
        rows = batch.decode(viterbi)
        first, chosen = batch.host_bins()
    confidence, cents, want_first, want_chosen = f64.decode(low, viterbi)
    np.testing.assert_array_equal(first, want_first)
    np.testing.assert_array_equal(chosen, want_chosen)
    print('decoder viterbi=%s: the path leaves the argmax on %d of %d frames' % (viterbi, (want_chosen != want_first).sum(), len(first)))
    np.testing.assert_array_equal(rows[:, 0], confidence)
    # margin: what the float32 statement's activation error does to the cents of the float64 statement
    _, cents64, _, chosen64 = f64.decode(want64, viterbi)
    same = chosen64 == want_chosen
    margin = float(np.abs(cents64[same] - cents[same]).max())
    got_cents = 1200.0 * np.log2(rows[:, 1] / 10.0)
    err = float(np.abs(got_cents - cents).max())
    print('decoder viterbi=%s: cents device against statement %.3g, float32 margin %.3g' % (viterbi, err, margin))
    assert err <= margin, (err, margin)


@pytest.mark.parametrize('capacity,seed', END_TO_END_CAPACITIES)
def test_end_to_end(gpu, tmp_path, monkeypatch, audio, audio_8k, capacity, seed):
    """(POV, Hz) frame by frame against the float64 statement.  A frame is left out only when the two largest
    bins of its float64 activation lie closer than the measured activation error (a legitimate flip of the
    argmax) or, with the smoothing, when it lies in the run of frames on which such a frame moved the path
    (`left_out`); at most 1 % of the frames.  On every other frame the chosen bin must equal the statement's.
    Bounds: the POV is one activation, so it carries the activation's bound e = 4 x the float32 statement's
    error; the cents are sum(s c) / sum(s) over at most 9 bins that lie within 160 cents of the average, so
    weights that are off by e each move them by at most 9 * 160 e / (sum(s) - 9 e), and a shift of d cents is a
    relative change of d ln 2 / 1200 in Hertz."""
    from shennong_amd import Audio
    for viterbi in (True, False):
        proc = processor_for(tmp_path, monkeypatch, capacity, seed, viterbi=viterbi)
        for name, samples in inputs(audio, audio_8k).items():
            want_act, low = statements(capacity, seed, name, samples)
            batch, got_act = device_activation(proc, samples)
            act_err = float(np.abs(got_act.astype(np.float64) - want_act).max())
            low_err = float(np.abs(low.astype(np.float64) - want_act).max())
            top = np.sort(want_act, axis=1)
            close = (top[:, -1] - top[:, -2]) <= act_err
            low_flips = np.argmax(low, axis=1) != np.argmax(want_act, axis=1)
            assert close.mean() <= 0.01 and low_flips.mean() <= 0.01, (capacity, name, close.sum(), low_flips.sum())
            with on_device():
                got_rows = batch.decode(viterbi)
                got_bins = batch.host_bins()[1]
            _, _, _, want_bins = f64.decode(want_act, viterbi)
            want_rows = f64.raw_rows(want_act, viterbi)
            differ = got_bins != want_bins
            keep = ~left_out(close, differ, viterbi)
            assert keep.mean() >= 0.99, (capacity, name, viterbi, int((~keep).sum()))
            assert not differ[keep].any(), (capacity, name, viterbi, np.flatnonzero(differ & keep))
            e = FACTOR * low_err
            window = np.array([want_act[t, max(0, c - 4):min(360, c + 5)].sum() for t, c in enumerate(want_bins)])
            hz_bound = 9 * 160.0 * e / (window - 9 * e) * np.log(2.0) / 1200.0
            pov_err = float(np.abs(got_rows[keep, 0] - want_rows[keep, 0]).max())
            hz_rel = np.abs(got_rows[keep, 1] / want_rows[keep, 1] - 1.0)
            print('end to end %s %s viterbi=%s: POV %.3g (bound %.3g), Hz relative %.3g (bound %.3g at that frame), '
                  '%d frames left out' % (capacity, name, viterbi, pov_err, e, hz_rel.max(),
                                          hz_bound[keep][np.argmax(hz_rel)], int((~keep).sum())))
            assert pov_err <= e, (pov_err, e)
            assert (hz_rel <= hz_bound[keep]).all()
            # the public class: the same rows brought to the output's row count by the Fourier method
            source = audio_8k if name == 'test.8k.wav' else Audio(samples, 16000)
            with on_device():
                feats = proc.process(source)
            assert feats.shape == (f64.output_rows(len(samples)), 2) and feats.dtype == np.float64
            np.testing.assert_array_equal(feats.data, f64.finish(got_rows.copy(), len(samples)))
            np.testing.assert_array_equal(feats.times, f64.times(feats.shape[0]))
            assert feats.properties == proc.get_properties()


def test_shapes(gpu, tmp_path, monkeypatch, audio):
    from shennong_amd.processor import CrepePitchPostProcessor
    capacity, seed = END_TO_END_CAPACITIES[0]
    proc = processor_for(tmp_path, monkeypatch, capacity, seed, frame_shift=0.01)
    with on_device():
        pitch = proc.process(audio)
    assert pitch.shape == (140, 2) and pitch.dtype == np.float64
    post = CrepePitchPostProcessor()
    with on_device():
        features = post.process(pitch)
    assert features.shape == (140, 3) and np.isfinite(features.data).all()
    assert features.properties['crepe']['crepe postprocessing'] == post.get_params()
    assert features.properties['pipeline'][0]['columns'] == [0, 2]
    for params, rows in (({'center': False}, 140), ({'frame_shift': 0.02}, 70),
                         ({'center': False, 'frame_shift': 0.02, 'viterbi': False}, 70)):
        proc.set_params(**dict({'center': True, 'frame_shift': 0.01, 'viterbi': True}, **params))
        hop = int(16000 * proc.frame_shift)
        want, low = statements(capacity, seed, 'test.wav', audio.data, hop, proc.center)
        batch, got = device_activation(proc, audio.data, hop, proc.center)
        assert got.shape == want.shape == (f64.num_frames(len(audio.data), hop, proc.center), 360)
        err = float(np.abs(got.astype(np.float64) - want).max())
        low_err = float(np.abs(low.astype(np.float64) - want).max())
        print('shapes %s: %d frames, device %.3g, float32 numpy %.3g' % (params, got.shape[0], err, low_err))
        assert err <= FACTOR * low_err, (params, err, low_err)
        with on_device():
            feats = proc.process(audio)
            raw = batch.decode(proc.viterbi)
        assert feats.shape == f64.process(audio.data, rounded(f64.make_weights(capacity, seed)), proc.viterbi,
                                          proc.center, proc.frame_shift, dtype=np.float32).shape == (rows, 2)
        np.testing.assert_array_equal(feats.data, f64.finish(raw, len(audio.data), proc.frame_shift))
        np.testing.assert_array_equal(feats.times, f64.times(rows, proc.frame_shift))


@pytest.mark.parametrize('viterbi', [True, False])
def test_batch_invariance(gpu, tmp_path, monkeypatch, viterbi):
    from shennong_amd import Audio, Utterances
    capacity, seed = END_TO_END_CAPACITIES[0]
    proc = processor_for(tmp_path, monkeypatch, capacity, seed, viterbi=viterbi)
    waves = [f64.synthetic_signal(seed=20 + i, seconds=0.25 + 0.07 * i, f0=110.0 + 23 * i) for i in range(9)]
    assert len({len(w) for w in waves}) == len(waves)
    audios = [Audio(w, 16000) for w in waves]
    with on_device():
        alone = [proc.process(a).data for a in audios]
        together = proc.process_all(Utterances([('utt%d' % i, a) for i, a in enumerate(audios)]))
    assert list(together.keys()) == ['utt%d' % i for i in range(len(waves))]
    for i, want in enumerate(alone):
        assert together['utt%d' % i].shape == want.shape == (f64.output_rows(len(waves[i])), 2)
        np.testing.assert_array_equal(together['utt%d' % i].data, want)
    order = [4, 8, 0, 2]
    with on_device():
        feats = proc._process_batch([audios[i] for i in order])
    for got, i in zip(feats, order):
        np.testing.assert_array_equal(got.data, alone[i])


@pytest.mark.parametrize('l', [1, 2])
def test_one_layer_alone(gpu, l):
    """The convolution kernel through its C entry at the shapes of the full model: block 1 (K = 512 at stride 4,
    N = 1024) and block 2 (K = 65 536, N = 128), on a few frames.

    Block 2 is the case the kernel's summation order answers to: chains of 256 consecutive k whose results are
    added in ascending order (256 of them here), where the statement adds 64 BLAS products of K = 1024.  The
    bound is the rule of the module's docstring; profiles/crepe_errors.txt holds the measured figures."""
    from shennong_amd.processor import pitch_crepe
    rng = np.random.RandomState(8)
    c1, c2 = f64.filters('full')[:2]
    weights = {k: v.astype(np.float32).astype(np.float64) for k, v in f64.make_weights('full', 5).items()
               if k.startswith(('conv1', 'conv2'))}
    cases = [(1, rng.randn(3, 1024, 1)), (2, np.abs(rng.randn(3, 128, c1)) * (rng.uniform(size=(3, 128, c1)) < 0.5))]
    cases = [case for case in cases if case[0] == l]
    for l, x in cases:
        x = x.astype(np.float32)
        want = f64.block(x.astype(np.float64), weights, l)
        low = f64.block(x, weights, l, np.float32)
        name = 'conv%d-BN/' % l
        scale = weights[name + 'gamma'] / np.sqrt(weights[name + 'moving_variance'] + 1e-3)
        shift = weights[name + 'beta'] - weights[name + 'moving_mean'] * scale
        k = weights['conv%d/kernel' % l]
        with on_device():
            got = pitch_crepe.conv_layer(x, k.reshape(k.shape[0], k.shape[2], k.shape[3]), weights['conv%d/bias' % l],
                                         scale, shift, stride=f64.STRIDES[l - 1], pad_left=254 if l == 1 else 31)
        assert got.shape == want.shape == (3, (256, 128)[l - 1] // 2, (c1, c2)[l - 1]) and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - want).max())
        low_err = float(np.abs(low.astype(np.float64) - want).max())
        print('full block %d: device %.3g, float32 numpy %.3g, bound %.3g' % (l, err, low_err, FACTOR * low_err))
        assert err <= FACTOR * low_err, (l, err, low_err)
        # a frame alone gives the bits it has in the block
        with on_device():
            alone = pitch_crepe.conv_layer(x[1:2], k.reshape(k.shape[0], k.shape[2], k.shape[3]),
                                           weights['conv%d/bias' % l], scale, shift, stride=f64.STRIDES[l - 1],
                                           pad_left=254 if l == 1 else 31)
        np.testing.assert_array_equal(alone[0], got[1])


def test_invalid(gpu, monkeypatch):
    L, ptr = gpu.lib(), 256
    assert L.snf_crepe_conv(0, ptr, -1, 128, 4, 64, 1, 31, 128, ptr, ptr, ptr, ptr, 4, 3, ptr, None) == -1
    assert L.snf_crepe_conv(0, ptr, 1, 128, 4, 64, 1, 31, 127, ptr, ptr, ptr, ptr, 4, 3, ptr, None) == -1
    assert L.snf_crepe_conv(0, ptr, 1, 128, 4, 64, 1, 31, 128, ptr, ptr, None, ptr, 4, 1, ptr, None) == -1
    assert L.snf_crepe_conv(0, ptr, 1, 128, 4, 64, 1, 31, 128, ptr, ptr, ptr, ptr, 4, 8, ptr, None) == -1
    assert L.snf_crepe_conv(0, ptr, 1, 128, 4, 64, 1, 31, 130, ptr, ptr, ptr, ptr, 4, 3, ptr, None) == -1
    assert L.snf_crepe_conv(0, ptr, 1, 1024, 1, 512, 4, 254, 258, ptr, ptr, ptr, ptr, 4, 3, ptr, None) == -1
    from shennong_amd import Audio
    from shennong_amd.processor import CrepePitchProcessor
    monkeypatch.delenv('SHENNONG_AMD_CREPE_DIR', raising=False)
    with pytest.raises(RuntimeError, match='file not found'):
        CrepePitchProcessor('large').process(Audio(np.zeros(4000, dtype=np.int16), 16000))
