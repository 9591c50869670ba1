"""CrepePitchProcessor without a device: parameters and messages (reference test/test_processor_pitch_crepe.py
territory), the weights loader, and tests/crepe_f64.py pinned against third parties: every convolution against
scipy.signal.correlate with explicit padding, the pool against a reshape, the Viterbi decoder against a
brute-force dynamic programme, the cents mapping and the local average against hand-computed cases."""

import os

import numpy as np
import pytest
import scipy.signal

import crepe_f64 as f64
from shennong_amd import Audio
from shennong_amd.processor import CrepePitchPostProcessor, CrepePitchProcessor
from shennong_amd.processor import pitch_crepe

# the inputs of the end-to-end GPU checks: (name, seed of the weights); test.wav and test.8k.wav come on top
END_TO_END_CAPACITIES = [('tiny', 11), ('medium', 12)]


def write_weights(directory, capacity, seed, **replace):
    weights = f64.make_weights(capacity, seed)
    weights.update(replace)
    os.makedirs(str(directory), exist_ok=True)
    path = os.path.join(str(directory), 'model-%s.npz' % capacity)
    np.savez(path, **{k: v.astype(np.float32) for k, v in weights.items()})
    return path


def left_out(close, differ, viterbi):
    """The frames the end-to-end check may leave out: those whose two largest float64 bins lie closer than the
    measured activation error (`close`), and, with the smoothing, the run of consecutive frames around such a
    frame on which the two paths part (`differ`): between two frames where the paths agree, and with the same
    observations in between, both are the best path between the same end points, so a run of differing frames
    without a close frame in it is not explained by a flip and is kept (and fails the comparison)."""
    out = close.copy()
    if not viterbi:
        return out
    t, n = 0, len(close)
    while t < n:
        e = t + 1
        if differ[t]:
            while e < n and differ[e]:
                e += 1
            if close[t:e].any():
                out[t:e] = True
        t = e
    return out


def test_left_out():
    close = np.zeros(12, dtype=bool)
    differ = np.zeros(12, dtype=bool)
    close[3] = True
    differ[2:5] = True      # a run around the close frame
    differ[8:10] = True     # a run that no close frame explains
    np.testing.assert_array_equal(np.flatnonzero(left_out(close, differ, True)), [2, 3, 4])
    np.testing.assert_array_equal(np.flatnonzero(left_out(close, differ, False)), [3])
    close[11] = True        # a close frame that did not flip is left out all the same
    np.testing.assert_array_equal(np.flatnonzero(left_out(close, differ, True)), [2, 3, 4, 11])
    assert not left_out(np.zeros(5, dtype=bool), np.ones(5, dtype=bool), True).any()


def test_params():
    assert CrepePitchProcessor().get_params() == {
        'model_capacity': 'full', 'viterbi': True, 'center': True, 'frame_shift': 0.01, 'frame_length': 0.025}
    params = {'model_capacity': 'tiny', 'viterbi': False, 'center': False, 'frame_shift': 0.02, 'frame_length': 0.05}
    proc = CrepePitchProcessor(**params)
    assert proc.get_params() == params
    other = CrepePitchProcessor()
    other.set_params(**params)
    assert other.get_params() == params
    assert proc.name == 'crepe' and proc.ndims == 2 and proc.sample_rate == 16000
    np.testing.assert_array_equal(proc.times(3), [[0.0, 0.05], [0.02, 0.07], [0.04, 0.09]])
    assert proc.get_properties() == {'pipeline': [{'name': 'crepe', 'columns': [0, 1]}], 'crepe': params}
    proc.viterbi = 0
    proc.center = 'yes'
    assert proc.viterbi is False and proc.center is True


def test_post_params():
    post = CrepePitchPostProcessor()
    assert post.name == 'crepe postprocessing' and post.ndims == 3
    params = post.get_params()
    assert sorted(params) == sorted([
        'pitch_scale', 'delta_pitch_scale', 'delta_pitch_noise_stddev', 'normalization_left_context',
        'normalization_right_context', 'delta_window', 'delay', 'add_pov_feature', 'add_normalized_log_pitch',
        'add_delta_pitch', 'add_raw_log_pitch'])
    assert params['pitch_scale'] == 2.0 and params['delta_pitch_scale'] == 10.0 and params['delay'] == 0
    assert params['normalization_left_context'] == 75 and params['add_raw_log_pitch'] is False
    post.add_raw_log_pitch = True
    assert post.ndims == 4


def test_errors():
    with pytest.raises(ValueError) as err:
        CrepePitchProcessor(model_capacity='huge')
    assert str(err.value) == 'Model capacity huge is not recognized.'
    with pytest.raises(ValueError, match='Model capacity 4 is not recognized'):
        CrepePitchProcessor(model_capacity=4)
    proc = CrepePitchProcessor(model_capacity='tiny')
    stereo = Audio(np.zeros((2000, 2), dtype=np.int16), 16000)
    with pytest.raises(ValueError) as err:
        proc.process(stereo)
    assert str(err.value) == 'audio must have one channel but has 2'
    from shennong_amd.features import Features
    post = CrepePitchPostProcessor()
    with pytest.raises(ValueError, match=r'data shape must be \(_, 2\), but it is \(_, 3\)'):
        post.process(Features(np.ones((5, 3)), f64.times(5), {'crepe': {}, 'pipeline': [{}]}))
    none = CrepePitchPostProcessor(add_pov_feature=False, add_normalized_log_pitch=False, add_delta_pitch=False)
    with pytest.raises(ValueError, match='at least one of the following options must be True'):
        none.process(Features(np.ones((5, 2)), f64.times(5), {'crepe': {}, 'pipeline': [{}]}))
    with pytest.raises(ValueError, match='No voiced frames'):
        post.process(Features(np.zeros((5, 2)), f64.times(5), {'crepe': {}, 'pipeline': [{}]}))


def test_weights_loader(tmp_path, monkeypatch):
    monkeypatch.setenv(pitch_crepe.ENV_DIR, str(tmp_path / 'nowhere'))
    with pytest.raises(RuntimeError) as err:
        pitch_crepe.load_model('tiny')
    assert str(err.value) == 'file not found: ' + os.path.join(str(tmp_path / 'nowhere'), 'model-tiny.npz')
    monkeypatch.setenv(pitch_crepe.ENV_DIR, str(tmp_path))
    path = write_weights(tmp_path, 'tiny', 1)
    (capacity, found), params = pitch_crepe.load_model('tiny')
    assert capacity == 'tiny' and found == path and len(params) == 26
    c = f64.filters('tiny')
    assert [p.shape for p in params[:4]] == [(512, c[0]), (c[0],), (c[0],), (c[0],)]
    assert params[4].shape == (64 * c[0], c[1]) and params[24].shape == (4 * c[5], 360) and params[25].shape == (360,)
    assert all(p.dtype == np.float32 and p.flags.c_contiguous for p in params)
    w = f64.make_weights('tiny', 1)
    scale = w['conv3-BN/gamma'].astype(np.float32).astype(np.float64) / np.sqrt(
        w['conv3-BN/moving_variance'].astype(np.float32).astype(np.float64) + 1e-3)
    np.testing.assert_allclose(params[4 * 2 + 2], scale, rtol=1e-6)
    assert (params[4 * 2 + 2] < 0).any() and (params[4 * 2 + 2] > 0).any()
    # the tiny file is not the small model
    os.replace(path, os.path.join(str(tmp_path), 'model-small.npz'))
    with pytest.raises(ValueError, match=r'array "conv1/kernel" has shape \(512, 1, 1, 128\), expected \(512, 1, 1, 256\)'):
        pitch_crepe.load_model('small')
    bad = write_weights(tmp_path / 'bad', 'tiny', 1, **{'classifier/bias': np.zeros(359)})
    with pytest.raises(ValueError, match=r'array "classifier/bias" has shape \(359,\), expected \(360,\)'):
        pitch_crepe.load_model('tiny', bad)
    weights = f64.make_weights('tiny', 1)
    del weights['conv2-BN/beta']
    os.makedirs(str(tmp_path / 'short'))
    np.savez(os.path.join(str(tmp_path / 'short'), 'model-tiny.npz'), **weights)
    with pytest.raises(ValueError, match='missing arrays conv2-BN/beta'):
        pitch_crepe.load_model('tiny', os.path.join(str(tmp_path / 'short'), 'model-tiny.npz'))


def test_expected_shapes_full():
    shapes = pitch_crepe.expected_shapes('full')
    assert shapes['conv1/kernel'] == (512, 1, 1, 1024) and shapes['conv2/kernel'] == (64, 1, 1024, 128)
    assert shapes['conv6/kernel'] == (64, 1, 256, 512) and shapes['classifier/kernel'] == (2048, 360)
    assert len(shapes) == 38
    assert [pitch_crepe.filters(c)[0] for c in ('tiny', 'small', 'medium', 'large', 'full')] == [128, 256, 512, 768, 1024]


@pytest.mark.parametrize('length,c_in,c_out,width,stride,before,after', [
    (1024, 1, 5, 512, 4, 254, 254), (128, 6, 4, 64, 1, 31, 32), (8, 3, 7, 64, 1, 31, 32)])
def test_conv_against_scipy(length, c_in, c_out, width, stride, before, after):
    rng = np.random.RandomState(length)
    x = rng.randn(2, length, c_in)
    kernel = rng.randn(width, c_in, c_out)
    assert f64.same_padding(length, width, stride) == (-(-length // stride), before, after)
    got = f64.conv(x, kernel, stride)
    xp = np.pad(x, ((0, 0), (before, after), (0, 0)))
    for f in range(2):
        for o in range(c_out):
            want = sum(scipy.signal.correlate(xp[f, :, i], kernel[:, i, o], mode='valid')[::stride] for i in range(c_in))
            np.testing.assert_allclose(got[f, :, o], want, rtol=1e-10, atol=1e-10)
    low = f64.conv(x, kernel, stride, np.float32)
    assert low.dtype == np.float32
    np.testing.assert_allclose(low, got, rtol=1e-3, atol=1e-3)


def test_pool_and_block():
    rng = np.random.RandomState(2)
    x = rng.randn(3, 8, 5)
    want = np.maximum(x[:, 0::2, :], x[:, 1::2, :])
    np.testing.assert_array_equal(f64.pool(x), want)
    # a negative scale flips the order inside a pair: the normalisation cannot move behind the pool
    w = f64.make_weights('tiny', 4)
    frames = rng.randn(2, 1024, 1)
    y = f64.block(frames, w, 1)
    assert y.shape == (2, 128, 128)
    k = w['conv1/kernel']
    z = np.maximum(f64.conv(frames, k.reshape(512, 1, 128), 4) + w['conv1/bias'], 0)
    z = (z - w['conv1-BN/moving_mean']) / np.sqrt(w['conv1-BN/moving_variance'] + 1e-3) * w['conv1-BN/gamma'] \
        + w['conv1-BN/beta']
    np.testing.assert_allclose(y, z.reshape(2, 128, 2, 128).max(axis=2), rtol=1e-12, atol=1e-12)
    assert (w['conv1-BN/gamma'] < 0).any() and (w['conv1-BN/gamma'] > 0).any()
    assert (w['conv1-BN/moving_variance'] > 0).all()


def test_framing():
    samples = f64.synthetic_signal(seconds=0.3)
    frames = f64.frames_of(samples, 160, True)
    assert frames.shape == (1 + len(samples) // 160, 1024) == (f64.num_frames(len(samples), 160), 1024)
    np.testing.assert_allclose(frames.mean(axis=1), 0, atol=1e-12)
    np.testing.assert_allclose(frames.std(axis=1), 1, rtol=1e-12)
    padded = np.pad(samples.astype(np.float64), 512)
    want = padded[320:320 + 1024]
    np.testing.assert_allclose(frames[2], (want - want.mean()) / want.std(), rtol=1e-12, atol=1e-12)
    assert f64.frames_of(samples, 320, False).shape == (1 + (len(samples) - 1024) // 320, 1024)
    assert np.array_equal(f64.frames_of(np.zeros(2048, np.int16), 160, False), np.zeros((7, 1024)))   # the floor
    assert pitch_crepe.num_frames(22713, 160, True) == f64.num_frames(22713, 160, True) == 142
    assert pitch_crepe.num_frames(22713, 160, False) == f64.num_frames(22713, 160, False) == 136
    assert f64.output_rows(22713) == 140 and CrepePitchProcessor('tiny')._output_rows(22713) == 140


def test_cents():
    assert f64.CENTS[0] == 1997.3794084376191 and abs(f64.CENTS[1] - f64.CENTS[0] - 20.0) < 1e-9
    assert abs(f64.CENTS[-1] - (7180 + 1997.3794084376191)) < 1e-9
    np.testing.assert_array_equal(pitch_crepe.cents_mapping(), f64.CENTS)
    s = np.zeros(360)
    s[100] = 1.0
    assert abs(f64.local_average_cents(s, 100) - f64.CENTS[100]) < 1e-9
    s[101] = 1.0   # two equal bins: half way
    assert abs(f64.local_average_cents(s, 100) - (f64.CENTS[100] + 10.0)) < 1e-9
    s[105] = 5.0   # outside [96, 105)
    assert abs(f64.local_average_cents(s, 100) - (f64.CENTS[100] + 10.0)) < 1e-9
    s[104] = 2.0   # inside: (c + c + 20 + 2 (c + 80)) / 4 = c + 45
    assert abs(f64.local_average_cents(s, 100) - (f64.CENTS[100] + 45.0)) < 1e-9
    edge = np.ones(360)   # clipped windows: bins 0..5 around 1, bins 354..359 around 358
    assert abs(f64.local_average_cents(edge, 1) - (f64.CENTS[0] + 50.0)) < 1e-9
    assert abs(f64.local_average_cents(edge, 358) - (f64.CENTS[359] - 50.0)) < 1e-9
    # 10 * 2^(cents / 1200): bin 0 is C1 = 32.70 Hz, 1200 cents above it twice that
    hz = f64.hertz(np.array([f64.CENTS[0], f64.CENTS[60], np.nan]))
    assert abs(hz[0] - 31.70) < 0.01 and abs(hz[1] / hz[0] - 2.0) < 1e-9 and hz[2] == 0


def brute_force_viterbi(obs):
    """O(S^2) per frame float64 dynamic programme over explicit probabilities; also returns the smallest gap
    between the best and the second best candidate met along the chosen path"""
    S = 360
    start = np.full(S, 1.0 / S)
    trans = np.array([[max(12 - abs(i - j), 0) for j in range(S)] for i in range(S)], dtype=np.float64)
    trans /= trans.sum(axis=1, keepdims=True)
    emit = np.full((S, S), 0.9 / S) + 0.1 * np.eye(S)
    with np.errstate(divide='ignore'):
        ls, lt, le = np.log(start), np.log(trans), np.log(emit)
    score = [ls[j] + le[j, obs[0]] for j in range(S)]
    back = []
    for o in obs[1:]:
        new, arg = [], []
        for j in range(S):
            best, who = -np.inf, 0
            for i in range(S):
                v = score[i] + lt[i, j]
                if v > best:
                    best, who = v, i
            new.append(best + le[j, o])
            arg.append(who)
        back.append((arg, score))
        score = new
    state = max(range(S), key=lambda j: (score[j], -j))
    gaps = [np.sort(score)[-1] - np.sort(score)[-2]]
    path = [state]
    for arg, prev in reversed(back):
        cand = np.array([prev[i] + lt[i, path[-1]] for i in range(S)])
        gaps.append(np.sort(cand)[-1] - np.sort(cand)[-2])
        path.append(arg[path[-1]])
    return np.array(path[::-1]), min(gaps)


@pytest.mark.parametrize('seed', [0, 1])
def test_viterbi_against_brute_force(seed):
    rng = np.random.RandomState(seed)
    n, outliers = 30, [5, 12, 20, 26]
    steps = rng.randint(-3, 4, n)
    for t in outliers:      # the track rests around an outlier: between two DIFFERENT neighbours the model itself
        steps[t] = steps[t + 1] = 0   # ties (the states on either side of the middle score the same)
    walk = 180 + np.cumsum(steps)
    obs = walk.copy()
    obs[outliers] = (walk[outliers] + 100 + rng.randint(0, 100, len(outliers))) % 360
    want, gap = brute_force_viterbi([int(o) for o in obs])
    assert gap > 1e-9    # no exact tie on the chosen path: the path does not hang on the tie rule
    got = f64.viterbi_path(obs)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, walk)   # outliers are smoothed away, the track is kept
    # the band of +-11 states of the device's tables holds every transition the model allows
    tables = pitch_crepe.decoder_tables()
    band = tables[:360 * 23].reshape(360, 23)
    _, transition, emission = f64.hmm_tables()
    for j in (0, 5, 11, 180, 348, 359):
        for d in range(23):
            i = j - 11 + d
            assert band[j, d] == (transition[i, j] if 0 <= i < 360 else -np.inf)
    assert np.isinf(transition[0, 12]) and np.isfinite(transition[0, 11])
    assert tables[360 * 23] == np.log(1.0 / 360) and tables[360 * 23 + 1] == emission[7, 7]
    assert tables[360 * 23 + 2] == emission[7, 8] and len(tables) == 360 * 23 + 3 + 360


def test_voicing_and_post_conversion():
    conf = np.concatenate([np.full(30, 0.05), np.full(40, 0.9), [0.1], np.full(40, 0.85), np.full(30, 0.02)])
    want = np.concatenate([np.zeros(30), np.ones(81), np.zeros(30)]).astype(int)   # the dip is bridged
    np.testing.assert_array_equal(f64.voicing(conf), want)
    np.testing.assert_array_equal(pitch_crepe.predict_voicing(conf), want)
    rng = np.random.RandomState(3)
    noisy = np.clip(conf + 0.2 * rng.randn(len(conf)), 0, 1)
    np.testing.assert_array_equal(pitch_crepe.predict_voicing(noisy), f64.voicing(noisy))
    # POV -> NCCF against scipy's bisection of the same map
    import scipy.optimize
    pov = np.array([0.0, 1.0, 0.02, 0.3, 0.77, 0.999])
    nccf = pitch_crepe.pov_to_nccf(pov)
    assert nccf[0] == 0 and nccf[1] == 1
    for p, x in zip(pov[2:], nccf[2:]):
        assert abs(x - scipy.optimize.bisect(lambda v: pitch_crepe._nccf_to_pov(v) - p, 0, 1)) < 1e-11
    with pytest.raises(ValueError):
        pitch_crepe.pov_to_nccf(np.array([1e-5]))


def end_to_end_inputs(wave):
    """name -> 16 kHz int16 samples of the end-to-end checks: the reference's clip, its 8 kHz version resampled,
    synthetic audio"""
    clip = Audio.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'test.8k.wav'))
    return {'test.wav': wave, 'test.8k.wav': clip.resample(16000).astype(np.int16).data,
            'synthetic': f64.synthetic_signal()}


@pytest.mark.parametrize('capacity,seed', END_TO_END_CAPACITIES)
def test_float32_statement_keeps_the_argmax(capacity, seed, wave):
    """The inputs of the GPU end-to-end check are chosen so that float32 arithmetic alone moves at most 1 % of
    the frames' argmax: asserted here, for every capacity and input of that check, on the float32 numpy
    statement against the float64 one"""
    weights = {k: v.astype(np.float32).astype(np.float64) for k, v in f64.make_weights(capacity, seed).items()}
    for name, samples in end_to_end_inputs(wave).items():
        hi = f64.activation(samples, weights)
        lo = f64.activation(samples, weights, dtype=np.float32)
        assert lo.dtype == np.float32 and hi.shape == lo.shape == (f64.num_frames(len(samples), 160), 360)
        err = float(np.abs(lo.astype(np.float64) - hi).max())
        top = np.sort(hi, axis=1)
        close = (top[:, -1] - top[:, -2]) <= err
        flips = np.argmax(hi, axis=1) != np.argmax(lo, axis=1)
        print('%s %s: float32 error %.3g, %d close frames, %d flips of %d' % (capacity, name, err, close.sum(), flips.sum(), len(hi)))
        assert close.mean() <= 0.01 and flips.mean() <= 0.01 and not (flips & ~close).any()
        assert 0.05 < hi.max() and hi.std() > 1e-3   # the sigmoids are neither saturated nor flat
        for viterbi in (True, False):   # and the decoded bins: left out as the GPU check leaves out
            bins = f64.decode(hi, viterbi)[3]
            differ = f64.decode(lo, viterbi)[3] != bins
            out = left_out(close, differ, viterbi)
            assert out.mean() <= 0.01 and not (differ & ~out).any(), (capacity, name, viterbi)
        rows = f64.process(samples, weights)
        assert rows.shape == (f64.output_rows(len(samples)), 2)
        assert np.isfinite(rows).all()
