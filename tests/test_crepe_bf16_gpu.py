"""The bfloat16 matrix-core path of the CREPE network (``precision='bfloat16'``) on the device: one block alone,
the rounding, the whole network against the float64 statement of tests/crepe_f64.py, the decoders behind it,
batch invariance, switching between the precisions and the new entry points' validation.

Bounds.  One block alone: the operands are rounded to bfloat16 beforehand for the statement, so every product is
exact in float32 and the float32 numpy result differs from the float64 one by its summation (and epilogue)
only; the device, which gets the unrounded operands and rounds them itself, may err 4 times that - the rule of
tests/test_crepe_gpu.py.  A truncation or any other rounding on the device would err by about 1e-3 against
about 1e-6.  The network: the test evaluates the numpy statement of the contract (tests/crepe_bf16.py) in float32
on the same input, takes its largest absolute error against the float64 statement (unquantised), and allows the
device 4 times that, never more than 2e-2 (the ceiling of tests/test_bottleneck_bf16.py).  Both errors are the
same quantisation (about 2.3e-3), so the ratio is near 1; float32 round-off flips bfloat16 roundings downstream,
so no whole-network assertion compares the device with a contract evaluation more tightly.

Every step on the device runs under `on_device` of tests/test_crepe_gpu.py; nothing is retried.  Measured figures
are printed (run with -s); profiles/crepe_bf16_errors.txt records them."""

import ctypes as C

import numpy as np
import pytest

import crepe_f64 as f64
from bottleneck_bf16 import bf16
from test_crepe import END_TO_END_CAPACITIES, left_out
from test_crepe_bf16 import END_TO_END_BF16, contract_statement
from test_crepe_gpu import FACTOR, inputs, on_device, processor_for, statements

pytestmark = pytest.mark.gpu
CEILING = 2e-2

# frames, length, C_in, C_out, width, stride, pad_left, norm, pool, sigmoid
LAYERS = [
    (1, 10, 8, 5, 3, 1, 1, True, False, False),            # K = 24, under one k tile; N under one fragment
    (2, 9, 8, 40, 3, 2, 1, True, False, False),            # stride 2
    (3, 128, 1024, 128, 64, 1, 31, True, True, False),     # block 2 of `full`: K = 65 536, three M tiles, 64 chains
    (3, 64, 16, 16, 64, 1, 31, True, True, False),         # M = 192, a partial M tile; N = 16
    (5, 8, 32, 64, 64, 1, 31, True, True, False),          # M = 40, more padding than data
    (4, 1, 256, 360, 1, 1, 0, False, False, True)]         # classifier-shaped: N = 360 with a partial N tile


def layer_weights(case):
    """Weights of one block under the names of block 2, drawn as tests/crepe_f64.py draws them, float32 values"""
    frames, length, c_in, c_out, width, stride, pad_left, norm, pool, sigmoid = case
    if (c_in, c_out, width) == (1024, 128, 64):
        w = {k: v for k, v in f64.make_weights('full', 5).items() if k.startswith('conv2')}
    else:
        rng = np.random.RandomState(c_in + c_out)
        spread = 3.0 * np.sqrt(3.0 / (width * c_in)) if sigmoid else np.sqrt(6.0 / (width * c_in))
        w = {'conv2/kernel': rng.uniform(-1.0, 1.0, (width, 1, c_in, c_out)) * spread,
             'conv2/bias': rng.uniform(-0.5, 0.5, c_out) - 2.0 if sigmoid else rng.uniform(-0.1, 0.1, c_out),
             'conv2-BN/gamma': rng.uniform(0.5, 1.5, c_out) * np.where(rng.uniform(size=c_out) < 0.3, -1.0, 1.0),
             'conv2-BN/beta': rng.uniform(-0.2, 0.2, c_out), 'conv2-BN/moving_mean': rng.uniform(0.2, 0.6, c_out),
             'conv2-BN/moving_variance': rng.uniform(0.5, 1.5, c_out)}
    return {k: v.astype(np.float32).astype(np.float64) for k, v in w.items()}


def layer_statement(x, w, case, dtype):
    """The block in `dtype` numpy: f64.block where the case is a block of the network, else its parts"""
    stride, norm, pool, sigmoid = case[5], case[7], case[8], case[9]
    if norm and pool and stride == 1:
        return f64.block(x.astype(dtype), w, 2, dtype)
    k = w['conv2/kernel']
    y = f64.conv(x, k.reshape(k.shape[0], k.shape[2], k.shape[3]), stride, dtype) + w['conv2/bias'].astype(dtype)
    if norm:
        g, b, m, v = (w['conv2-BN/' + n].astype(dtype) for n in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
        y = (np.maximum(y, dtype(0)) - m) / np.sqrt(v + dtype(f64.EPSILON)) * g + b
    if pool:
        y = f64.pool(y)
    return (f64.sigmoid(y) if sigmoid else y).astype(dtype)


@pytest.mark.parametrize('case', LAYERS, ids=lambda c: 'x'.join(str(v) for v in c[:7]))
def test_layer_alone(gpu, case):
    from shennong_amd.processor import pitch_crepe
    frames, length, c_in, c_out, width, stride, pad_left, norm, pool, sigmoid = case
    rng = np.random.RandomState(8)
    w = layer_weights(case)
    x = (np.abs(rng.randn(frames, length, c_in)) * (rng.uniform(size=(frames, length, c_in)) < 0.5)).astype(np.float32)
    assert not np.array_equal(bf16(x), x) and not np.array_equal(bf16(w['conv2/kernel']), w['conv2/kernel'])
    wq = dict(w, **{'conv2/kernel': bf16(w['conv2/kernel']).astype(np.float64)})
    want = layer_statement(bf16(x).astype(np.float64), wq, case, np.float64)
    low = layer_statement(bf16(x), wq, case, np.float32)
    scale = w['conv2-BN/gamma'] / np.sqrt(w['conv2-BN/moving_variance'] + 1e-3)
    shift = w['conv2-BN/beta'] - w['conv2-BN/moving_mean'] * scale
    kernel = w['conv2/kernel'].reshape(width, c_in, c_out)

    def run(x, **how):
        with on_device():
            return pitch_crepe.conv_layer(x, kernel, w['conv2/bias'], scale if norm else None, shift if norm else None,
                                          stride=stride, pad_left=pad_left, pool=pool, sigmoid=sigmoid,
                                          precision='bfloat16', **how)

    got = run(x)
    assert got.shape == want.shape and got.dtype == low.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want).max())
    low_err = float(np.abs(low.astype(np.float64) - want).max())
    print('layer %s: device %.3g, float32 numpy %.3g, bound %.3g' % (case[:7], err, low_err, FACTOR * low_err))
    assert err <= FACTOR * low_err, (case, err, low_err)
    # a source rounded beforehand and stored as bfloat16 gives the same bits as the loader's own rounding
    np.testing.assert_array_equal(run(bf16(x), source='bfloat16').view(np.uint32), got.view(np.uint32))
    # a frame alone gives the bits it has in the block
    f = frames // 2
    np.testing.assert_array_equal(run(x[f:f + 1])[0].view(np.uint32), got[f].view(np.uint32))


def test_rounding_on_device(gpu):
    """Through the identity kernel (width 1, 8 channels, no bias, no normalisation, no pool) an output is its
    input's rounding times 1 plus zeros: it equals bf16(x) bit for bit, stored as float32 and, widened, stored as
    bfloat16.  Where bf16(x) is a zero the sign is not compared: a sum that starts from +0 is +0."""
    from shennong_amd.processor import pitch_crepe
    top = np.array([0x7F7F0000, 0x7F7F7FFF, 0xFF7F0000, 0xFF7F7FFF], dtype=np.uint32).view(np.float32)   # +-max
    values = np.array([1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3.0 * 2.0 ** -8),     # ties
                       1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20, -(1.0 + 3.0 * 2.0 ** -8 + 2.0 ** -20),
                       -(1.0 + 3.0 * 2.0 ** -8 - 2.0 ** -20), 2.0 - 2.0 ** -9, 0.5 + 2.0 ** -9, -0.3, 255.0,
                       2.0 ** -126 * (1.0 + 2.0 ** -8), 2.0 ** -126 * 1.37, -2.0 ** -125 * (1.0 + 3.0 * 2.0 ** -8),
                       2.0 ** -133, 1.5 * 2.0 ** -133, -2.5 * 2.0 ** -133, 2.0 ** -130 * 1.37, -2.0 ** -128 * 1.9,  # subnormals
                       2.0 ** -149, -2.0 ** -140, 0.0, -0.0], dtype=np.float32)
    x = np.concatenate([values, top, np.random.RandomState(4).uniform(-2.0, 2.0, 20).astype(np.float32)])
    assert x.size == 48
    x = x.reshape(2, 3, 8)
    want = bf16(x)
    assert not np.array_equal(want, x) and np.isfinite(want).all()
    identity = np.eye(8, dtype=np.float32)[None]
    for store in ('float32', 'bfloat16'):
        with on_device():
            got = pitch_crepe.conv_layer(x, identity, np.zeros(8, np.float32), pad_left=0, pool=False,
                                         precision='bfloat16', store=store)
        assert got.shape == x.shape and got.dtype == np.float32
        differ = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(-1) & (want != 0).reshape(-1))
        print('rounding, %s store: %d of %d values differ %s' % (store, differ.size, x.size, x.reshape(-1)[differ]))
        assert differ.size == 0, (store, x.reshape(-1)[differ], got.reshape(-1)[differ], want.reshape(-1)[differ])
        np.testing.assert_array_equal(got, want)      # (the zeros, either sign)


def device_activation(proc, samples):
    from shennong_amd.processor import pitch_crepe
    with on_device():
        batch = pitch_crepe.CrepeBatch([samples], 160, True)
        batch.forward(pitch_crepe.device_model(proc.model_capacity, batch.device), precision='bfloat16')
        return batch, batch.host_activation()


@pytest.mark.parametrize('capacity,seed', END_TO_END_CAPACITIES)
def test_activation(gpu, tmp_path, monkeypatch, audio, audio_8k, capacity, seed):
    proc = processor_for(tmp_path, monkeypatch, capacity, seed)
    for name, samples in inputs(audio, audio_8k).items():
        want, _ = statements(capacity, seed, name, samples)
        low = contract_statement(capacity, seed, name, samples)
        _, got = device_activation(proc, samples)
        assert got.shape == want.shape == (f64.num_frames(len(samples), 160), 360) and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - want).max())
        low_err = float(np.abs(low.astype(np.float64) - want).max())
        print('activation bfloat16 %s %s: device %.3g, float32 numpy contract %.3g, bound %.3g'
              % (capacity, name, err, low_err, min(FACTOR * low_err, CEILING)))
        assert err <= FACTOR * low_err and err <= CEILING, (capacity, name, err, low_err)


def test_end_to_end(gpu, tmp_path, monkeypatch, audio, audio_8k):
    """(POV, Hz) frame by frame as tests/test_crepe_gpu.py checks the float32 path, with e = the activation bound
    above; first the decoder, which is unchanged and exact: the float64 decoder of the statement on the device's
    own activation gives the device's bins, its POV bit for bit and its cents."""
    from shennong_amd import Audio
    capacity, seed = END_TO_END_BF16
    for viterbi in (True, False):
        proc = processor_for(tmp_path, monkeypatch, capacity, seed, viterbi=viterbi)
        proc.precision = 'bfloat16'
        for name, samples in inputs(audio, audio_8k).items():
            want_act, _ = statements(capacity, seed, name, samples)
            low = contract_statement(capacity, seed, name, samples)
            batch, got_act = device_activation(proc, samples)
            act_err = float(np.abs(got_act.astype(np.float64) - want_act).max())
            e = min(FACTOR * float(np.abs(low.astype(np.float64) - want_act).max()), CEILING)
            assert act_err <= e, (name, act_err, e)
            with on_device():
                got_rows = batch.decode(viterbi)
                got_first, got_bins = batch.host_bins()
            confidence, cents, first, chosen = f64.decode(got_act, viterbi)
            np.testing.assert_array_equal(got_first, first)
            np.testing.assert_array_equal(got_bins, chosen)
            np.testing.assert_array_equal(got_rows[:, 0], confidence)
            _, want_cents, _, want_bins = f64.decode(want_act, viterbi)
            same = want_bins == chosen
            margin = float(np.abs(want_cents[same] - cents[same]).max())
            cents_err = float(np.abs(1200.0 * np.log2(got_rows[:, 1] / 10.0) - cents).max())
            assert cents_err <= margin, (cents_err, margin)
            # against the float64 statement
            top = np.sort(want_act, axis=1)
            close = (top[:, -1] - top[:, -2]) <= act_err
            differ = got_bins != want_bins
            keep = ~left_out(close, differ, viterbi)
            assert keep.mean() >= 0.99, (name, viterbi, int((~keep).sum()))
            assert not differ[keep].any(), (name, viterbi, np.flatnonzero(differ & keep))
            want_rows = f64.raw_rows(want_act, viterbi)
            window = np.array([want_act[t, max(0, c - 4):min(360, c + 5)].sum() for t, c in enumerate(want_bins)])
            with np.errstate(divide='ignore'):   # (no bound where 9 e reaches the window's sum)
                hz_bound = np.where(window > 9 * e, 9 * 160.0 * e / (window - 9 * e) * np.log(2.0) / 1200.0, np.inf)
            pov_err = float(np.abs(got_rows[keep, 0] - want_rows[keep, 0]).max())
            hz_rel = np.abs(got_rows[keep, 1] / want_rows[keep, 1] - 1.0)
            print('end to end bfloat16 %s %s viterbi=%s: activation %.3g, POV %.3g (bound %.3g), Hz relative %.3g '
                  '(bound %.3g at that frame), cents against the decoder %.3g, %d frames left out'
                  % (capacity, name, viterbi, act_err, pov_err, e, hz_rel.max(), hz_bound[keep][np.argmax(hz_rel)],
                     cents_err, int((~keep).sum())))
            assert pov_err <= e, (pov_err, e)
            assert (hz_rel <= hz_bound[keep]).all()
            source = audio_8k if name == 'test.8k.wav' else Audio(samples, 16000)
            with on_device():
                feats = proc.process(source)
            assert feats.shape == (f64.output_rows(len(samples)), 2) and feats.dtype == np.float64
            np.testing.assert_array_equal(feats.data, f64.finish(got_rows.copy(), len(samples)))
            assert feats.properties == proc.get_properties()
            assert feats.properties['crepe']['precision'] == 'bfloat16'


@pytest.mark.parametrize('viterbi', [True, False])
def test_batch_invariance(gpu, tmp_path, monkeypatch, viterbi):
    from shennong_amd import Audio, Utterances
    capacity, seed = END_TO_END_CAPACITIES[0]
    proc = processor_for(tmp_path, monkeypatch, capacity, seed, viterbi=viterbi)
    proc.precision = 'bfloat16'
    waves = [f64.synthetic_signal(seed=20 + i, seconds=0.25 + 0.07 * i, f0=110.0 + 23 * i) for i in range(9)]
    audios = [Audio(w, 16000) for w in waves]
    with on_device():
        alone = [proc.process(a).data for a in audios]
        together = proc.process_all(Utterances([('utt%d' % i, a) for i, a in enumerate(audios)]))
    for i, want in enumerate(alone):
        assert together['utt%d' % i].shape == want.shape == (f64.output_rows(len(waves[i])), 2)
        np.testing.assert_array_equal(together['utt%d' % i].data, want)
        assert together['utt%d' % i].properties['crepe']['precision'] == 'bfloat16'
    order = [4, 8, 0, 2]
    with on_device():
        feats = proc._process_batch([audios[i] for i in order])
    for got, i in zip(feats, order):
        np.testing.assert_array_equal(got.data, alone[i])


def test_switching(gpu, tmp_path, monkeypatch, audio):
    from shennong_amd.processor import pitch_crepe
    capacity, seed = END_TO_END_CAPACITIES[0]
    samples = audio.data

    def activation(proc):
        with on_device():
            batch = pitch_crepe.CrepeBatch([samples], 160, True)
            batch.forward(pitch_crepe.device_model(proc.model_capacity, batch.device), proc.precision)
            return batch.host_activation()

    fresh = activation(processor_for(tmp_path / 'a', monkeypatch, capacity, seed))
    proc = processor_for(tmp_path / 'b', monkeypatch, capacity, seed)
    first = activation(proc)
    proc.precision = 'bfloat16'
    low = activation(proc)
    proc.precision = 'float32'
    again = activation(proc)
    np.testing.assert_array_equal(first.view(np.uint32), again.view(np.uint32))
    np.testing.assert_array_equal(first.view(np.uint32), fresh.view(np.uint32))
    want, _ = statements(capacity, seed, 'test.wav', samples)
    bound = min(FACTOR * float(np.abs(contract_statement(capacity, seed, 'test.wav', samples) - want).max()), CEILING)
    diff = float(np.abs(low.astype(np.float64) - first).max())
    print('switching: largest |bfloat16 - float32| %.3g, bound %.3g' % (diff, bound))
    assert 0.0 < diff < bound
    with on_device():   # and through the public class
        a = proc.process(audio).data
        proc.precision = 'bfloat16'
        b = proc.process(audio).data
        proc.precision = 'float32'
        np.testing.assert_array_equal(proc.process(audio).data, a)
    assert not np.array_equal(a, b)


def test_invalid_arguments(gpu):
    L, ptr = gpu.lib(), 256

    def conv(x=ptr, x_type=0, c_in=8, packed=ptr, y=ptr, y_type=0, frames=1):
        return L.snf_crepe_conv_bf16(0, x, x_type, frames, 128, c_in, 64, 1, 31, 128, packed, ptr, ptr, ptr, 4, 3, y,
                                     y_type, None)

    assert conv(frames=0) == 0                          # (the arguments below differ from valid ones in one place)
    assert conv(c_in=4) == -1 and conv(c_in=12) == -1
    assert conv(packed=ptr + 8) == -1                   # a misaligned image
    assert conv(x=ptr + 8, x_type=1) == -1              # a misaligned bfloat16 source
    assert conv(x_type=2) == -1 and conv(y_type=-1) == -1 and conv(y_type=2) == -1
    assert conv(y=ptr + 1, y_type=1) == -1
    assert conv(frames=-1) == -1 and conv(packed=None) == -1 and conv(x=None) == -1    # the checks of snf_crepe_conv
    assert L.snf_crepe_conv_bf16(0, ptr, 0, 1, 128, 8, 64, 1, 31, 127, ptr, ptr, ptr, ptr, 4, 3, ptr, 0, None) == -1
    assert L.snf_crepe_conv_bf16(0, ptr, 0, 1, 128, 8, 64, 1, 31, 128, ptr, ptr, None, ptr, 4, 1, ptr, 0, None) == -1
    assert L.snf_crepe_conv_bf16(0, ptr, 0, 1, 128, 8, 64, 1, 31, 128, ptr, ptr, ptr, ptr, 4, 8, ptr, 0, None) == -1
    off = (C.c_int64 * 2)(0, 2048)
    filters = (C.c_int32 * 6)(128, 16, 16, 16, 32, 64)
    params = (C.c_void_p * 26)(*([ptr] * 26))
    assert L.snf_crepe_forward_bf16(0, ptr, off, 0, 160, 1, filters, params, ptr, None) == 0
    assert L.snf_crepe_forward_bf16(0, ptr, off, -1, 160, 1, filters, params, ptr, None) == -1
    assert L.snf_crepe_forward_bf16(0, ptr, off, 1, 0, 1, filters, params, ptr, None) == -1
    assert L.snf_crepe_forward_bf16(0, ptr, off, 1, 160, 1, None, params, ptr, None) == -1
    assert L.snf_crepe_forward_bf16(0, None, off, 1, 160, 1, filters, params, ptr, None) == -1
    params[8] = None                                    # a null image slot
    assert L.snf_crepe_forward_bf16(0, ptr, off, 1, 160, 1, filters, params, ptr, None) == -1
    params[8] = ptr + 4                                 # a misaligned one
    assert L.snf_crepe_forward_bf16(0, ptr, off, 1, 160, 1, filters, params, ptr, None) == -1
    params[8] = ptr
    filters[2] = 20                                     # C_in of block 4 is no multiple of 8
    assert L.snf_crepe_forward_bf16(0, ptr, off, 1, 160, 1, filters, params, ptr, None) == -1
