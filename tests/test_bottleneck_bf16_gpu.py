"""The bfloat16 matrix-core path of the bottleneck networks (``precision='bfloat16'``) on the device: the layer
alone, the rounding, the new entry points' validation, the networks against the reference's float64 outputs
in tests/golden/reference_bottleneck.npz, batch invariance and switching between the precisions.

Error bound, as in tests/test_bottleneck_gpu.py: the test evaluates the numpy statement of the contract
(tests/bottleneck_bf16.py) in float32 on the same input, takes its largest absolute error against the float64
reference, and allows the device 4 times that, never more than 2e-2.  For the layer alone the operands are
rounded to bfloat16 beforehand, so every product is exact in float32 and the float32 numpy result differs from
float64 by its accumulation only.  For the networks both errors are dominated by the same quantisation (about
3e-3), so the ratio is near 1 and the factor 4 is margin (activations on rounding ties fall either side:
about 6e-4).  Measured figures are printed; DESIGN 4.9 records them."""

import numpy as np
import pytest

import bottleneck_bf16 as b16
import bottleneck_f64 as f64
from test_bottleneck import cases
from test_bottleneck_gpu import FACTOR, bound, golden, processor_for, ragged_batch  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 7, 1), (3, 8, 5), (63, 17, 96), (63, 80, 96), (129, 96, 129), (257, 200, 80),
          (63, 500, 500), (63, 1500, 80), (130, 1500, 1500)]


@pytest.mark.parametrize('act', ['identity', 'sigmoid'])
def test_dense_layer_bf16(gpu, act):
    from shennong_amd.processor import bottleneck
    rng = np.random.RandomState(1)
    for m, k, n in SHAPES:
        x = b16.bf16(rng.uniform(0.0, 1.0, (m, k)).astype(np.float32))
        w = b16.bf16((rng.uniform(-1.0, 1.0, (k, n)) / np.sqrt(k)).astype(np.float32))
        b = rng.uniform(-0.1, 0.1, n).astype(np.float32)
        want = x.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
        low = x @ w + b
        if act == 'sigmoid':
            want, low = f64._sigmoid(want), f64._sigmoid(low)
        got = bottleneck.dense_layer(x, w, b, act, precision='bfloat16')
        assert got.shape == (m, n) and got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - want).max())
        limit = bound(low, want)
        print('dense bfloat16 %s %dx%dx%d: device %.3g, float32 numpy %.3g' % (act, m, k, n, err, limit / FACTOR))
        assert err <= limit, (act, m, k, n, err, limit)
        # a row alone gives the bits it has in the block
        row = m // 2
        alone = bottleneck.dense_layer(x[row:row + 1], w, b, act, precision='bfloat16')
        np.testing.assert_array_equal(alone[0], got[row])


def test_rounding_on_device(gpu):
    """The device rounds both operands to nearest, ties to even: operands rounded on the host beforehand give
    the same bits"""
    from shennong_amd.processor import bottleneck
    rng = np.random.RandomState(2)
    ties = np.array([1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3.0 * 2.0 ** -8),
                     2.0 - 2.0 ** -9, 0.5 + 2.0 ** -9, 2.0 ** -126 * (1.0 + 2.0 ** -8),
                     -2.0 ** -125 * (1.0 + 3.0 * 2.0 ** -8), 2.0 ** -126 * 1.37, 2.0 ** -124 * 1.9999],
                    dtype=np.float32)
    for m, k, n in [(5, 7, 3), (70, 100, 131)]:
        x = rng.uniform(-2.0, 2.0, (m, k)).astype(np.float32)
        w = rng.uniform(-1.0, 1.0, (k, n)).astype(np.float32)
        x.reshape(-1)[rng.choice(x.size, 3 * ties.size, replace=False)] = np.tile(ties, 3)
        w.reshape(-1)[rng.choice(w.size, 2 * ties.size, replace=False)] = np.tile(ties, 2)
        b = rng.uniform(-0.1, 0.1, n).astype(np.float32)
        assert not np.array_equal(b16.bf16(x), x) and not np.array_equal(b16.bf16(w), w)
        raw = bottleneck.dense_layer(x, w, b, precision='bfloat16')
        rounded = bottleneck.dense_layer(b16.bf16(x), b16.bf16(w), b, precision='bfloat16')
        assert np.isfinite(raw).all()
        np.testing.assert_array_equal(raw.view(np.uint32), rounded.view(np.uint32))
        assert not np.array_equal(raw, bottleneck.dense_layer(x, w, b))     # (the float32 layer does not round)


def test_invalid_arguments(gpu):
    import ctypes as C
    L, ptr = gpu.lib(), 256
    assert L.snf_dense_layer_bf16(0, ptr, -1, 4, ptr, ptr, 4, 0, ptr, None) == -1
    assert L.snf_dense_layer_bf16(0, ptr, 4, 0, ptr, ptr, 4, 0, ptr, None) == -1
    assert L.snf_dense_layer_bf16(0, ptr, 4, 4, ptr, ptr, 4, 2, ptr, None) == -1
    assert L.snf_dense_layer_bf16(0, None, 4, 4, ptr, ptr, 4, 0, ptr, None) == -1
    assert L.snf_dense_layer_bf16(0, ptr, 4, 4, None, ptr, 4, 0, ptr, None) == -1
    assert L.snf_dense_layer_bf16(0, ptr, 4, 4, ptr + 8, ptr, 4, 0, ptr, None) == -1     # image not 16-byte aligned
    assert L.snf_dense_layer_bf16(0, ptr, 4, (1 << 20) + 1, ptr, ptr, 4, 0, ptr, None) == -1
    assert L.snf_pack_weights_bf16(0, ptr, 0, 4, ptr, None) == -1
    assert L.snf_pack_weights_bf16(0, ptr, 4, -1, ptr, None) == -1
    assert L.snf_pack_weights_bf16(0, None, 4, 4, ptr, None) == -1
    assert L.snf_pack_weights_bf16(0, ptr, 4, 4, None, None) == -1
    assert L.snf_pack_weights_bf16(0, ptr, 4, 4, ptr + 2, None) == -1
    assert L.snf_packed_weights_bf16_size(0, 4) == 0 and L.snf_packed_weights_bf16_size(4, (1 << 20) + 1) == 0
    assert L.snf_packed_weights_bf16_size(1, 1) == 64 and L.snf_packed_weights_bf16_size(64, 3) == 192
    assert L.snf_packed_weights_bf16_size(65, 3) == 384 and L.snf_packed_weights_bf16_size(1500, 80) == 80 * 1536
    off = (C.c_int64 * 2)(0, 30)
    widths = (C.c_int32 * 4)(8, 8, 8, 8)
    params = (C.c_void_p * 12)(*([ptr] * 12))
    assert L.snf_bottleneck_forward_bf16(0, ptr, off, -1, widths, params, ptr, ptr, None) == -1
    assert L.snf_bottleneck_forward_bf16(0, ptr, None, 1, widths, params, ptr, ptr, None) == -1
    assert L.snf_bottleneck_forward_bf16(0, ptr, off, 1, None, params, ptr, ptr, None) == -1
    assert L.snf_bottleneck_forward_bf16(0, None, off, 1, widths, params, ptr, ptr, None) == -1
    short = (C.c_int64 * 2)(0, 20)
    assert L.snf_bottleneck_forward_bf16(0, ptr, short, 1, widths, params, ptr, ptr, None) == -1
    params[8] = ptr + 4
    assert L.snf_bottleneck_forward_bf16(0, ptr, off, 1, widths, params, ptr, ptr, None) == -1
    params[8] = None
    assert L.snf_bottleneck_forward_bf16(0, ptr, off, 1, widths, params, ptr, ptr, None) == -1
    widths[2] = 0
    params[8] = ptr
    assert L.snf_bottleneck_forward_bf16(0, ptr, off, 1, widths, params, ptr, ptr, None) == -1


def test_fixture_cases_bf16(gpu, golden, tmp_path, monkeypatch):  # noqa: F811
    from shennong_amd import Audio
    from shennong_amd.processor import bottleneck
    for n in cases(golden):
        seed, hidden, context = (int(v) for v in golden['case_' + n])
        key = str(golden['signal_' + n])
        samples = golden['input_' + key]
        proc = processor_for(tmp_path / n, monkeypatch, seed, hidden, context)
        low = b16.extract(samples, f64.make_weights(seed, hidden, context), np.float32)
        dnet = proc._device_network(_device())
        # the float32 path first: the front end of the bfloat16 path is its code, unchanged
        plain = bottleneck.BottleneckBatch([samples])
        plain_voiced = plain.vad()
        plain.fbank(0.0)
        plain_out = plain.forward(dnet)
        batch = bottleneck.BottleneckBatch([samples])
        voiced = batch.vad()
        batch.fbank(0.0)
        out = batch.forward(dnet, precision='bfloat16')
        np.testing.assert_array_equal(batch.host_mask(), plain.host_mask())
        np.testing.assert_array_equal(batch.host_mask(), golden['vad_' + key])
        np.testing.assert_array_equal(voiced, plain_voiced)
        np.testing.assert_array_equal(batch.host_logmel().view(np.uint32), plain.host_logmel().view(np.uint32))
        assert not np.array_equal(out, plain_out)
        for stage, got in (('bn', batch.host_bn()), ('out', out)):
            want = golden[stage + '_' + n]
            assert got.shape == want.shape and got.dtype == np.float32
            err = float(np.abs(got.astype(np.float64) - want).max())
            limit = bound(low[stage], want)
            print('%s %s bfloat16: device %.3g, float32 numpy %.3g, bound %.3g' % (n, stage, err, limit / FACTOR, limit))
            assert err <= limit, (n, stage, err, limit)
        # through the public class
        proc.precision = 'bfloat16'
        feats = proc.process(Audio(samples, 8000))
        assert feats.dtype == np.float32
        np.testing.assert_array_equal(feats.data, out)
        np.testing.assert_array_equal(feats.times, f64.times(feats.shape[0]))
        assert feats.properties == proc.get_properties()
        assert feats.properties['bottleneck']['precision'] == 'bfloat16'


def _device():
    from shennong_amd import _backend
    return _backend.get_device()


def test_batch_invariance_bf16(gpu, tmp_path, monkeypatch):
    from shennong_amd import Audio, Utterances
    proc = processor_for(tmp_path, monkeypatch, seed=21, hidden=200, context=5)
    proc.precision = 'bfloat16'
    count = 23
    waves = ragged_batch(count)
    audios = [Audio(w, 8000) for w in waves]
    alone = [proc.process(a).data for a in audios]
    utts = Utterances([('utt%02d' % i, a) for i, a in enumerate(audios)])
    together = proc.process_all(utts)
    for i, want in enumerate(alone):
        got = together['utt%02d' % i]
        assert got.shape == want.shape == (f64.num_frames(len(waves[i])), 80)
        np.testing.assert_array_equal(got.data, want)
        assert got.properties['bottleneck']['precision'] == 'bfloat16'
    probe = 7
    for position in (0, count // 2, count - 1):
        order = [i for i in range(count) if i != probe]
        order.insert(position, probe)
        feats = proc._process_batch([audios[i] for i in order])
        np.testing.assert_array_equal(feats[position].data, alone[probe])


def test_switching(gpu, golden, tmp_path, monkeypatch):  # noqa: F811
    from shennong_amd import Audio
    audio = Audio(golden['input_wav'], 8000)
    fresh = processor_for(tmp_path / 'a', monkeypatch, seed=31, hidden=96, context=5)
    want = fresh.process(audio).data
    proc = processor_for(tmp_path / 'b', monkeypatch, seed=31, hidden=96, context=5)
    proc.precision = 'bfloat16'
    low = proc.process(audio).data
    np.testing.assert_array_equal(proc.process(audio).data, low)
    proc.precision = 'float32'
    np.testing.assert_array_equal(proc.process(audio).data, want)
    proc.precision = 'bfloat16'
    np.testing.assert_array_equal(proc.process(audio).data, low)
    assert not np.array_equal(low, want)
    diff = float(np.abs(low.astype(np.float64) - want).max())
    print('switching: largest |bfloat16 - float32| %.3g' % diff)
    assert 0.0 < diff <= 2e-2
