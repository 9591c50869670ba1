"""BottleneckProcessor.precision on the host: the bfloat16 rounding helper's known answers, the attribute, and
the numpy statement of the bfloat16 contract (tests/bottleneck_bf16.py) in float64 against the reference's
outputs in tests/golden/reference_bottleneck.npz.

Bound of the statement: the 2e-2 absolute that the reference's own comparison with the original extractor
allows (CEILING of tests/test_bottleneck_gpu.py).  Measured: at most 3.1e-3 (`out`) and 3.0e-3 (`bn`)."""

import numpy as np
import pytest

import bottleneck_bf16 as b16
import bottleneck_f64 as f64
from test_bottleneck import cases, golden, weights_dir, write_weights  # noqa: F401  (fixtures)

CEILING = 2e-2


def test_bf16_known_answers():
    def one(v):
        return float(b16.bf16(np.array([v], dtype=np.float32))[0])

    for exact in (0.0, 1.0, -1.0, 0.5, 1.0 + 2.0 ** -7, 3.0, -2.0 ** -120, 2.0 ** 100, 255.0):
        assert one(exact) == exact
    assert one(1.0 + 2.0 ** -8) == 1.0                           # a tie: to the even mantissa below
    assert one(1.0 + 3.0 * 2.0 ** -8) == 1.0 + 2.0 ** -6         # a tie: to the even mantissa above
    assert one(1.0 + 2.0 ** -8 + 2.0 ** -20) == 1.0 + 2.0 ** -7  # just above the tie
    assert one(1.0 + 2.0 ** -8 - 2.0 ** -20) == 1.0              # just below the tie
    assert one(-(1.0 + 2.0 ** -8)) == -1.0
    assert one(-(1.0 + 3.0 * 2.0 ** -8)) == -(1.0 + 2.0 ** -6)
    assert one(-0.3) == -0.30078125                              # -0x1.34p-2
    assert one(2.0 - 2.0 ** -9) == 2.0                           # the mantissa carries into the exponent
    assert one(-(4.0 - 2.0 ** -20)) == -4.0
    assert one(2.0 ** -126 * (1.0 + 2.0 ** -8)) == 2.0 ** -126   # a tie in the smallest normal binade
    out = b16.bf16(np.arange(6, dtype=np.float32).reshape(2, 3) / 7)
    assert out.shape == (2, 3) and out.dtype == np.float32
    assert not (out.view(np.uint32) & 0xFFFF).any()


def test_precision_attribute(weights_dir):  # noqa: F811
    from shennong_amd.processor import BottleneckProcessor
    write_weights(weights_dir)
    proc = BottleneckProcessor(dither=0)
    assert proc.precision == 'float32'
    assert proc.get_params() == {'weights': 'BabelMulti', 'dither': 0.0}
    default = proc.get_properties()
    assert default['bottleneck'] == {'weights': 'BabelMulti', 'dither': 0.0}
    for bad in ('float16', 'bf16', 'BFLOAT16', None, 32):
        with pytest.raises(ValueError) as err:
            proc.precision = bad
        assert 'float32' in str(err.value) and 'bfloat16' in str(err.value)
        assert proc.precision == 'float32'
    proc.precision = 'bfloat16'
    assert proc.precision == 'bfloat16'
    assert proc.get_params() == {'weights': 'BabelMulti', 'dither': 0.0}
    props = proc.get_properties()
    assert props['bottleneck'] == {'weights': 'BabelMulti', 'dither': 0.0, 'precision': 'bfloat16'}
    assert props['pipeline'] == default['pipeline']
    with pytest.raises(ValueError, match='invalid parameter precision'):
        proc.set_params(precision='float32')
    assert proc.precision == 'bfloat16'
    with pytest.raises(TypeError):
        BottleneckProcessor(precision='bfloat16')
    proc.precision = 'float32'
    assert proc.get_properties() == default


def test_arguments_validated():
    from shennong_amd.processor import bottleneck
    x, w, b = np.zeros((2, 3), np.float32), np.zeros((3, 4), np.float32), np.zeros(4, np.float32)
    with pytest.raises(ValueError, match='float32, bfloat16'):
        bottleneck.dense_layer(x, w, b, precision='half')
    batch = object.__new__(bottleneck.BottleneckBatch)
    with pytest.raises(ValueError, match='float32, bfloat16'):
        batch.forward(None, precision='half')


def test_bf16_statement_against_reference(golden):  # noqa: F811
    worst = {'bn': 0.0, 'out': 0.0}
    for n in cases(golden):
        seed, hidden, context = (int(v) for v in golden['case_' + n])
        key = str(golden['signal_' + n])
        got = b16.extract(golden['input_' + key], f64.make_weights(seed, hidden, context))
        np.testing.assert_array_equal(got['vad'], golden['vad_' + key])
        for stage in ('bn', 'out'):
            want = golden[stage + '_' + n]
            assert got[stage].shape == want.shape and got[stage].dtype == np.float64
            err = float(np.abs(got[stage] - want).max())
            print('%s %s: bfloat16 statement %.3g (largest magnitude %.3g)' % (n, stage, err, np.abs(want).max()))
            worst[stage] = max(worst[stage], err)
    assert 0.0 < worst['bn'] <= CEILING and 0.0 < worst['out'] <= CEILING, worst
