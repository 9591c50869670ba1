"""The summation order of the FP32 matrix-core kernels on the device, in bits: bn_dense_kernel (one chain of fused
multiply-adds over k ascending) and crepe_conv_kernel (chains of 256 k, added in ascending order) against the host
statement of tests/gemm_order.py, whose every step is exact on these operands (tests/test_gemm_order.py).  The
bfloat16 kernels are not stated here: the order inside a matrix-core step of 16 k is the hardware's."""

import numpy as np
import pytest

import gemm_order as go
from test_crepe_gpu import on_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', go.DENSE_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_dense_layer_order(gpu, case):
    from shennong_amd.processor import bottleneck
    x, w, b = go.dense_case(*case)
    want = go.dense_statement(case)
    with on_device():
        got = bottleneck.dense_layer(x, w, b, 'identity')
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('case', go.CONV_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_conv_layer_order(gpu, case):
    from shennong_amd.processor import pitch_crepe
    frames, length, c_in, width, stride, pad_left, c_out = case
    x, kernel, b, _ = go.conv_case(*case)
    want = go.conv_statement(case)
    with on_device():
        got = pitch_crepe.conv_layer(x, kernel, b, stride=stride, pad_left=pad_left, pool=False)
    assert got.shape == want.shape == (frames, -(-length // stride), c_out) and got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
