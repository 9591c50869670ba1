"""The host statement of the FP32 kernels' summation order (tests/gemm_order.py) is worth comparing bits with: on
the cases of tests/test_gemm_order_gpu.py every emulated fused multiply-add rounds once, and a kernel that summed in
another order would differ from the statement in most output elements."""

import numpy as np
import pytest

import gemm_order as go

CASES = [('dense', c) for c in go.DENSE_CASES] + [('conv', c) for c in go.CONV_CASES]
IDS = ['%s-%s' % (kind, 'x'.join(str(v) for v in c)) for kind, c in CASES]


def matrices(kind, case):
    if kind == 'dense':
        x, w, _ = go.dense_case(*case)
        return x, w
    _, kernel, _, a = go.conv_case(*case)
    return a, kernel.reshape(-1, kernel.shape[2])


@pytest.mark.parametrize('kind,case', CASES, ids=IDS)
def test_steps_round_once(kind, case):
    """Every step of one chain over all k, the longest sums there are: the float64 step equals the np.longdouble one"""
    a, w = matrices(kind, case)
    assert a.shape[1] < 512 and (a * 128 == np.round(a * 128)).all() and (w * 4096 == np.round(w * 4096)).all()
    assert 0 <= a.min() and a.max() < 2 and 0 <= w.min() and w.max() < 1
    acc = np.zeros((a.shape[0], w.shape[1]), np.float32)
    for k in range(a.shape[1]):
        nxt = go.fma_step(a[:, k, None], w[None, k, :], acc)
        wide = go.fma_step(a[:, k, None], w[None, k, :], acc, np.longdouble)
        np.testing.assert_array_equal(nxt.view(np.uint32), wide.view(np.uint32))
        exact = a[:, k, None].astype(np.float64) * w[None, k, :].astype(np.float64) + acc.astype(np.float64)
        assert (exact * 2.0 ** 19 == np.round(exact * 2.0 ** 19)).all() and exact.max() < 2.0 ** 10
        acc = nxt
    np.testing.assert_array_equal(acc.view(np.uint32), go.chained_matmul(a, w, 0).view(np.uint32))


def test_conv_rows():
    """The implicit matrix against the definition, element by element, with padding on both sides"""
    frames, length, c_in, width, stride, pad_left, _ = go.CONV_CASES[1]
    x, _, _, a = go.conv_case(*go.CONV_CASES[1])
    positions = -(-length // stride)
    assert a.shape == (frames * positions, width * c_in)
    for f in range(frames):
        for t in range(positions):
            for tap in range(width):
                p = t * stride - pad_left + tap
                want = x[f, p] if 0 <= p < length else np.zeros(c_in, np.float32)
                np.testing.assert_array_equal(a[f * positions + t, tap * c_in:(tap + 1) * c_in], want)
    assert (a[0, :pad_left * c_in] == 0).all() and (a[-1, -c_in:] == 0).all()


def differing(a, w, right, wrong):
    return float((go.chained_matmul(a, w, wrong).view(np.uint32) != go.chained_matmul(a, w, right).view(np.uint32)).mean())


@pytest.mark.parametrize('kind,case', CASES, ids=IDS)
def test_order_matters(kind, case):
    """One chain instead of 256 (convolution), 256 instead of one (dense layer), chains of 32 for both: each differs
    from the kernel's order in at least half of the output elements.  Exempt, because the condition cannot hold
    there: K = 33, where no sum reaches the rounding range (that case tests indexing only), and the two convolutions
    whose runs are mostly padding (gemm_order.CONV_CASES_MOSTLY_PADDING: one chain and chains of 256 are the same
    sums in 39 of 48 rows and in all rows; their figures are printed)."""
    a, w = matrices(kind, case)
    right, wrong = (go.DENSE_CHAIN, go.CONV_CHAIN) if kind == 'dense' else (go.CONV_CHAIN, go.DENSE_CHAIN)
    for chain in (wrong, 32):
        share = differing(a, w, right, chain)
        print('%s %s: chains of %d against %d differ in %.2f of the elements' % (kind, case, chain, right, share))
        if a.shape[1] == 33 or case in go.CONV_CASES_MOSTLY_PADDING:
            continue
        assert share >= 0.5, (kind, case, chain, share)


@pytest.mark.parametrize('k', [320, 300])
def test_order_matters_without_padding(k):
    """The same on plain matrices of the K of the convolution cases, for both kernels' orders"""
    x, w, _ = go.operands(np.random.RandomState(3), 40, k, 8)
    for right, wrong in ((go.CONV_CHAIN, go.DENSE_CHAIN), (go.CONV_CHAIN, 32), (go.DENSE_CHAIN, go.CONV_CHAIN),
                         (go.DENSE_CHAIN, 32)):
        share = differing(x, w, right, wrong)
        print('K = %d: chains of %d against %d differ in %.2f of the elements' % (k, wrong, right, share))
        assert share >= 0.5, (k, right, wrong, share)
