"""The summation order of the FP32 matrix-core kernels (shennong_amd/csrc/gemm_tiles.h: gemm_f32), stated on the
host in bits: every output element is chains of `chain` consecutive k of fused multiply-adds from a float32 zero,
k ascending, the chains' results added in float32 in ascending order; ``chain = 0`` is one chain over all k (the
dense layer of the bottleneck networks), ``chain = 256`` the CREPE convolution.  The bias is added last, in float32.

One step is ``float32(float64(a) * float64(b) + float64(acc))``.  That is the float32 fused multiply-add exactly
when the operands are coarse enough, and `operands` draws such: x in multiples of 2^-7 in [0, 2), w in multiples of
2^-12 in [0, 1), the bias in multiples of 2^-7.  A product is then a multiple of 2^-19 below 2 and a running sum a
multiple of 2^-19 below 2^10 (K < 512): 29 bits, so product and sum are exact in float64 and the step rounds once.
tests/test_gemm_order.py checks that against np.longdouble steps, and that the order matters at these sizes."""

import functools

import numpy as np

# (M, K, N) of bottleneck.dense_layer, identity activation
DENSE_CASES = [(3, 33, 5),         # scalar loaders, odd K across a k tile (no sum reaches the rounding range)
               (5, 320, 7),        # vector A, scalar B
               (5, 321, 8),        # scalar A, vector B
               (130, 320, 132)]    # two M tiles, two N tiles, partial in both
# (frames, length, C_in, width, stride, pad_left, C_out) of pitch_crepe.conv_layer, no scale or shift, no pool
CONV_CASES = [(3, 16, 8, 40, 1, 19, 7),      # K = 320: chains of 256 + 64, vector A, runs into the padding on both sides
              (2, 64, 1, 300, 4, 149, 8),    # K = 300: chains of 256 + 44, scalar A
              (1, 96, 8, 40, 1, 19, 7)]      # K = 320 with whole runs inside the frame: both chains carry data
# In the first two the frame is shorter than the kernel, so a run is mostly padding: the second chain holds data in 9
# of 48 rows of the first and in no row of the second (its data end at k = 212).  They test addressing and padding;
# the third is the one in which one chain and chains of 256 give different bits (tests/test_gemm_order.py).
CONV_CASES_MOSTLY_PADDING = CONV_CASES[:2]
DENSE_CHAIN, CONV_CHAIN = 0, 256


def fma_step(a, b, acc, wide=np.float64):
    """float32 fma(a, b, acc) elementwise, computed in `wide` and rounded once"""
    return (a.astype(wide) * b.astype(wide) + acc.astype(wide)).astype(np.float32)


def chained_matmul(a, w, chain):
    """a [M, K] times w [K, N], float32, in the kernels' order"""
    a, w = np.asarray(a, np.float32), np.asarray(w, np.float32)
    acc = np.zeros((a.shape[0], w.shape[1]), np.float32)
    total = np.zeros_like(acc)
    for k in range(a.shape[1]):
        acc = fma_step(a[:, k, None], w[None, k, :], acc)
        if chain and ((k + 1) % chain == 0 or k + 1 == a.shape[1]):
            total = total + acc                      # float32 + float32: one rounding
            acc = np.zeros_like(acc)
    return total if chain else acc


def conv_rows(x, width, stride, pad_left):
    """The implicit matrix of the convolution: row (frame, position t) is the run of width * C_in values of
    x [frames, length, C_in] from position t * stride - pad_left on, zeros outside the frame"""
    frames, length, c_in = x.shape
    positions = -(-length // stride)
    padded = np.zeros((frames, pad_left + positions * stride + width, c_in), np.float32)
    padded[:, pad_left:pad_left + length] = x
    rows = [padded[:, t * stride:t * stride + width].reshape(frames, width * c_in) for t in range(positions)]
    return np.stack(rows, axis=1).reshape(frames * positions, width * c_in)


def operands(rng, m, k, n):
    x = (rng.randint(0, 256, (m, k)) / 128.0).astype(np.float32)
    w = (rng.randint(0, 4096, (k, n)) / 4096.0).astype(np.float32)
    b = (rng.randint(-64, 64, n) / 128.0).astype(np.float32)
    return x, w, b


@functools.lru_cache(maxsize=None)
def dense_case(m, k, n):
    """x [M, K], w [K, N], b [N]"""
    return operands(np.random.RandomState(3), m, k, n)


@functools.lru_cache(maxsize=None)
def conv_case(frames, length, c_in, width, stride, pad_left, c_out):
    """x [frames, length, C_in], kernel [width, C_in, C_out], b [C_out] and the implicit matrix [rows, K]"""
    x, w, b = operands(np.random.RandomState(3), frames * length, c_in, c_out)
    x = x.reshape(frames, length, c_in)
    kernel = (np.random.RandomState(4).randint(0, 4096, (width, c_in, c_out)) / 4096.0).astype(np.float32)
    return x, kernel, b, conv_rows(x, width, stride, pad_left)


def dense_statement(case, chain=DENSE_CHAIN):
    x, w, b = dense_case(*case)
    return chained_matmul(x, w, chain) + b


def conv_statement(case, chain=CONV_CHAIN):
    x, kernel, b, a = conv_case(*case)
    out = chained_matmul(a, kernel.reshape(-1, kernel.shape[2]), chain) + b
    return out.reshape(x.shape[0], -1, kernel.shape[2])
