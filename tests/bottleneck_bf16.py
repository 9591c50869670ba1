"""Numpy statement of the bottleneck networks' bfloat16 contract (``precision='bfloat16'``): the networks of
tests/bottleneck_f64.py with every activation and every weight rounded to bfloat16 (to nearest, ties to
even) at the inputs of W2, W3, W6 and W7; products, sums, bias and sigmoid in `dtype`.  A plain helper module
of the test suite: it shares no code with shennong_amd.processor.bottleneck."""

import numpy as np

import bottleneck_f64 as f64


def bf16(a):
    """float32 -> bfloat16 (round to nearest, ties to even), returned as float32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def forward(x, weights, dtype=np.float64):
    """(final [rows - 20, 80], first stage [rows, 80]) as bottleneck_f64.forward, W2 W3 W6 W7 in bfloat16"""
    dtype = np.dtype(dtype)
    w = {k: np.asarray(v).astype(dtype) for k, v in weights.items() if k != 'context'}

    def q(a):
        return bf16(a).astype(dtype)

    y = (np.asarray(x, dtype=dtype) + w['input_mean']) * w['input_std']
    y = f64._sigmoid(y @ w['W1'] + w['b1'])
    y = f64._sigmoid(q(y) @ q(w['W2']) + w['b2'])
    bn = q(y) @ q(w['W3']) + w['b3']
    n = bn.shape[0] - 20
    z = np.concatenate([bn[5 * j:5 * j + n] for j in range(5)], axis=1)
    z = (z + w['bn_mean']) * w['bn_std']
    z = f64._sigmoid(z @ w['W5'] + w['b5'])
    z = f64._sigmoid(q(z) @ q(w['W6']) + w['b6'])
    return (q(z) @ q(w['W7']) + w['b7']).astype(dtype), bn.astype(dtype)


def extract(samples, weights, dtype=np.float64):
    """The stages of one utterance (8 kHz int16, no dither) with the networks in the bfloat16 contract"""
    context = int(weights['context'])
    mask = f64.vad(samples)
    fea = f64.logmel(samples, dtype)
    out, bn = forward(f64.nn_input(fea, mask, context, dtype), weights, dtype)
    return {'vad': mask, 'logmel': fea, 'bn': bn, 'out': out}
