"""Numpy statement of the CREPE network's bfloat16 contract (``precision='bfloat16'``): the network of
tests/crepe_f64.py with every activation and every kernel weight rounded to bfloat16 (to nearest, ties to even)
at the inputs of convolution blocks 2 to 6; products, sums, bias, ReLU, normalisation and pool in `dtype`.  The
ingest, block 1 and the classifier are those of crepe_f64 unchanged.  A plain helper module of the test suite:
it shares no code with shennong_amd.processor.pitch_crepe."""

import numpy as np

import crepe_f64 as f64
from bottleneck_bf16 import bf16


def quantised_block(x, weights, l, dtype=np.float64):
    """Block `l` of crepe_f64 on the bfloat16 roundings of `x` and of the block's kernel"""
    name = 'conv%d/kernel' % l
    w = dict(weights)
    w[name] = bf16(weights[name]).astype(dtype)
    return f64.block(bf16(x).astype(dtype), w, l, dtype)


def activation_of_frames(frames, weights, dtype=np.float64):
    x = f64.block(frames.astype(dtype)[:, :, None], weights, 1, dtype)
    for l in range(2, 7):
        x = quantised_block(x, weights, l, dtype)
    flat = x.reshape(x.shape[0], -1)
    z = flat @ weights['classifier/kernel'].astype(dtype) + weights['classifier/bias'].astype(dtype)
    return f64.sigmoid(z).astype(dtype)


def activation(samples, weights, hop=160, center=True, dtype=np.float64):
    return activation_of_frames(f64.frames_of(samples, hop, center, dtype), weights, dtype)
