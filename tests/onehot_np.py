"""The framed one-hot rule in numpy, written from its statement and independent of the product's code:
float64 sample times, float32 sums in sample order.

An alignment is (onset of the first token, offsets [ntokens] in seconds, ids [ntokens]).  Sample `i` sits at
``i / rate + onset0`` and carries the first token whose offset is greater than that time (the last token when
there is none).  Frame `f` covers samples ``[f * shift, f * shift + length)``.  A frame whose samples carry one
token takes it; otherwise every token of the frame weighs the float32 sum of the window coefficients of its
samples, added one after the other in sample order starting from zero, the largest weight wins and an exact
tie goes to the token that comes first in the frame."""

import numpy as np


def num_samples(onset0, offsets, rate):
    return int((offsets[-1] - onset0) * rate) if len(offsets) else 0


def num_frames(nsamples, length, shift):
    """Kaldi's NumFrames for whole frames only (snip_edges)"""
    return 0 if nsamples < length else 1 + (nsamples - length) // shift


def sample_ids(onset0, offsets, ids, rate):
    """The token id of every sample"""
    offsets = np.asarray(offsets, dtype=np.float64)
    times = np.arange(num_samples(onset0, offsets, rate)) / rate + onset0
    segment = np.searchsorted(offsets, times, side='right')
    return np.asarray(ids)[np.minimum(segment, len(offsets) - 1)] if len(offsets) else np.zeros(0, dtype=int)


def sequential_sum(values):
    """((0 + v0) + v1) + ... in float32"""
    total = np.float32(0)
    for v in np.asarray(values, dtype=np.float32):
        total = np.float32(total + v)
    return total


def frame_winner(frame_ids, window):
    """The id that labels a frame of per-sample ids"""
    if np.all(frame_ids == frame_ids[0]):
        return int(frame_ids[0])
    _, first = np.unique(frame_ids, return_index=True)
    best, winner = None, None
    for position in np.sort(first):          # tokens in order of first appearance
        token = frame_ids[position]
        weight = sequential_sum(window[frame_ids == token])
        if best is None or weight > best:
            best, winner = weight, int(token)
    return winner


def framed_winners(onset0, offsets, ids, rate, length, shift, window):
    """The winning id of every frame, int32 [nframes]"""
    window = np.asarray(window, dtype=np.float32)
    assert window.shape == (length,)
    sampled = sample_ids(onset0, offsets, ids, rate)
    nframes = num_frames(sampled.shape[0], length, shift)
    return np.array([frame_winner(sampled[f * shift:f * shift + length], window) for f in range(nframes)],
                    dtype=np.int32).reshape(nframes)


def framed_onehot(onset0, offsets, ids, width, rate, length, shift, window):
    """bool [nframes, width]"""
    winners = framed_winners(onset0, offsets, ids, rate, length, shift, window)
    data = np.zeros((winners.shape[0], width), dtype=bool)
    data[np.arange(winners.shape[0]), winners] = True
    return data
