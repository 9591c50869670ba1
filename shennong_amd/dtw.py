"""DTW distances between feature items, on the GPU

An extension with no counterpart in the reference.  Its worked examples (reference examples/features_abx,
examples/vtln_training) extract features and then evaluate them by ABX discrimination: an external toolkit
computes, on the CPU and one pair at a time, a dynamic-time-warping distance over a frame-wise cosine distance,
normalised by the length of the path (``abx-distance -n 1``, examples/features_abx/scripts/abx_score.sh:21).
:func:`dtw_distances` computes that distance for all the pairs of a call on the rows of a
:class:`~shennong_amd.device.DeviceFeaturesCollection` where they lie in HBM (snf_dtw_pairs):

    feats = processor.process_all_device(utterances)
    items = [('utt1', 0.31, 0.52), ('utt2', 1.10, 1.38), ...]         # (name, onset, offset) in seconds
    dist = dtw_distances(feats, [(0, 1), (0, 2)], items=items)         # float32 [P]

For the items x [N, D] and y [M, D] of a pair, with d[i, j] the frame distance of row i of x and row j of y:

    cosine       d = arccos(clip(x_i.y_j / (|x_i| |y_j|), -1, 1)) / pi; 1 if one of the rows is zero, 0 if both
    sqeuclidean  d = sum_k (x_ik - y_jk)^2
    symkl        d = 0.5 sum_k (x~_ik - y~_jk) (ln x~_ik - ln y~_jk), x~ = max(x, 2^-40) element-wise: the symmetric
                 KL divergence of rows of probabilities (posteriorgrams, ``DiagUbmProcessor.posteriorgrams``); zero
                 and negative entries count as 2^-40, rows need not sum to 1
    C[0, 0] = d[0, 0], L[0, 0] = 1;  C[i, j] = d[i, j] + C[p], L[i, j] = L[p] + 1, p the predecessor of smallest
    C among (i-1, j-1), (i-1, j), (i, j-1), ties to the first of that order
    distance = C[N-1, M-1] / L[N-1, M-1] if normalized else C[N-1, M-1]

The definition is this project's own (tests/dtw_f64.py and tests/symkl_f64.py state it in float64); agreement with
the external toolkit, its KL divergence included, is not pinned (DESIGN sections 4.14 and 4.16).
"""

import numpy as np

from shennong_amd import _backend
from shennong_amd.device import DeviceFeaturesCollection

__all__ = ['dtw_distances', 'MAX_FRAMES']

MAX_FRAMES = _backend.DTW_MAX_FRAMES


def _centres(times):
    """Centre time of every row: the mean of a [n, 2] (start, stop) row, the value of a [n] one"""
    times = np.asarray(times, dtype=np.float64)
    return times.mean(axis=1) if times.ndim == 2 else times


def _layout(features):
    """(name -> first row, dim, device block or None) of the one block the rows lie in, or would lie in after
    ``DeviceFeaturesCollection.from_host``; ValueError for different ndims or several device blocks"""
    if isinstance(features, DeviceFeaturesCollection):
        features._alive()
        dims = sorted({block.dim for block in features._blocks})
        if len(dims) > 1:
            raise ValueError('items have different ndims: {}'.format(dims))
        if len(features._blocks) > 1:
            raise ValueError('the utterances lie in {} device blocks (one per sample rate): DTW distances are '
                             'made of one block'.format(len(features._blocks)))
        if not features._blocks:
            return {}, 0, None
        block = features._blocks[0]
        return dict(zip(block.names, block.foff[:-1].tolist())), block.dim, block
    dims = sorted({feats.ndims for feats in features.values() if feats.nframes})
    if len(dims) > 1:
        raise ValueError('items have different ndims: {}'.format(dims))
    first, row = {}, 0
    for name, feats in features.items():   # (the row order of from_host)
        first[name] = row
        row += feats.nframes
    return first, dims[0] if dims else 0, None


def _select(features, pairs, items):
    """(first row, row count) of every item and the pairs as an int32 array [P, 2] into them, all checked"""
    first_of, dim, block = _layout(features)
    if items is None:
        # every utterance named by a pair is an item, in the order of first appearance
        pairs = [tuple(pair) for pair in pairs]
        if any(len(pair) != 2 for pair in pairs):
            raise ValueError('pairs must be pairs of utterance names')
        index, names = {}, []
        for pair in pairs:
            for name in pair:
                if name not in index:
                    if name not in first_of:
                        raise ValueError(f'utterance "{name}" is not in the collection')
                    index[name] = len(names)
                    names.append(name)
        first = np.array([first_of[name] for name in names], dtype=np.int64)
        count = np.array([features[name].nframes for name in names], dtype=np.int64)
        what = ['utterance "{}"'.format(name) for name in names]
        pairs = np.array([(index[a], index[b]) for a, b in pairs], dtype=np.int32).reshape(-1, 2)
    else:
        items = list(items)
        first = np.zeros(len(items), dtype=np.int64)
        count = np.zeros(len(items), dtype=np.int64)
        centres = {}
        for k, item in enumerate(items):
            name, onset, offset = item
            if name not in first_of:
                raise ValueError(f'item {k}: utterance "{name}" is not in the collection')
            if name not in centres:
                centres[name] = _centres(features[name].times)
            lo = int(np.searchsorted(centres[name], float(onset), side='left'))
            hi = int(np.searchsorted(centres[name], float(offset), side='right'))
            first[k], count[k] = first_of[name] + lo, max(hi - lo, 0)
        what = ['item {} ("{}", {}, {})'.format(k, *item) for k, item in enumerate(items)]
        pairs = np.asarray(pairs)
        if pairs.size == 0:
            pairs = np.zeros((0, 2), dtype=np.int32)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in 'iu':
            raise ValueError('pairs must be an integer array [P, 2] of indices into items')
        bad = np.argwhere((pairs < 0) | (pairs >= len(items)))
        if bad.size:
            p = int(bad[0, 0])
            raise ValueError('pair {} ({}, {}) is out of range for {} items'.format(
                p, int(pairs[p, 0]), int(pairs[p, 1]), len(items)))
        pairs = pairs.astype(np.int32)
    for k in np.flatnonzero(count < 1).tolist()[:1]:
        raise ValueError('{} has no frames'.format(what[k]))
    for k in np.flatnonzero(count > MAX_FRAMES).tolist()[:1]:
        raise ValueError('{} has {} frames, the limit is {}'.format(what[k], int(count[k]), MAX_FRAMES))
    return first, count.astype(np.int32), pairs, dim, block


def dtw_distances(features, pairs, items=None, metric='cosine', normalized=True, return_lengths=False):
    """DTW distances of pairs of items of `features`, a float32 array [P] in the order of `pairs`

    `features`: a :class:`DeviceFeaturesCollection` (the rows are used where they lie), or a host
    :class:`FeaturesCollection`, uploaded once (``DeviceFeaturesCollection.from_host``).
    `items` None: every utterance is one item and `pairs` holds pairs of names.  Otherwise a sequence of
    ``(name, onset, offset)`` in seconds - an item is the run of rows whose centre time lies in
    [onset, offset] - and `pairs` is an integer array [P, 2] into it.
    `metric`: 'cosine', 'sqeuclidean' or 'symkl' (the module's docstring).  `normalized`: the cost divided by the length of the path (float32
    division on the host; the kernel writes both).  `return_lengths`: ``(distances, lengths)``, lengths int32.

    ValueError, before any device work: an unknown metric, a name that is not in the collection, an index out of
    range, an item without frames or of more than ``MAX_FRAMES`` frames, items of different ndims, a collection
    in several device blocks."""
    if metric not in _backend.DTW_METRICS:
        raise ValueError('invalid metric "{}", choose in "{}"'.format(metric, ', '.join(_backend.DTW_METRICS)))
    first, count, pairs, dim, block = _select(features, pairs, items)
    n_pairs = pairs.shape[0]
    cost = np.zeros(n_pairs, dtype=np.float32)
    lengths = np.zeros(n_pairs, dtype=np.int32)
    if n_pairs:
        owned = None
        if block is None:
            owned = DeviceFeaturesCollection.from_host(features)
            block = owned._blocks[0]
        try:
            buffer = block.alive()
            d_cost = _backend.DeviceBuffer(4 * n_pairs, buffer.device)
            d_len = _backend.DeviceBuffer(4 * n_pairs, buffer.device)
            try:
                _backend.dtw_pairs(buffer.ptr, dim, first, count, pairs, metric, d_cost.ptr, d_len.ptr,
                                   device=buffer.device)
                d_cost.download(cost)
                d_len.download(lengths)
            finally:
                d_cost.free()
                d_len.free()
        finally:
            if owned is not None:
                owned.release()
    distances = cost / lengths.astype(np.float32) if normalized and n_pairs else cost
    return (distances, lengths) if return_lengths else distances
