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

:func:`dtw_search` is the other classic use of the same rows, query-by-example search: where does a short query
occur inside whole utterances?  The same lattice with a free start and a free end in the target (subsequence DTW,
snf_dtw_search; its docstring has the definition, DESIGN section 4.17 the rest):

    found = dtw_search(feats, queries=[('utt1', 0.31, 0.52)], targets=['utt2', 'utt3'])    # a DtwMatches
    best = found.ranked(0)[0]                         # the pair of query 0 with the smallest score
    found.target[best], found.onset[best], found.offset[best]

:func:`dtw_detect` finds every place a query occurs in a target, not only the best one, and the best few hits of a
query over a whole corpus, all picked on the device (snf_dtw_detect, snf_dtw_topk):

    hits = dtw_detect(feats, queries, targets, max_detections=4, top_k=10)                  # a DtwDetections
    rows = hits.ranked(0)                             # the rows of query 0, the best first
    hits.target[rows], hits.onset[rows], hits.offset[rows]

:func:`dtw_align` returns the alignment itself, the warping path of every pair, walked back on the device from the
decisions that the lattice takes anyway (snf_dtw_align); ``dtw_search`` and ``dtw_detect`` give
the paths of their hits with ``return_paths=True``:

    paths = dtw_align(feats, [(0, 1), (0, 2)], items=items)            # a DtwPaths
    paths.path(0)                                     # int32 [L, 2]: (frame of item 0, frame of item 1) per cell
    paths.y_range_of_x(0)                             # per frame of item 0 the first and last frame matched to it
    found = dtw_search(feats, queries, targets, return_paths=True)
    found.path(best)                                  # (query frame, target frame) of the best match's cells
"""

import numpy as np

from shennong_amd import _backend
from shennong_amd.device import DeviceFeaturesCollection

__all__ = ['dtw_distances', 'dtw_search', 'dtw_detect', 'dtw_align', 'DtwMatches', 'DtwDetections', 'DtwPaths',
           'MAX_FRAMES']

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


def _item_rows(features, first_of, centres, kind, k, item):
    """(first row in the block, row count) of the item ``(name, onset, offset)``: the run of rows of the utterance
    whose centre time lies in [onset, offset].  `centres` caches the centre times per name; `kind` and `k` name the
    item in the error ('item 3', 'query 0')"""
    name, onset, offset = item
    if name not in first_of:
        raise ValueError(f'{kind} {k}: utterance "{name}" is not in the collection')
    if name not in centres:
        centres[name] = _centres(features[name].times)
    lo = int(np.searchsorted(centres[name], float(onset), side='left'))
    hi = int(np.searchsorted(centres[name], float(offset), side='right'))
    return first_of[name] + lo, max(hi - lo, 0)


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
            first[k], count[k] = _item_rows(features, first_of, centres, 'item', k, item)
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


class _PathStore:
    """The paths of the rows of a result, concatenated: row k owns the elements first[k] .. first[k + 1] of `x` and
    `y` (int32 frames, counted from the first row of each item).  `centres`: per item the centre times of its rows,
    `x_item`, `y_item`: the items of every row (or None: no times)"""

    def __init__(self, first, x, y, centres=None, x_item=None, y_item=None):
        self.first = np.asarray(first, dtype=np.int64)
        self.x = np.asarray(x, dtype=np.int32)
        self.y = np.asarray(y, dtype=np.int32)
        if self.first.ndim != 1 or self.first.shape[0] < 1 or self.first[0] != 0 or (np.diff(self.first) < 0).any():
            raise ValueError('first must hold ascending offsets [rows + 1] from 0')
        if self.x.shape != self.y.shape or self.x.ndim != 1 or self.x.shape[0] != self.first[-1]:
            raise ValueError('x_frame and y_frame must hold the {} frames that first counts'.format(
                int(self.first[-1])))
        self.centres, self.x_item, self.y_item = centres, x_item, y_item

    def __len__(self):
        return self.first.shape[0] - 1

    def bounds(self, k, what):
        if not -len(self) <= k < len(self):
            raise IndexError('{} {} is out of range for {}'.format(what, k, len(self)))
        k = k % len(self)
        return k, int(self.first[k]), int(self.first[k + 1])

    def path(self, k, what):
        _, lo, hi = self.bounds(k, what)
        return np.stack([self.x[lo:hi], self.y[lo:hi]], axis=1)

    def times(self, k, what):
        if self.centres is None:
            raise ValueError('no times: the paths were not made from a collection')
        k, lo, hi = self.bounds(k, what)
        return np.stack([self.centres[self.x_item[k]][self.x[lo:hi]],
                         self.centres[self.y_item[k]][self.y[lo:hi]]], axis=1)


def _item_centres(features, names, rows, count):
    """Per item the centre times of its rows: item k is `count[k]` rows of utterance `names[k]` from its row
    `rows[k]`"""
    whole = {}
    for name in set(names):
        whole[name] = _centres(features[name].times)
    return [whole[name][lo:lo + n] for name, lo, n in zip(names, rows, count)]


def _compact(path_first, length, x, y):
    """(first [S + 1], x, y): the first length[s] elements from path_first[s] of `x` and `y`, one stretch behind the
    other"""
    length = np.asarray(length, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    at = np.repeat(np.asarray(path_first, dtype=np.int64) - first[:-1], length) + np.arange(first[-1])
    return first, x[at], y[at]


def _aligned(buffer, dim, first, count, index_pairs, metric, mode, normalized=True, slots=1, max_score=None,
             scratch_bytes=0):
    """One snf_dtw_align over `index_pairs` [P, 2]: (counts [P], cost, length, start, end [P * slots], path_first
    [P * slots], x, y) on the host; every slot owns N + M - 1 elements of x and y"""
    n_pairs = index_pairs.shape[0]
    room = (count[index_pairs[:, 0]].astype(np.int64) + count[index_pairs[:, 1]] - 1).repeat(slots)
    path_first = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    total = int(path_first[-1])
    if total >= 2 ** 31:
        raise ValueError('the paths of the {} pairs need room for {} cells, the limit is 2^31 - 1: align in parts'
                         .format(n_pairs, total))
    counts = np.ones(n_pairs, dtype=np.int32)
    cost = np.zeros(n_pairs * slots, dtype=np.float32)
    length, start, end = (np.zeros(n_pairs * slots, dtype=np.int32) for _ in range(3))
    x, y = np.zeros(total, dtype=np.int32), np.zeros(total, dtype=np.int32)
    buffers = []
    try:
        sizes = (n_pairs,) + (n_pairs * slots,) * 4 + (total,) * 2
        for size in sizes:
            buffers.append(_backend.DeviceBuffer(4 * max(size, 1), buffer.device))
        d_count, d_cost, d_len, d_start, d_end, d_x, d_y = (b.ptr for b in buffers)
        _backend.dtw_align(buffer.ptr, dim, first, count, index_pairs, metric, mode, d_cost, d_len, path_first[:-1],
                           d_x, d_y, normalized=normalized, max_detections=slots, max_score=max_score,
                           d_count=d_count, d_start=d_start, d_end=d_end, scratch_bytes=scratch_bytes,
                           device=buffer.device)
        outs = (cost, length, x, y) if mode == 'global' else (counts, cost, length, start, end, x, y)
        which = (1, 2, 5, 6) if mode == 'global' else range(7)
        for k, out in zip(which, outs):
            if out.size:
                buffers[k].download(out)
    finally:
        for b in buffers:
            b.free()
    return counts, cost, length, start, end, path_first[:-1], x, y


class DtwPaths:
    """The warping paths of a :func:`dtw_align`: numpy columns [P] in the order of the pairs, and the paths
    concatenated

    `cost` (float32), `length` (int32): C and L of the end cell, as ``dtw_distances`` has them; `distance`
    (float32): ``cost / length`` if normalized, else the cost.  `first` (int64 [P + 1]): pair p owns the elements
    first[p] .. first[p + 1] of `x_frame` and `y_frame` (int32), the frames of the cells of its path from (0, 0) to
    (N-1, M-1), counted from the first row of each item."""

    def __init__(self, cost, length, first, x_frame, y_frame, normalized=True, centres=None, pairs=None):
        self.cost = np.asarray(cost, dtype=np.float32)
        self.length = np.asarray(length, dtype=np.int32)
        if self.cost.ndim != 1 or self.cost.shape != self.length.shape:
            raise ValueError('cost and length must be one-dimensional and of one length')
        pairs = None if pairs is None else np.asarray(pairs).reshape(-1, 2)
        self._store = _PathStore(first, x_frame, y_frame, centres, None if pairs is None else pairs[:, 0],
                                 None if pairs is None else pairs[:, 1])
        if len(self._store) != self.cost.shape[0] or (np.diff(self._store.first) != self.length).any():
            raise ValueError('first must count length[p] cells for every one of the {} pairs'.format(
                self.cost.shape[0]))
        self.first, self.x_frame, self.y_frame = self._store.first, self._store.x, self._store.y
        self.normalized = bool(normalized)
        self.distance = (self.cost / self.length.astype(np.float32) if self.normalized and len(self)
                         else self.cost.copy())

    def __len__(self):
        return self.cost.shape[0]

    def path(self, p):
        """int32 [L, 2]: (frame of x, frame of y) of every cell of the path of pair `p`, forward"""
        return self._store.path(p, 'pair')

    def times(self, p):
        """float64 [L, 2]: the centre times in seconds of the two frames of every cell (the mean of a [n, 2] (start,
        stop) row of the utterance's times, the value of a [n] one)"""
        return self._store.times(p, 'pair')

    def y_range_of_x(self, p):
        """int32 [N, 2]: per frame of x the first and the last frame of y that the path of pair `p` matches to it"""
        path = self.path(p)
        x, y = path[:, 0], path[:, 1]
        turn = np.flatnonzero(np.diff(x))   # (x does not descend and leaves no frame out)
        return np.stack([y[np.concatenate([[0], turn + 1])], y[np.concatenate([turn, [x.shape[0] - 1]])]],
                        axis=1).astype(np.int32)

    def save_csv(self, path):
        """Writes the cells to `path`: a header line ``pair,x_frame,y_frame``, then one line per cell, pair by pair"""
        pair = np.repeat(np.arange(len(self)), np.diff(self.first))
        with open(path, 'w') as out:
            out.write('pair,x_frame,y_frame\n')
            for row in zip(pair.tolist(), self.x_frame.tolist(), self.y_frame.tolist()):
                out.write('{},{},{}\n'.format(*row))


def dtw_align(features, pairs, items=None, metric='cosine', normalized=True, scratch_bytes=0):
    """The warping paths of pairs of items of `features` (snf_dtw_align), a :class:`DtwPaths`

    The lattice, `features`, `pairs`, `items`, `metric` and `normalized` are those of :func:`dtw_distances`, and so
    are cost and length, bit for bit.  Every cell also keeps which predecessor it took - (i-1, j-1), (i-1, j) or
    (i, j-1): the one of smallest C, ties to the first of that order - and the path of a pair follows these
    decisions back from (N-1, M-1) to (0, 0); it has exactly `length` cells.  The walk runs on the device, behind
    the lattice; the definition is this project's own (tests/dtw_align_f64.py states it in float64).
    `scratch_bytes`: the bound on the device memory that holds the decisions, 16 bytes per step of every strip of 64
    rows (0: 1 GiB); the pairs are worked in as many runs as that takes.

    ValueError, before any device work: what ``dtw_distances`` raises, paths that need room for 2^31 cells or more,
    a `scratch_bytes` below the need of the largest pair."""
    if metric not in _backend.DTW_METRICS:
        raise ValueError('invalid metric "{}", choose in "{}"'.format(metric, ', '.join(_backend.DTW_METRICS)))
    if items is None:
        pairs = [tuple(pair) for pair in pairs]
    else:
        items = list(items)
    given = pairs
    first, count, pairs, dim, block = _select(features, pairs, items)
    n_pairs = pairs.shape[0]
    if not _int_in(scratch_bytes, 0, 2 ** 62):
        raise ValueError('scratch_bytes must be a non-negative int, not {!r}'.format(scratch_bytes))
    if n_pairs and scratch_bytes:
        need = int(_backend.dtw_record_bytes(count[pairs[:, 0]], count[pairs[:, 1]]).max())
        if scratch_bytes < need:
            raise ValueError('scratch_bytes {} is below the {} bytes that the largest pair needs'.format(
                scratch_bytes, need))
    # the centre times of the rows of every item (items None: the utterances in the order of first appearance)
    first_of, _, _ = _layout(features)
    names = (list(dict.fromkeys(name for pair in given for name in pair)) if items is None
             else [item[0] for item in items])
    rows = [int(row) - first_of[name] for row, name in zip(first.tolist(), names)]
    centres = _item_centres(features, names, rows, count.tolist())
    if not n_pairs:
        return DtwPaths(np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32),
                        np.zeros(0, np.int32), normalized, centres, pairs)
    owned = None
    if block is None:
        owned = DeviceFeaturesCollection.from_host(features)
        block = owned._blocks[0]
    try:
        _, cost, length, _, _, path_first, x, y = _aligned(block.alive(), dim, first, count, pairs, metric, 'global',
                                                           scratch_bytes=scratch_bytes)
    finally:
        if owned is not None:
            owned.release()
    return DtwPaths(cost, length, *_compact(path_first, length, x, y), normalized=normalized, centres=centres,
                    pairs=pairs)


class DtwMatches:
    """The best match of every (query, target) pair of a :func:`dtw_search`: numpy columns [P] in the order of
    the pairs

    `query`, `target` (int32): indices into the queries and the targets of the call.  `score`, `cost` (float32):
    the score of the best end (the cost over the length if normalized, else the cost) and the cost of its path.
    `length`, `start_frame`, `end_frame` (int32): the cells of the path, its first and its last frame, counted from
    the first row of the target item.  `onset`, `offset` (float64 seconds): the start time of the start row and
    the stop time of the end row of the target utterance ([n, 2] times), or their single time ([n] times)."""

    columns = ('query', 'target', 'score', 'cost', 'length', 'start_frame', 'end_frame', 'onset', 'offset')

    def __init__(self, query, target, score, cost, length, start_frame, end_frame, onset, offset, curves=None,
                 paths=None):
        self.query = np.asarray(query, dtype=np.int32)
        self.target = np.asarray(target, dtype=np.int32)
        self.score = np.asarray(score, dtype=np.float32)
        self.cost = np.asarray(cost, dtype=np.float32)
        self.length = np.asarray(length, dtype=np.int32)
        self.start_frame = np.asarray(start_frame, dtype=np.int32)
        self.end_frame = np.asarray(end_frame, dtype=np.int32)
        self.onset = np.asarray(onset, dtype=np.float64)
        self.offset = np.asarray(offset, dtype=np.float64)
        sizes = {getattr(self, name).shape for name in self.columns}
        if len(sizes) != 1 or len(next(iter(sizes))) != 1:
            raise ValueError('the columns must be one-dimensional and of one length: {}'.format(sorted(sizes)))
        # (first [P + 1], cost, length, start): pair p owns the elements first[p] .. first[p + 1] of the three
        self._curves = curves
        self._paths = paths   # (a _PathStore with one path per pair, or None)

    def __len__(self):
        return self.query.shape[0]

    def path(self, p):
        """int32 [length, 2]: (query frame, target frame) of every cell of the path of the match of pair `p`, from
        (0, start_frame) to (N-1, end_frame); the target frames are counted as `start_frame` is.  ValueError when
        the search did not ask for paths"""
        if self._paths is None:
            raise ValueError('no paths: call dtw_search with return_paths=True')
        return self._paths.path(p, 'pair')

    def times(self, p):
        """float64 [length, 2]: the centre times in seconds of the query frame and the target frame of every cell of
        the path of pair `p`"""
        if self._paths is None:
            raise ValueError('no paths: call dtw_search with return_paths=True')
        return self._paths.times(p, 'pair')

    def curve(self, p):
        """``(cost [M], length [M], start [M])`` of pair `p`: C, L and B of the path that ends at every frame of the
        target (the score of an end is ``cost / length`` in float32, or ``cost``).  The material for several
        detections per pair.  ValueError when the search did not ask for curves"""
        if self._curves is None:
            raise ValueError('no curves: call dtw_search with return_curves=True')
        if not -len(self) <= p < len(self):
            raise IndexError('pair {} is out of range for {} pairs'.format(p, len(self)))
        first, cost, length, start = self._curves
        p = p % len(self)
        lo, hi = int(first[p]), int(first[p + 1])
        return cost[lo:hi], length[lo:hi], start[lo:hi]

    def ranked(self, query):
        """The indices of the pairs of query `query` by ascending score, equal scores in the order of the pairs"""
        mine = np.flatnonzero(self.query == query)
        return mine[np.argsort(self.score[mine], kind='stable')]


def _select_search(features, queries, targets, pairs):
    """The queries then the targets as items (first row, row count), the pairs as an int32 array [P, 2] of (query
    index, target index), and per target its utterance and its first row in it - all checked"""
    first_of, dim, block = _layout(features)
    centres = {}
    first, count, what, where = [], [], [], []
    sizes = []
    for kind, entries in (('query', queries), ('target', targets)):
        entries = list(entries)
        sizes.append(len(entries))
        for k, entry in enumerate(entries):
            if isinstance(entry, str):
                if entry not in first_of:
                    raise ValueError(f'{kind} {k}: utterance "{entry}" is not in the collection')
                name, rows = entry, (first_of[entry], features[entry].nframes)
                what.append('{} {} ("{}")'.format(kind, k, entry))
            else:
                entry = tuple(entry)
                if len(entry) != 3:
                    raise ValueError('{} {}: not an utterance name or (name, onset, offset): {}'.format(kind, k, entry))
                name, rows = entry[0], _item_rows(features, first_of, centres, kind, k, entry)
                what.append('{} {} ("{}", {}, {})'.format(kind, k, *entry))
            first.append(rows[0])
            count.append(rows[1])
            where.append((name, rows[0] - first_of[name]))
    n_queries, n_targets = sizes
    if pairs is None:   # every query against every target, query-major
        pairs = np.stack(np.meshgrid(np.arange(n_queries), np.arange(n_targets), indexing='ij'), axis=-1)
        pairs = pairs.reshape(-1, 2)
    else:
        pairs = np.asarray(pairs)
        if pairs.size == 0:
            pairs = np.zeros((0, 2), dtype=np.int32)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in 'iu':
            raise ValueError('pairs must be an integer array [P, 2] of (query index, target index)')
        bad = np.argwhere((pairs < 0) | (pairs >= np.array([n_queries, n_targets])))
        if bad.size:
            p = int(bad[0, 0])
            raise ValueError('pair {} ({}, {}) is out of range for {} queries and {} targets'.format(
                p, int(pairs[p, 0]), int(pairs[p, 1]), n_queries, n_targets))
    pairs = pairs.astype(np.int32)
    count = np.array(count, dtype=np.int64)
    for k in np.flatnonzero(count < 1).tolist()[:1]:
        raise ValueError('{} has no frames'.format(what[k]))
    for k in np.flatnonzero(count > MAX_FRAMES).tolist()[:1]:
        raise ValueError('{} has {} frames, the limit is {}'.format(what[k], int(count[k]), MAX_FRAMES))
    return (np.array(first, dtype=np.int64), count.astype(np.int32), pairs, n_queries, where[n_queries:], dim, block)


def _times(features, where, target, start, end):
    """(onset, offset) in seconds of the paths from frame `start` to frame `end` of the targets `target` (indices
    into `where`, which ``_select_search`` returns): the start time of the start row and the stop time of the end
    row of the target's utterance ([n, 2] times), or their single time ([n] times)"""
    # the start and stop times of the targets' utterances laid end to end, and per target the place of its first
    # row in them
    placed, begins, ends, rows = {}, [np.zeros(0)], [np.zeros(0)], 0
    base = np.zeros(len(where), dtype=np.int64)
    for t, (name, row) in enumerate(where):
        if name not in placed:
            stamps = np.asarray(features[name].times, dtype=np.float64)
            begins.append(stamps[:, 0] if stamps.ndim == 2 else stamps)
            ends.append(stamps[:, 1] if stamps.ndim == 2 else stamps)
            placed[name] = rows
            rows += stamps.shape[0]
        base[t] = placed[name] + row
    at = base[target] if len(target) else np.zeros(0, dtype=np.int64)
    return np.concatenate(begins)[at + start], np.concatenate(ends)[at + end]


def _entry_centres(features, entries, first, count):
    """Per query and target (`entries`, the queries then the targets) the centre times of its rows"""
    first_of, _, _ = _layout(features)
    names = [entry if isinstance(entry, str) else tuple(entry)[0] for entry in entries]
    rows = [int(row) - first_of[name] for row, name in zip(first.tolist(), names)]
    return _item_centres(features, names, rows, count.tolist())


def _hit_paths(buffer, dim, first, count, index_pairs, metric, normalized, slots, max_score, want, found):
    """The paths of the detections `want` = (pair [R], rank [R]) by a second pass over their distinct pairs alone
    (snf_dtw_align, which keeps the decisions of the lattice): (first [R + 1], x, y).  `found` = (length, start, end)
    [R] of the first pass, which the second must find again"""
    pair, rank = want
    distinct, place = np.unique(pair, return_inverse=True)
    _, _, length, start, end, path_first, x, y = _aligned(buffer, dim, first, count, index_pairs[distinct], metric,
                                                          'subsequence', normalized, slots, max_score)
    slot = place.reshape(-1) * slots + rank
    if not all(np.array_equal(a[slot], b) for a, b in zip((length, start, end), found)):
        raise RuntimeError('dtw: internal error, the alignment pass found other detections than the search')
    return _compact(path_first[slot], length[slot], x, y)


def dtw_search(features, queries, targets, pairs=None, metric='cosine', normalized=True, return_curves=False,
               return_paths=False):
    """Query-by-example search: where does every query occur in every target?  Subsequence DTW on the GPU
    (snf_dtw_search), a :class:`DtwMatches` with the best match of every (query, target) pair

    For the query x [N, D] and the target y [M, D] of a pair, with d[i, j] the frame distance of the module's
    docstring, the start and the end of the path in the target are free:

        C[0, j] = d[0, j], L[0, j] = 1, B[0, j] = j for every j
        i >= 1: C[i, j] = d[i, j] + C[p], L[i, j] = L[p] + 1, B[i, j] = B[p], p the predecessor of smallest C among
        (i-1, j-1), (i-1, j), (i, j-1) that exist, ties to the first of that order
        score[j] = C[N-1, j] / L[N-1, j] (float32 division) if normalized else C[N-1, j]
        end_frame = the smallest j of minimal score, start_frame = B[N-1, end_frame], cost and length of that cell

    As in :func:`dtw_distances` the dynamic programme minimises the cost C; the normalisation only ranks the ends,
    it does not look for the path of smallest mean.  The definition is this project's own (tests/dtw_search_f64.py
    states it in float64); agreement with any outside toolkit is not pinned.

    `features`: a :class:`DeviceFeaturesCollection` (the rows are used where they lie), or a host
    :class:`FeaturesCollection`, uploaded once.  Queries and targets lie in the one collection: a user with keyword
    examples from elsewhere builds one collection of both.
    `queries`, `targets`: sequences whose entries are an utterance name (all of its rows) or ``(name, onset,
    offset)`` in seconds (the run of rows whose centre time lies in [onset, offset], as the items of
    ``dtw_distances``).
    `pairs` None: every query against every target, query-major.  Otherwise an integer array [P, 2] of (query
    index, target index).
    `return_curves`: keep (C, L, B) of every end of every pair for ``DtwMatches.curve``.
    `return_paths`: keep the warping path of every match for ``DtwMatches.path`` and ``DtwMatches.times``, by a
    second pass that records the decisions of the lattice (snf_dtw_align; :func:`dtw_align` has the definition).

    ValueError, before any device work: an unknown metric, a name that is not in the collection, an index out of
    range, an item without frames or of more than ``MAX_FRAMES`` frames, items of different ndims, a collection in
    several device blocks, curves of 2^31 elements or more."""
    if metric not in _backend.DTW_METRICS:
        raise ValueError('invalid metric "{}", choose in "{}"'.format(metric, ', '.join(_backend.DTW_METRICS)))
    queries, targets = list(queries), list(targets)
    first, count, pairs, n_queries, where, dim, block = _select_search(features, queries, targets, pairs)
    n_pairs = pairs.shape[0]
    columns = count[n_queries + pairs[:, 1]].astype(np.int64)   # M of every pair
    curve_first = np.concatenate([[0], np.cumsum(columns)]).astype(np.int64)
    total = int(curve_first[-1])
    if return_curves and total >= 2 ** 31:
        raise ValueError('the curves of the {} pairs hold {} elements, the limit is 2^31 - 1: search in parts'.format(
            n_pairs, total))
    cost = np.zeros(n_pairs, dtype=np.float32)
    length, start, end = (np.zeros(n_pairs, dtype=np.int32) for _ in range(3))
    curves = None
    paths = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    if return_curves:
        curves = (curve_first, np.zeros(total, dtype=np.float32), np.zeros(total, dtype=np.int32),
                  np.zeros(total, dtype=np.int32))
    if n_pairs:
        owned = None
        if block is None:
            owned = DeviceFeaturesCollection.from_host(features)
            block = owned._blocks[0]
        buffers = []
        try:
            buffer = block.alive()
            for _ in range(4):
                buffers.append(_backend.DeviceBuffer(4 * n_pairs, buffer.device))
            if return_curves:
                for _ in range(3):
                    buffers.append(_backend.DeviceBuffer(4 * total, buffer.device))
            index_pairs = pairs + np.array([0, n_queries], dtype=np.int32)   # (the targets lie behind the queries)
            _backend.dtw_search(buffer.ptr, dim, first, count, index_pairs, metric, normalized,
                                *[b.ptr for b in buffers[:4]],
                                **(dict(curve_first=curve_first[:-1], d_curve_cost=buffers[4].ptr,
                                        d_curve_len=buffers[5].ptr, d_curve_start=buffers[6].ptr)
                                   if return_curves else {}),
                                device=buffer.device)
            for b, out in zip(buffers, (cost, length, start, end) + (curves[1:] if return_curves else ())):
                b.download(out)
            if return_paths:
                paths = _hit_paths(buffer, dim, first, count, index_pairs, metric, normalized, 1, None,
                                   (np.arange(n_pairs), np.zeros(n_pairs, dtype=np.int64)), (length, start, end))
        finally:
            for b in buffers:
                b.free()
            if owned is not None:
                owned.release()
    score = cost / length.astype(np.float32) if normalized and n_pairs else cost.copy()
    onset, offset = _times(features, where, pairs[:, 1], start, end)
    store = None
    if return_paths:
        store = _PathStore(*paths, _entry_centres(features, queries + targets, first, count), pairs[:, 0],
                           n_queries + pairs[:, 1])
    return DtwMatches(pairs[:, 0], pairs[:, 1], score, cost, length, start, end, onset, offset, curves, store)


class DtwDetections:
    """The detections of a :func:`dtw_detect`: numpy columns, one row per detection

    `pair` (int32): the index of the (query, target) pair in the pairs of the call; `query`, `target` (int32): the
    indices of its query and its target; `rank` (int32): 0 for the best detection of the pair, 1 for the next ...
    `score`, `cost` (float32), `length`, `start_frame`, `end_frame` (int32), `onset`, `offset` (float64 seconds): as
    the columns of :class:`DtwMatches`.

    Without `top_k` the rows are in the order of the pairs, then by rank, and `counts` [P] holds the detections of
    every pair.  With `top_k` the rows are in the order of the queries, then by (score, pair, rank), and `counts`
    [Q] holds the rows of every query."""

    columns = ('pair', 'query', 'target', 'rank', 'score', 'cost', 'length', 'start_frame', 'end_frame', 'onset',
               'offset')
    _types = (np.int32, np.int32, np.int32, np.int32, np.float32, np.float32, np.int32, np.int32, np.int32,
              np.float64, np.float64)

    def __init__(self, pair, query, target, rank, score, cost, length, start_frame, end_frame, onset, offset,
                 counts, curves=None, top_k=None, paths=None):
        given = (pair, query, target, rank, score, cost, length, start_frame, end_frame, onset, offset)
        for name, column, dtype in zip(self.columns, given, self._types):
            setattr(self, name, np.asarray(column, dtype=dtype))
        sizes = {getattr(self, name).shape for name in self.columns}
        if len(sizes) != 1 or len(next(iter(sizes))) != 1:
            raise ValueError('the columns must be one-dimensional and of one length: {}'.format(sorted(sizes)))
        self.counts = np.asarray(counts, dtype=np.int32)
        if self.counts.ndim != 1 or int(self.counts.sum()) != len(self):
            raise ValueError('counts must be one-dimensional and sum to the {} rows'.format(len(self)))
        self.top_k = top_k
        # (first [P + 1], cost, length, start): pair p owns the elements first[p] .. first[p + 1] of the three
        self._curves = curves
        self._paths = paths   # (a _PathStore with one path per row, or None)

    def __len__(self):
        return self.pair.shape[0]

    def path(self, k):
        """int32 [length, 2]: (query frame, target frame) of every cell of the path of the detection of row `k`,
        from (0, start_frame) to (N-1, end_frame).  ValueError when the call did not ask for paths"""
        if self._paths is None:
            raise ValueError('no paths: call dtw_detect with return_paths=True')
        return self._paths.path(k, 'row')

    def times(self, k):
        """float64 [length, 2]: the centre times in seconds of the query frame and the target frame of every cell of
        the path of row `k`"""
        if self._paths is None:
            raise ValueError('no paths: call dtw_detect with return_paths=True')
        return self._paths.times(k, 'row')

    def of_pair(self, p):
        """The rows of pair `p`, by ascending rank"""
        return np.flatnonzero(self.pair == p)

    def ranked(self, query):
        """The rows of query `query` by ascending (score, pair, rank)"""
        mine = np.flatnonzero(self.query == query)
        mine = mine[np.lexsort((self.rank[mine], self.pair[mine]))]
        return mine[np.argsort(self.score[mine], kind='stable')]

    def curve(self, p):
        """``(cost [M], length [M], start [M])`` of pair `p`, as ``DtwMatches.curve``: what the detections of the
        pair were picked from.  ValueError when the call did not ask for curves"""
        if self._curves is None:
            raise ValueError('no curves: call dtw_detect with return_curves=True')
        first, cost, length, start = self._curves
        n_pairs = first.shape[0] - 1
        if not -n_pairs <= p < n_pairs:
            raise IndexError('pair {} is out of range for {} pairs'.format(p, n_pairs))
        p = p % n_pairs
        lo, hi = int(first[p]), int(first[p + 1])
        return cost[lo:hi], length[lo:hi], start[lo:hi]

    def save_csv(self, path):
        """Writes the rows to `path`: a header line with the names of the columns, then one line per detection
        (floats with the digits that give the same value back)"""
        with open(path, 'w') as out:
            out.write(','.join(self.columns) + '\n')
            values = [getattr(self, name).tolist() for name in self.columns]
            for row in zip(*values):
                out.write(','.join(repr(v) for v in row) + '\n')


def _int_in(value, lo, hi):
    return isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_)) and lo <= value <= hi


def dtw_detect(features, queries, targets, pairs=None, metric='cosine', normalized=True, max_detections=4,
               max_score=None, top_k=None, return_curves=False, return_paths=False):
    """Query-by-example detection: every place a query occurs in a target, not only the best one (snf_dtw_detect), and
    per query the best few over all its targets (snf_dtw_topk); a :class:`DtwDetections`

    The lattice, the score of an end and the arguments `features`, `queries`, `targets`, `pairs`, `metric`,
    `normalized` and `return_curves` are those of :func:`dtw_search`.  The detections of a pair are a greedy
    non-maximum suppression over its ends; every end is alive at first, and then, at most `max_detections` times:

        e = the smallest alive end of minimal score; stop if `max_score` is given and not score[e] <= max_score
        (a float32 comparison); (score, cost, length, start, end) of e is the detection of the next rank; every end
        whose path interval [start, end] shares a frame with that of e is no longer alive

    So the detections of a pair come in ascending score, their intervals in the target are pairwise disjoint, and
    rank 0 is the match of ``dtw_search``.  The definition is this project's own (tests/dtw_detect_f64.py states
    it); agreement with any outside toolkit is not pinned.

    `top_k` T: per query only its T best detections, by (score ascending, pair index, rank), are selected on the
    device and downloaded - Q T records instead of P max_detections.
    `return_paths`: keep the warping path of every row for ``DtwDetections.path`` and ``DtwDetections.times``, by a
    second pass (snf_dtw_align) over the distinct pairs of the rows alone: with `top_k`, of the surviving detections.

    ValueError, before any device work: what ``dtw_search`` raises, `max_detections` not an int in [1, 64], `top_k`
    not an int in [1, 1024], a NaN `max_score`, `top_k` together with `return_curves`."""
    if metric not in _backend.DTW_METRICS:
        raise ValueError('invalid metric "{}", choose in "{}"'.format(metric, ', '.join(_backend.DTW_METRICS)))
    if not _int_in(max_detections, 1, _backend.DTW_MAX_DETECTIONS):
        raise ValueError('max_detections must be an int in [1, {}], not {!r}'.format(
            _backend.DTW_MAX_DETECTIONS, max_detections))
    if top_k is not None and not _int_in(top_k, 1, _backend.DTW_MAX_TOPK):
        raise ValueError('top_k must be None or an int in [1, {}], not {!r}'.format(_backend.DTW_MAX_TOPK, top_k))
    if max_score is not None:
        max_score = float(max_score)
        if max_score != max_score:
            raise ValueError('max_score must be None or a number, not {!r}'.format(max_score))
    if top_k is not None and return_curves:
        raise ValueError('top_k={} with return_curves=True: the curves are per pair, ask for them without top_k'
                         .format(top_k))
    queries, targets = list(queries), list(targets)
    first, count, pairs, n_queries, where, dim, block = _select_search(features, queries, targets, pairs)
    n_pairs, k = pairs.shape[0], int(max_detections)
    columns = count[n_queries + pairs[:, 1]].astype(np.int64)   # M of every pair
    curve_first = np.concatenate([[0], np.cumsum(columns)]).astype(np.int64)
    total = int(curve_first[-1])
    if return_curves and total >= 2 ** 31:
        raise ValueError('the curves of the {} pairs hold {} elements, the limit is 2^31 - 1: search in parts'.format(
            n_pairs, total))
    # what comes down: per pair k slots, or per query top_k places
    groups, slots = (n_pairs, k) if top_k is None else (n_queries, int(top_k))
    counts = np.zeros(groups, dtype=np.int32)
    cost = np.zeros(groups * slots, dtype=np.float32)
    length, start, end = (np.zeros(groups * slots, dtype=np.int32) for _ in range(3))
    top_pair, top_rank = (np.zeros(groups * slots, dtype=np.int32) for _ in range(2))
    curves = None
    paths = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    if return_curves:
        curves = (curve_first, np.zeros(total, dtype=np.float32), np.zeros(total, dtype=np.int32),
                  np.zeros(total, dtype=np.int32))
    if n_pairs:
        owned = None
        if block is None:
            owned = DeviceFeaturesCollection.from_host(features)
            block = owned._blocks[0]
        buffers = []
        try:
            buffer = block.alive()
            buffers.append(_backend.DeviceBuffer(4 * n_pairs, buffer.device))
            for _ in range(4):
                buffers.append(_backend.DeviceBuffer(4 * n_pairs * k, buffer.device))
            if return_curves:
                for _ in range(3):
                    buffers.append(_backend.DeviceBuffer(4 * total, buffer.device))
            index_pairs = pairs + np.array([0, n_queries], dtype=np.int32)   # (the targets lie behind the queries)
            _backend.dtw_detect(buffer.ptr, dim, first, count, index_pairs, metric, normalized, k, max_score,
                                *[b.ptr for b in buffers[:5]],
                                **(dict(curve_first=curve_first[:-1], d_curve_cost=buffers[5].ptr,
                                        d_curve_len=buffers[6].ptr, d_curve_start=buffers[7].ptr)
                                   if return_curves else {}),
                                device=buffer.device)
            if top_k is None:
                for b, out in zip(buffers, (counts, cost, length, start, end) + (curves[1:] if return_curves else ())):
                    b.download(out)
            else:
                # the pairs grouped by query, in the caller's order within a query; the detections stay where they are
                order = np.argsort(pairs[:, 0], kind='stable').astype(np.int32)
                bounds = np.concatenate([[0], np.cumsum(np.bincount(pairs[:, 0], minlength=n_queries))])
                best = [_backend.DeviceBuffer(4 * n_queries, buffer.device)]
                buffers.append(best[0])
                for _ in range(6):
                    best.append(_backend.DeviceBuffer(4 * n_queries * slots, buffer.device))
                    buffers.append(best[-1])
                _backend.dtw_topk(*[b.ptr for b in buffers[:5]], n_pairs, k, normalized, order, bounds, slots,
                                  *[b.ptr for b in best], device=buffer.device)
                for b, out in zip(best, (counts, top_pair, top_rank, cost, length, start, end)):
                    b.download(out)
            if return_paths:
                live = np.flatnonzero(np.tile(np.arange(slots), groups) < np.repeat(counts, slots))
                want = (live // slots, live % slots) if top_k is None else (top_pair[live], top_rank[live])
                if live.size:
                    paths = _hit_paths(buffer, dim, first, count, index_pairs, metric, normalized, k, max_score, want,
                                       (length[live], start[live], end[live]))
        finally:
            for b in buffers:
                b.free()
            if owned is not None:
                owned.release()
    # the rows: the first counts[g] slots of every group
    slot = np.tile(np.arange(slots, dtype=np.int32), groups)
    keep = np.flatnonzero(slot < np.repeat(counts, slots))
    group = (keep // slots).astype(np.int32)
    if top_k is None:
        pair, rank = group, slot[keep]
    else:
        pair, rank = top_pair[keep], top_rank[keep]
    cost, length, start, end = cost[keep], length[keep], start[keep], end[keep]
    score = cost / length.astype(np.float32) if normalized and keep.size else cost.copy()
    target = pairs[pair, 1] if keep.size else np.zeros(0, dtype=np.int32)
    onset, offset = _times(features, where, target, start, end)
    store = None
    if return_paths:
        store = _PathStore(*paths, _entry_centres(features, queries + targets, first, count),
                           pairs[pair, 0] if keep.size else target, n_queries + target)
    return DtwDetections(pair, pairs[pair, 0] if keep.size else target, target, rank, score, cost, length, start,
                         end, onset, offset, counts, curves, top_k, store)
