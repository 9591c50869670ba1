"""ABX discriminability scores of feature items, on the GPU

An extension with no counterpart in the reference.  Its worked examples (reference examples/features_abx) evaluate
features by ABX discrimination with three calls of an external toolkit on the CPU
(examples/features_abx/scripts/abx_score.sh:21-23: distances, scores, analysis) and average the scores
(examples/features_abx/scripts/collapse_abx.py:35-42).  :func:`abx_scores` builds the task from an item table,
computes the distances it needs with the DTW kernel of :mod:`shennong_amd.dtw` - they stay on the device - and
counts the triplets of every cell with a HIP kernel (snf_abx_cells):

    feats = processor.process_all_device(utterances)
    items = AbxItems.load('corpus.item')          # '#file onset offset #phone context talker'
    within = abx_scores(feats, items, on='phone', by=['talker', 'context'])
    across = abx_scores(feats, items, on='phone', across='talker', by=['context'])
    within.error_rate([['context', 'phone_1', 'phone_2'], ['phone_1', 'phone_2']])

Definitions (this project's own, tests/abx_np.py states them with plain loops; agreement with the external toolkit
is not pinned).  An item is the rows of an utterance whose centre time lies in
[onset, offset], with named labels.  A by-block is the set of items equal on every `by` column.  A triplet
(A, B, X) is three distinct items of one by-block with on(A) == on(X) != on(B) and, with `across`,
ac(A) == ac(B) != ac(X).  Its cell has the key (by values, on(A), on(B)[, ac(A), ac(X)]).  With d(Y, X) the DTW
distance of Y (first argument) and X (second) - both orders are computed, nothing is assumed symmetric -, a cell
counts less = #{d(A, X) < d(B, X)}, equal = #{d(A, X) == d(B, X)} over its n triplets, and
score = (less + 0.5 equal) / n in float64.  A triplet with a non-finite distance is an error.

Layout.  The items of a block are sorted by (across, on): every A-, B- and X-list of a cell is a contiguous range
of them.  The distances of a block of m items are the dense m x m table of all ordered pairs, X-major: element
x m + y is d(item y, item x).  A cell record addresses two sub-matrices of that table through offsets and the row
stride m (snf_abx_cells).  Blocks without a cell get no table.  The pairs that no triplet reads are the diagonal,
the rows of items that are the X of no triplet, the columns of items that are neither an A nor a B for that X and,
in an across task, the pairs whose two items share the `across` value: about half of the pairs computed on a
sparse corpus.
"""

import numpy as np

from shennong_amd import _backend
from shennong_amd import dtw as _dtw
from shennong_amd.device import DeviceFeaturesCollection

__all__ = ['AbxItems', 'AbxTable', 'abx_scores', 'build_task']


class AbxItems:
    """An item table: ``names`` (utterances), ``onsets`` and ``offsets`` in seconds (float64), ``labels`` a dict
    column name -> array of one label per item"""
    def __init__(self, names, onsets, offsets, labels):
        self.names = [str(name) for name in names]
        self.onsets = np.array(onsets, dtype=np.float64).reshape(-1)
        self.offsets = np.array(offsets, dtype=np.float64).reshape(-1)
        n = len(self.names)
        if self.onsets.shape[0] != n or self.offsets.shape[0] != n:
            raise ValueError('names, onsets and offsets have different lengths')
        late = np.flatnonzero(~(self.offsets >= self.onsets))
        if late.size:
            k = int(late[0])
            raise ValueError('item {} ("{}", {}, {}): offset < onset'.format(
                k, self.names[k], self.onsets[k], self.offsets[k]))
        self.labels = {}
        for column, values in dict(labels).items():
            values = np.asarray(values)
            if values.dtype.kind == 'O':
                values = values.astype(str)
            if values.ndim != 1 or values.shape[0] != n:
                raise ValueError('column "{}" does not hold one label per item'.format(column))
            self.labels[str(column)] = values

    def __len__(self):
        return len(self.names)

    @classmethod
    def load(cls, path):
        """Reads an ``.item`` file: the header ``#file onset offset #<label> <label> ...``, then one
        whitespace-separated row per item.  Labels are strings."""
        with open(path) as stream:
            lines = [line for line in (raw.strip() for raw in stream) if line]
        if not lines:
            raise ValueError('{}: missing header'.format(path))
        head = lines[0].split()
        if (len(head) < 4 or head[:3] != ['#file', 'onset', 'offset'] or not head[3].startswith('#')
                or len(head[3]) < 2):
            raise ValueError('{}: malformed header "{}", expected "#file onset offset #<label> ..."'.format(
                path, lines[0]))
        columns = [head[3][1:]] + head[4:]
        for column in columns:
            if columns.count(column) > 1:
                raise ValueError('{}: column "{}" is named twice'.format(path, column))
        names, times, rows = [], [], []
        for number, line in enumerate(lines[1:], start=2):
            fields = line.split()
            if len(fields) != 3 + len(columns):
                raise ValueError('{}: line {} has {} fields, the header names {}'.format(
                    path, number, len(fields), 3 + len(columns)))
            try:
                times.append((float(fields[1]), float(fields[2])))
            except ValueError:
                raise ValueError('{}: line {}: non-numeric time in "{} {}"'.format(
                    path, number, fields[1], fields[2])) from None
            names.append(fields[0])
            rows.append(fields[3:])
        times = np.array(times, dtype=np.float64).reshape(-1, 2)
        late = np.flatnonzero(~(times[:, 1] >= times[:, 0]))
        if late.size:
            raise ValueError('{}: line {}: offset < onset'.format(path, int(late[0]) + 2))
        labels = {column: np.array([row[k] for row in rows], dtype=str) for k, column in enumerate(columns)}
        return cls(names, times[:, 0], times[:, 1], labels)

    def save(self, path):
        """Writes the ``.item`` format that :meth:`load` reads (times with ``repr``: they round-trip)"""
        columns = list(self.labels)
        if not columns:
            raise ValueError('an .item file needs at least one label column')
        if any(len(column.split()) != 1 for column in columns):
            raise ValueError('a column name is empty or holds white space')
        lines = ['#file onset offset #{}'.format(' '.join(columns))]
        for k, name in enumerate(self.names):
            fields = [name, repr(float(self.onsets[k])), repr(float(self.offsets[k]))]
            fields += [str(self.labels[column][k]) for column in columns]
            if any(len(field.split()) != 1 for field in fields):
                raise ValueError('item {}: a field is empty or holds white space'.format(k))
            lines.append(' '.join(fields))
        with open(path, 'w') as stream:   # (every field has been checked: a refusal leaves no file behind)
            stream.write('\n'.join(lines) + '\n')


def _expand(counts):
    """For counts [n]: (rep, k) with rep = each i repeated counts[i] times and k = 0 .. counts[i] - 1 within"""
    counts = np.asarray(counts, dtype=np.int64)
    starts = np.cumsum(counts) - counts
    rep = np.repeat(np.arange(counts.shape[0], dtype=np.int64), counts)
    return rep, np.arange(rep.shape[0], dtype=np.int64) - starts[rep]


def _runs(change):
    """For a boolean array that marks the first element of every run: (run id, first index, size) per element"""
    run = np.cumsum(change) - 1
    first = np.flatnonzero(change)
    size = np.diff(np.append(first, change.shape[0]))
    return run, first[run], size[run]


class AbxTask:
    """The cells of a task over an item table, as ranges of the items sorted by (by, across, on): what
    :func:`build_task` returns.  Per cell (arrays, in the order of the table's rows): ``cell_block``, the label
    codes ``on_1``, ``on_2``, ``ac_1``, ``ac_2``, the ranges ``start_a``, ``start_b``, ``start_x`` (positions within
    the block), ``n_a``, ``n_b``, ``n_x``, and ``n`` (triplets).  Per block: ``block_start`` (into ``order``),
    ``block_size``, ``block_codes`` [blocks, len(by)]."""

    def runs(self, max_pairs):
        """Lists of consecutive blocks (those that have a cell) whose dense tables hold at most `max_pairs`
        pairs together; ValueError for a block that needs more on its own"""
        used = np.unique(self.cell_block)
        need = self.block_size[used] ** 2
        for b in used[need > max_pairs].tolist()[:1]:
            raise ValueError('the by-block {} has {} items and needs {} pairs, max_pairs is {}: tiling a block is '
                             'not supported'.format(self.block_name(b), int(self.block_size[b]),
                                                    int(self.block_size[b]) ** 2, int(max_pairs)))
        runs, current, total = [], [], 0
        for b, pairs in zip(used.tolist(), need.tolist()):
            if current and total + pairs > max_pairs:
                runs.append(np.array(current, dtype=np.int64))
                current, total = [], 0
            current.append(b)
            total += pairs
        if current:
            runs.append(np.array(current, dtype=np.int64))
        return runs

    def block_name(self, b):
        if not self.by:
            return '(all items)'
        return '({})'.format(', '.join('{}={}'.format(column, self.values[column][code])
                                       for column, code in zip(self.by, self.block_codes[b].tolist())))

    def tables(self, blocks):
        """(pairs int32 [P, 2], records int64 [n, 8], cells int64 [n]) of a run of blocks: pair p = (Y, X) as item
        indices, X-major within each block's dense table; the records of snf_abx_cells address it; `cells`
        are the indices of the records' cells in this task"""
        size, start = self.block_size[blocks], self.block_start[blocks]
        need = size ** 2
        base = np.cumsum(need) - need
        pairs = np.empty((int(need.sum()), 2), dtype=np.int32)
        order = self.order.astype(np.int32)
        for first, m, at in zip(start.tolist(), size.tolist(), base.tolist()):   # (one pass per block)
            mine = order[first:first + m]
            table = pairs[at:at + m * m].reshape(m, m, 2)
            table[:, :, 0] = mine[None, :]
            table[:, :, 1] = mine[:, None]
        lo = np.searchsorted(self.cell_block, blocks, side='left')
        hi = np.searchsorted(self.cell_block, blocks, side='right')
        which, within = _expand(hi - lo)
        cells = lo[which] + within
        m, row0 = size[which], base[which] + self.start_x[cells] * size[which]
        records = np.zeros((cells.shape[0], 8), dtype=np.int64)
        records[:, 0] = row0 + self.start_a[cells]
        records[:, 1] = row0 + self.start_b[cells]
        records[:, 2] = m
        records[:, 3] = self.n_a[cells]
        records[:, 4] = self.n_b[cells]
        records[:, 5] = self.n_x[cells]
        records[:, 6] = 0 if self.across else 1
        return pairs, records, cells


def build_task(labels, on, across=None, by=()):
    """The :class:`AbxTask` of the label columns `labels` (a dict name -> one label per item); vectorised numpy,
    no loop per pair, per triplet or per cell"""
    by = [by] if isinstance(by, str) else list(by)
    for column in [on] + ([across] if across is not None else []) + by:
        if column not in labels:
            raise ValueError('unknown column "{}", the items have "{}"'.format(column, ', '.join(labels)))
    if on in by or on == across:
        raise ValueError('the on column "{}" is also named in by or across'.format(on))
    if across is not None and across in by:
        raise ValueError('the across column "{}" is also named in by'.format(across))
    if len(set(by)) != len(by):
        raise ValueError('a by column is named twice')
    task = AbxTask()
    task.on, task.across, task.by = on, across, by
    task.values, codes = {}, {}
    for column in [on] + ([across] if across is not None else []) + by:
        task.values[column], codes[column] = np.unique(np.asarray(labels[column]), return_inverse=True)
        codes[column] = codes[column].reshape(-1).astype(np.int64)
    n_items = codes[on].shape[0]
    ac = codes[across] if across is not None else np.zeros(n_items, dtype=np.int64)
    # sorted by (by ..., across, on), equal ones in the order of the table (lexsort: the last key is the first)
    order = np.lexsort([codes[on], ac] + [codes[column] for column in reversed(by)]).astype(np.int64)
    task.order = order
    empty = np.zeros(0, dtype=np.int64)
    if n_items == 0:
        task.block_start = task.block_size = empty
        task.block_codes = np.zeros((0, len(by)), dtype=np.int64)
        for field in ('cell_block', 'on_1', 'on_2', 'ac_1', 'ac_2', 'start_a', 'start_b', 'start_x', 'n_a', 'n_b',
                      'n_x', 'n'):
            setattr(task, field, empty)
        return task
    by_sorted = np.stack([codes[column][order] for column in by], axis=1) if by else np.zeros((n_items, 0), np.int64)
    new_block = np.ones(n_items, dtype=bool)
    new_block[1:] = (by_sorted[1:] != by_sorted[:-1]).any(axis=1)
    block_of, block_first, _ = _runs(new_block)
    task.block_start = np.flatnonzero(new_block).astype(np.int64)
    task.block_size = np.diff(np.append(task.block_start, n_items)).astype(np.int64)
    task.block_codes = by_sorted[task.block_start]
    # groups: the runs of equal (block, across, on)
    on_sorted, ac_sorted = codes[on][order], ac[order]
    new_group = new_block.copy()
    new_group[1:] |= (on_sorted[1:] != on_sorted[:-1]) | (ac_sorted[1:] != ac_sorted[:-1])
    at = np.flatnonzero(new_group)
    g_block, g_on, g_ac = block_of[at], on_sorted[at], ac_sorted[at]
    g_start = at - block_first[at]
    g_n = np.diff(np.append(at, n_items))
    n_groups = at.shape[0]
    if across is None:
        # every ordered pair (P, Q) of different groups of a block, P with two items or more: A = X = P, B = Q
        change = np.ones(n_groups, dtype=bool)
        change[1:] = g_block[1:] != g_block[:-1]
        _, first, size = _runs(change)
        g_p, k = _expand(size)
        g_q = first[g_p] + k
        keep = (g_p != g_q) & (g_n[g_p] >= 2)
        g_a, g_b, g_x = g_p[keep], g_q[keep], g_p[keep]
        n = g_n[g_a] * (g_n[g_a] - 1) * g_n[g_b]
    else:
        # A and X: ordered pairs of different groups with the same (block, on) - contiguous once the groups are
        # sorted by (block, on, across); B: the other groups with A's (block, across), contiguous as they stand
        perm = np.lexsort([g_ac, g_on, g_block])
        change = np.ones(n_groups, dtype=bool)
        change[1:] = (g_block[perm][1:] != g_block[perm][:-1]) | (g_on[perm][1:] != g_on[perm][:-1])
        _, first, size = _runs(change)
        i, k = _expand(size)
        j = first[i] + k
        keep = i != j
        g_a, g_x = perm[i[keep]], perm[j[keep]]
        change = np.ones(n_groups, dtype=bool)
        change[1:] = (g_block[1:] != g_block[:-1]) | (g_ac[1:] != g_ac[:-1])
        _, first, size = _runs(change)
        rep, k = _expand(size[g_a])
        g_a, g_x = g_a[rep], g_x[rep]
        g_b = first[g_a] + k
        keep = g_b != g_a
        g_a, g_b, g_x = g_a[keep], g_b[keep], g_x[keep]
        n = g_n[g_a] * g_n[g_b] * g_n[g_x]
    # the rows of the table: sorted by (by ..., on_1, on_2, across_1, across_2) - the blocks are in `by` order
    # (one int64 key, not a lexsort of five: at 12 million cells the sort is the largest item of the construction)
    n_on, n_ac = int(task.values[on].shape[0]), int(ac.max()) + 1
    if float(g_block.max() + 1) * n_on * n_on * n_ac * n_ac >= 2.0 ** 62:
        raise ValueError('too many by-blocks and labels for one 64-bit row key')
    key = (((g_block[g_a] * n_on + g_on[g_a]) * n_on + g_on[g_b]) * n_ac + g_ac[g_a]) * n_ac + g_ac[g_x]
    rows = np.argsort(key, kind='stable')
    del key
    g_a, g_b, g_x, task.n = g_a[rows], g_b[rows], g_x[rows], n[rows].astype(np.int64)
    task.cell_block = g_block[g_a]
    task.on_1, task.on_2, task.ac_1, task.ac_2 = g_on[g_a], g_on[g_b], g_ac[g_a], g_ac[g_x]
    task.start_a, task.start_b, task.start_x = g_start[g_a], g_start[g_b], g_start[g_x]
    task.n_a, task.n_b, task.n_x = g_n[g_a], g_n[g_b], g_n[g_x]
    return task


class AbxTable:
    """The scores of a task, one row per cell, as numpy columns: ``<on>_1``, ``<on>_2`` (the labels of A and of B),
    with across ``<across>_1`` (of A and B) and ``<across>_2`` (of X), one column per `by` name, ``score``
    (float64), ``n``, ``less``, ``equal`` (int64).  The rows are sorted by (the `by` columns in the order given,
    ``<on>_1``, ``<on>_2``, ``<across>_1``, ``<across>_2``), every column in the order ``numpy.unique`` gives its
    values."""
    def __init__(self, columns):
        self.columns = dict(columns)
        sizes = {np.asarray(values).shape[0] for values in self.columns.values()}
        if len(sizes) > 1:
            raise ValueError('the columns have different lengths')

    def __len__(self):
        return int(self.columns['score'].shape[0])

    def __getitem__(self, column):
        return self.columns[column]

    def collapse(self, levels=()):
        """Successive unweighted means of ``score``, each grouped by the columns of one entry of `levels`, then
        the mean of what is left (reference examples/features_abx/scripts/collapse_abx.py:35-42).  An empty table
        gives nan."""
        columns, score = self.columns, np.asarray(self.columns['score'], dtype=np.float64)
        for level in levels:
            level = [level] if isinstance(level, str) else list(level)
            for column in level:
                if column not in columns or column in ('score', 'n', 'less', 'equal'):
                    raise ValueError('cannot group by column "{}"'.format(column))
            if not level or not score.shape[0]:
                continue
            codes = [np.unique(np.asarray(columns[column]), return_inverse=True)[1].reshape(-1) for column in level]
            order = np.lexsort(codes[::-1])
            keys = np.stack([code[order] for code in codes], axis=1)
            first = np.ones(order.shape[0], dtype=bool)
            first[1:] = (keys[1:] != keys[:-1]).any(axis=1)
            at = np.flatnonzero(first)
            count = np.diff(np.append(at, order.shape[0]))
            score = np.add.reduceat(score[order], at) / count
            columns = {column: np.asarray(columns[column])[order][at] for column in level}
        return float(score.mean()) if score.shape[0] else float('nan')

    def error_rate(self, levels=()):
        """``(1 - collapse(levels)) * 100``"""
        return (1.0 - self.collapse(levels)) * 100.0

    def save_csv(self, path):
        """Tab-separated text, one header line (``score`` with ``repr``: it round-trips)"""
        names = list(self.columns)
        with open(path, 'w') as stream:
            stream.write('\t'.join(names) + '\n')
            for k in range(len(self)):
                fields = []
                for name in names:
                    value = self.columns[name][k]
                    fields.append(repr(float(value)) if name == 'score' else str(value))
                stream.write('\t'.join(fields) + '\n')


def _resolve(features, items):
    """(first row, row count) of every item in the one block of `features`, its dim and the device block or None:
    what ``dtw_distances(items=...)`` selects and refuses, with one searchsorted pair per utterance"""
    first_of, dim, block = _dtw._layout(features)
    names = np.array(items.names, dtype=str) if len(items) else np.zeros(0, dtype=str)
    first = np.zeros(len(items), dtype=np.int64)
    count = np.zeros(len(items), dtype=np.int64)
    distinct, inverse = np.unique(names, return_inverse=True)
    order = np.argsort(inverse, kind='stable')
    bounds = np.searchsorted(inverse[order], np.arange(distinct.shape[0] + 1))
    for u, name in enumerate(distinct.tolist()):
        mine = order[bounds[u]:bounds[u + 1]]
        if name not in first_of:
            raise ValueError('item {}: utterance "{}" is not in the collection'.format(int(mine.min()), name))
        centres = _dtw._centres(features[name].times)
        lo = np.searchsorted(centres, items.onsets[mine], side='left')
        hi = np.searchsorted(centres, items.offsets[mine], side='right')
        first[mine] = first_of[name] + lo
        count[mine] = np.maximum(hi - lo, 0)

    def what(k):
        return 'item {} ("{}", {}, {})'.format(k, items.names[k], items.onsets[k], items.offsets[k])
    for k in np.flatnonzero(count < 1).tolist()[:1]:
        raise ValueError('{} has no frames'.format(what(k)))
    for k in np.flatnonzero(count > _dtw.MAX_FRAMES).tolist()[:1]:
        raise ValueError('{} has {} frames, the limit is {}'.format(what(k), int(count[k]), _dtw.MAX_FRAMES))
    return first, count.astype(np.int32), dim, block


def abx_scores(features, items, on, across=None, by=(), metric='cosine', normalized=True, max_pairs=1 << 26):
    """The :class:`AbxTable` of the task (`on`, `across`, `by`) over `items` (an :class:`AbxItems`)

    `features`: a :class:`DeviceFeaturesCollection` (the rows are used where they lie), or a host
    :class:`FeaturesCollection`, uploaded once.  `metric` ('cosine', 'sqeuclidean', or 'symkl' for posteriorgrams),
    `normalized`: as in ``dtw_distances``; the normalised value compared is the float32 quotient that
    ``dtw_distances(normalized=True)`` returns, bit for bit.
    The work is done in runs of whole by-blocks whose dense distance tables hold at most `max_pairs` pairs
    together; the distances never come to the host and the distances, path lengths and counts of a run are freed
    after it (the pair and cell tables of the last call stay in the slots of ``snf_dtw_pairs`` and
    ``snf_abx_cells``, which the next call reuses: 16 bytes per pair and 40 per cell).

    ValueError, before any device work: an unknown column or metric, `on` also named in `by` or `across`, a
    by-block that needs more than `max_pairs` pairs on its own, and what ``dtw_distances`` refuses (a name that is
    not in the collection, an item without frames or of more than ``MAX_FRAMES`` frames, items of different ndims,
    a collection in several device blocks).  Afterwards: a cell with a triplet whose distance is not finite."""
    if metric not in _backend.DTW_METRICS:
        raise ValueError('invalid metric "{}", choose in "{}"'.format(metric, ', '.join(_backend.DTW_METRICS)))
    if not isinstance(items, AbxItems):
        raise ValueError('items must be an AbxItems')
    task = build_task(items.labels, on, across, by)
    first, count, dim, block = _resolve(features, items)
    runs = task.runs(int(max_pairs))
    counts = np.zeros((task.n.shape[0], 3), dtype=np.uint64)
    if runs:
        owned = None
        if block is None:
            owned = DeviceFeaturesCollection.from_host(features)
            block = owned._blocks[0]
        try:
            buffer = block.alive()
            for blocks in runs:
                pairs, records, cells = task.tables(blocks)
                n_pairs = pairs.shape[0]
                got = np.zeros((cells.shape[0], 3), dtype=np.uint64)
                held = []
                try:
                    for nbytes in (4 * n_pairs, 4 * n_pairs, 24 * cells.shape[0]):
                        held.append(_backend.DeviceBuffer(nbytes, buffer.device))
                    d_cost, d_len, d_counts = held
                    _backend.dtw_pairs(buffer.ptr, dim, first, count, pairs, metric, d_cost.ptr, d_len.ptr,
                                       device=buffer.device)
                    del pairs
                    _backend.abx_cells(d_cost.ptr, d_len.ptr if normalized else None, n_pairs, records,
                                       d_counts.ptr, device=buffer.device)
                    d_counts.download(got)
                finally:
                    for one in held:
                        one.free()
                counts[cells] = got
        finally:
            if owned is not None:
                owned.release()
    return _table(task, counts)


def _table(task, counts):
    """The table of `task` from the counts [cells, 3] (less, equal, bad) of its cells"""
    for c in np.flatnonzero(counts[:, 2]).tolist()[:1]:
        key = ['{}={}'.format(column, task.values[column][code])
               for column, code in zip(task.by, task.block_codes[task.cell_block[c]].tolist())]
        key += ['{}_1={}'.format(task.on, task.values[task.on][task.on_1[c]]),
                '{}_2={}'.format(task.on, task.values[task.on][task.on_2[c]])]
        if task.across is not None:
            key += ['{}_1={}'.format(task.across, task.values[task.across][task.ac_1[c]]),
                    '{}_2={}'.format(task.across, task.values[task.across][task.ac_2[c]])]
        raise ValueError('the cell ({}) has {} triplets with a distance that is not finite'.format(
            ', '.join(key), int(counts[c, 2])))
    less, equal = counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64)
    columns = {task.on + '_1': task.values[task.on][task.on_1], task.on + '_2': task.values[task.on][task.on_2]}
    if task.across is not None:
        columns[task.across + '_1'] = task.values[task.across][task.ac_1]
        columns[task.across + '_2'] = task.values[task.across][task.ac_2]
    for k, column in enumerate(task.by):
        columns[column] = task.values[column][task.block_codes[task.cell_block, k]]
    columns['score'] = (less.astype(np.float64) + 0.5 * equal.astype(np.float64)) / task.n.astype(np.float64)
    columns['n'], columns['less'], columns['equal'] = task.n, less, equal
    return AbxTable(columns)
