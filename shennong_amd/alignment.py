"""Time alignments of speech signals: ``<item> <onset> <offset> <token>``

Counterpart of reference shennong/alignment.py: :class:`Alignment` (:93-354) is the alignment of one
item - `ntokens` (onset, offset) pairs in seconds and as many tokens -, :class:`AlignmentCollection`
(:357-496) a dict item -> :class:`Alignment` that reads and writes alignment files, plain or gzip.
Alignments feed :class:`~shennong_amd.processor.onehot.OneHotProcessor` and
:class:`~shennong_amd.processor.onehot.FramedOneHotProcessor`.

Host only: an alignment is a few dozen numbers.  One difference from the reference is documented at
:meth:`Alignment.at_sample_rate`.
"""

import gzip
import os

import numpy as np


class Alignment:
    """Tokens with their onsets and offsets: `times` [ntokens, 2] in seconds, `tokens` [ntokens]

    With `validate` (the default) a ValueError is raised unless :meth:`validate` passes."""

    def __init__(self, times, tokens, validate=True):
        self._times = times
        self._tokens = tokens
        if validate is True:
            self.validate()

    @property
    def times(self):
        """(onset, offset) of every token, in seconds"""
        return self._times

    @property
    def onsets(self):
        """Onset of every token, in seconds"""
        return self._times[:, 0]

    @property
    def offsets(self):
        """Offset of every token, in seconds"""
        return self._times[:, 1]

    @property
    def tokens(self):
        """The aligned tokens"""
        return self._tokens

    @staticmethod
    def from_list(data, validate=True):
        """An alignment from (onset, offset, token) triplets"""
        for i, entry in enumerate(data):
            if len(entry) != 3:
                raise ValueError(f'line {i}: entry must have 3 fields but has {len(entry)}')
        times = np.array([entry[:2] for entry in data], dtype=float)
        tokens = np.array([entry[2] for entry in data])
        return Alignment(times, tokens, validate=validate)

    def validate(self):
        """Raises a ValueError unless times and tokens have one length, every token has a strictly
        positive duration, onsets increase and every offset is the next token's onset"""
        ntokens = self.tokens.shape[0]
        if self._times.shape[0] != ntokens:
            raise ValueError('timestamps and tokens must have the same length')
        if ntokens == 0:
            return
        onsets, offsets = self.onsets, self.offsets
        late = np.flatnonzero(onsets >= offsets)
        if late.size:
            raise ValueError(f'token {late[0]}: onset must be lesser than offset')
        # (reported in token order, the two conditions of one token in this order)
        unsorted = onsets[:-1] > onsets[1:]
        gap = offsets[:-1] != onsets[1:]
        bad = np.flatnonzero(unsorted | gap)
        if bad.size:
            if unsorted[bad[0]]:
                raise ValueError('timestamps must be sorted in increasing order')
            raise ValueError('mismatch in tstop/tstart timestamps')

    def is_valid(self):
        """True when :meth:`validate` passes"""
        try:
            self.validate()
        except ValueError:
            return False
        return True

    def __eq__(self, other):
        return np.array_equal(self._times, other._times) and np.array_equal(self.tokens, other.tokens)

    def __getitem__(self, time):
        """The part of the alignment inside a slice of time in seconds, ``alignment[0.5:2.0]``: the
        slice is clipped to the alignment, the first and last tokens are cut at its ends; an empty
        alignment when nothing is left, the alignment itself when the slice covers it"""
        if not isinstance(time, slice):
            raise ValueError(f'time must be a slice but is {type(time)}')
        if time.step is not None:
            raise ValueError('time.step is defined but is useless')
        tmin, tmax = self.onsets[0], self.offsets[-1]
        tstart = tmin if time.start is None or time.start < tmin else time.start
        tstop = tmax if time.stop is None or time.stop > tmax else time.stop
        if tstart >= tstop or tstart >= tmax or tstop <= tmin:
            return Alignment(np.array([]), np.array([]), validate=False)
        if tstart == tmin and tstop == tmax:
            return self
        # the token under way at tstart (the last one that has begun) ... at tstop (the first that ends there
        # or later)
        first = np.searchsorted(self.onsets, tstart, side='right') - 1
        last = np.searchsorted(self.offsets, tstop, side='left')
        if first == last:
            return Alignment(np.array([[tstart, tstop]]), np.array(self.tokens[first:first + 1]), validate=False)
        times = np.copy(self._times[first:last + 1])
        times[0, 0], times[-1, 1] = tstart, tstop
        return Alignment(times, self.tokens[first:last + 1], validate=False)

    def __repr__(self):
        return '\n'.join(f'{onset} {offset} {token}' for onset, offset, token in self.to_list())

    def to_list(self):
        """(onset, offset, token) triplets: the reverse of :meth:`from_list`"""
        return [(self.onsets[i], self.offsets[i], self.tokens[i]) for i in range(self.tokens.shape[0])]

    def sample_times(self, sample_rate):
        """Time of every sample of :meth:`at_sample_rate`, float64: ``i / sample_rate + onsets[0]``, one IEEE
        division then one addition (the device evaluates the same expression, csrc/kernels_onehot.hip)"""
        nsamples = int(self.duration() * sample_rate)
        return np.arange(nsamples) / sample_rate + (self.onsets[0] if nsamples else 0.0)

    def at_sample_rate(self, sample_rate):
        """The token of every sample at `sample_rate`, ``int(duration * sample_rate)`` of them: sample `i`
        takes the first token whose offset is greater than ``i / sample_rate + onsets[0]``.

        The reference (alignment.py:321-337) walks over the samples; this is one search.  When rounding
        puts the last samples at or past the final offset they take the last token, where the reference's
        walk runs off the end of the alignment (IndexError)."""
        times = self.sample_times(sample_rate)
        if times.shape[0] == 0:
            return np.zeros((0,), dtype=self.tokens.dtype)
        index = np.searchsorted(self.offsets, times, side='right')
        return self.tokens[np.minimum(index, self.tokens.shape[0] - 1)]

    def duration(self):
        """Duration of the alignment in seconds"""
        if len(self.tokens) == 0:
            return 0
        return self.offsets[-1] - self.onsets[0]

    def get_tokens_inventory(self):
        """The set of the tokens of the alignment"""
        return set(self.tokens)


class AlignmentCollection(dict):
    """A dict item -> :class:`Alignment` built from (item, onset, offset, token) quadruplets

    Raises a ValueError for an entry that is not a quadruplet and for an item whose alignment is not
    valid."""

    def __init__(self, data):
        super().__init__()
        entries = {}
        for i, entry in enumerate(data):
            if len(entry) != 4:
                raise ValueError(f'alignment must have 4 columns but line {i + 1} has {len(entry)}')
            entries.setdefault(entry[0], []).append(entry[1:])
        for item, triplets in entries.items():
            try:
                self[item] = Alignment.from_list(triplets, validate=True)
            except ValueError as err:
                raise ValueError(f'item {item}: {err}') from None

    @staticmethod
    def load(filename, compress=False):
        """The collection read from a text file of ``<item> <onset> <offset> <token>`` lines (utf8,
        gzip with `compress`)"""
        if not os.path.isfile(filename):
            raise ValueError(f'{filename}: file not found')
        opener = gzip.open if compress is True else open
        with opener(filename, 'rt', encoding='utf8') as stream:
            return AlignmentCollection([line.split() for line in stream])

    def save(self, filename, sort=False, compress=False):
        """Writes the collection to `filename`, which must not exist; items in lexicographical order
        with `sort`, gzip with `compress`"""
        if os.path.isfile(filename):
            raise ValueError(f'{filename} already exist')
        items = sorted(self.keys()) if sort is True else self.keys()
        opener = gzip.open if compress is True else open
        try:
            with opener(filename, 'wt', encoding='utf8') as stream:
                for item in items:
                    stream.write('\n'.join(self._list_str(item)) + '\n')
        except FileNotFoundError:
            raise ValueError(f'cannot write to {filename}') from None

    def _list_str(self, item):
        return [f'{item} {onset} {offset} {token}' for onset, offset, token in self[item].to_list()]

    def get_tokens_inventory(self):
        """The set of the tokens of all the alignments"""
        return set().union(*(a.get_tokens_inventory() for a in self.values()))
