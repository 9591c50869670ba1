"""One hot encoding of time-aligned tokens: Alignment --> {Framed}OneHotProcessor --> Features

Counterpart of reference shennong/processor/onehot.py: :class:`OneHotProcessor` (:99-140) turns the tokens
of an :class:`~shennong_amd.alignment.Alignment` into one-hot rows on the alignment's own timestamps,
:class:`FramedOneHotProcessor` (:143-267) labels the frames of the grid the MFCC or filterbank features of
the same signal live on.

The first is indexing and stays on the host.  The second is the reference's loop over frames, over the
samples of every frame that holds a token boundary, over the samples of the alignment before that
(alignment.py:321-337): here one call of ``snf_framed_onehot`` (csrc/kernels_onehot.hip) for a whole
collection - :meth:`FramedOneHotProcessor.process_all`, an extension of this package - with no CPU path.

One documented difference from the reference: when rounding puts the last samples of an alignment at or
past its final offset they take the last token; the reference ends in an IndexError there.
"""

import ctypes as C

import numpy as np

from shennong_amd import _abi, _backend, window
from shennong_amd.features import Features, FeaturesCollection
from shennong_amd.frames import Frames
from shennong_amd.processor.base import FeaturesProcessor
from shennong_amd.utils import get_njobs


class _OneHotBase(FeaturesProcessor):
    def __init__(self, tokens=None):
        super().__init__()
        self.tokens = tokens

    @property
    def name(self):
        return 'onehot'

    @property
    def tokens(self):
        """The tokens of the one-hot columns, sorted; None: those of the alignment being processed"""
        return self._tokens

    @tokens.setter
    def tokens(self, value):
        self._tokens = None if value is None else sorted(set(value))

    @property
    def ndims(self):
        if self.tokens:
            return len(self.tokens)
        raise ValueError('onehot tokens are not defined, cannot know their dimension')

    def _tokens_set(self, alignment):
        if self.tokens is None:
            return alignment.get_tokens_inventory()
        known = set(self.tokens)
        errors = [p for p in set(alignment.tokens) if p not in known]
        if errors != []:
            raise ValueError(
                'following tokens are in alignment but not defined in the '
                'onehot features processor: {}'.format(errors))
        return self.tokens

    def _token2index(self, alignment):
        return {p: i for i, p in enumerate(sorted(self._tokens_set(alignment)))}

    def _properties(self, token2index):
        """``get_properties()`` with the tokens of this call where the processor has none, plus `token2index`"""
        params = self.get_params()
        if not self.tokens:
            params['tokens'] = sorted(token2index)
        params['token2index'] = token2index
        return {'pipeline': [{'name': self.name, 'columns': [0, len(params['tokens']) - 1]}], self.name: params}


class OneHotProcessor(_OneHotBase):
    """One-hot rows of the tokens of an alignment, on the alignment's own timestamps

    `tokens`: the tokens of the columns, for rows that mean the same across alignments; by default the
    tokens of the alignment given to :meth:`process`."""

    def __init__(self, tokens=None):
        super().__init__(tokens=tokens)

    def process(self, alignment):
        token2index = self._token2index(alignment)
        data = np.zeros((alignment.tokens.shape[0], len(token2index)), dtype=bool)
        columns = [token2index[p] for p in alignment.tokens]
        data[np.arange(data.shape[0]), columns] = True
        return Features(data, alignment.times, properties=self._properties(token2index))


class FramedOneHotProcessor(_OneHotBase):
    """One-hot label of every frame of an aligned signal

    A frame takes the token all its samples carry; a frame with several takes the token with the largest
    window weight (the sum of the window coefficients of its samples), the first of them in the frame when
    two weigh the same.  `tokens` as for :class:`OneHotProcessor`; `sample_rate` in Hertz, `frame_shift` and
    `frame_length` in seconds: the grid of the features the labels go with; `window_type` one of
    :func:`shennong_amd.window.types`, `blackman_coeff` for the blackman window."""

    def __init__(self, tokens=None, sample_rate=16000,
                 frame_shift=0.01, frame_length=0.025,
                 window_type='povey', blackman_coeff=0.42):
        super().__init__(tokens=tokens)
        self.frame = Frames(sample_rate=sample_rate, frame_shift=frame_shift, frame_length=frame_length)
        self.window_type = window_type
        self.blackman_coeff = blackman_coeff

    @property
    def sample_rate(self):
        """Sample frequency of the frames, in Hertz"""
        return self.frame.sample_rate

    @sample_rate.setter
    def sample_rate(self, value):
        self.frame.sample_rate = value

    @property
    def frame_shift(self):
        """Frame shift in seconds"""
        return self.frame.frame_shift

    @frame_shift.setter
    def frame_shift(self, value):
        self.frame.frame_shift = value

    @property
    def frame_length(self):
        """Frame length in seconds"""
        return self.frame.frame_length

    @frame_length.setter
    def frame_length(self, value):
        self.frame.frame_length = value

    def process(self, alignment):
        """Features [nframes, ntokens] of bool, times ``Frames.boundaries(nframes) / sample_rate``"""
        return self._process_batch([alignment])[0]

    def process_all(self, alignments, njobs=None):
        """The framed one-hot features of every alignment of an :class:`AlignmentCollection` (or a dict name ->
        :class:`Alignment`) as a :class:`FeaturesCollection`: one batch on the device.  An extension of this
        package (the reference has no `process_all` over alignments).  `njobs` is checked and otherwise unused.

        With `tokens` None every alignment is encoded over its own inventory, as by :meth:`process`; for one
        label space pass ``tokens=alignments.get_tokens_inventory()``.  The matrices are views of one
        batch-sized array, like those of every other `process_all` here."""
        get_njobs(njobs, log=self.log)
        names = list(alignments.keys())
        return FeaturesCollection(zip(names, self._process_batch([alignments[n] for n in names])))

    def _process_batch(self, alignments, timing=None):
        """`timing`: a dict that receives ``kernel_ms`` (device time of the kernels, from events) and ``winners``
        (the int32 token id of every frame of the batch)"""
        rate = self.frame.sample_rate
        length, shift = self.frame.samples_per_frame, self.frame.samples_per_shift
        if self.window_type not in window.types():
            raise ValueError(f'type must be in {window.types()} but is {self.window_type}')
        n = len(alignments)
        maps, ids, offsets = [], [], []
        seg_off = np.zeros(n + 1, dtype=np.int64)
        row_off = np.zeros(n + 1, dtype=np.int64)
        onset0 = np.zeros(n, dtype=np.float64)
        nsamples = np.zeros(n, dtype=np.int64)
        nframes = np.zeros(n, dtype=np.int64)
        ntokens = np.zeros(n, dtype=np.int32)
        frames_of = {}
        for a, alignment in enumerate(alignments):
            token2index = self._token2index(alignment)
            maps.append(token2index)
            count = alignment.tokens.shape[0]
            seg_off[a + 1] = seg_off[a] + count
            ntokens[a] = len(token2index)
            if count:
                ids.extend(token2index[p] for p in alignment.tokens.tolist())
                offsets.append(np.asarray(alignment.offsets, dtype=np.float64))
                onset0[a] = alignment.onsets[0]
                nsamples[a] = int(alignment.duration() * rate)
            samples = int(nsamples[a])
            if samples not in frames_of:
                frames_of[samples] = self.frame.nframes(samples)
            nframes[a] = frames_of[samples]
            row_off[a + 1] = row_off[a] + (int(nframes[a]) * int(ntokens[a]) + 15) // 16 * 16
        if _backend.device_count() < 1:
            raise RuntimeError('no HIP device visible: FramedOneHotProcessor has no CPU path')
        ids = np.asarray(ids, dtype=np.int32)
        offsets = np.concatenate(offsets) if offsets else np.zeros(0, dtype=np.float64)
        total_frames, total_bytes = int(nframes.sum()), int(row_off[-1])
        device = _backend.get_device()
        d_winner = _backend.DeviceBuffer(max(16, 4 * total_frames), device)
        d_rows = _backend.DeviceBuffer(max(16, total_bytes), device)
        kernel_ms = C.c_float(0.0)
        p64, p32, pf64 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
        try:
            _backend.check(_backend.lib().snf_framed_onehot(
                device, float(rate), length, shift, _abi.WINDOW_TYPES[self.window_type], float(self.blackman_coeff), n,
                seg_off.ctypes.data_as(p64), onset0.ctypes.data_as(pf64), offsets.ctypes.data_as(pf64),
                ids.ctypes.data_as(p32), nsamples.ctypes.data_as(p64), nframes.ctypes.data_as(p64),
                ntokens.ctypes.data_as(p32), row_off.ctypes.data_as(p64), C.c_void_p(d_winner.ptr),
                C.c_void_p(d_rows.ptr), C.byref(kernel_ms), None))
            rows = _backend.result_array((total_bytes,), np.uint8)
            if total_bytes:
                d_rows.download(rows)
            if timing is not None:
                timing['kernel_ms'] = float(kernel_ms.value)
                timing['winners'] = d_winner.download(np.empty(total_frames, dtype=np.int32))
        finally:
            d_winner.free(synced=True)
            d_rows.free(synced=True)
        times_of, out = {}, []
        for a in range(n):
            frames, width = int(nframes[a]), int(ntokens[a])
            data = rows[row_off[a]:row_off[a] + frames * width].reshape(frames, width).view(np.bool_)
            if frames not in times_of:
                times_of[frames] = self.frame.boundaries(frames) / rate
            out.append(Features._of_batch(data, times_of[frames], self._properties(maps[a])))
        return out
