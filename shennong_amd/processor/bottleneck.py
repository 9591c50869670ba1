"""Extraction of bottleneck features from a speech signal

    :class:`~shennong_amd.audio.Audio` ---> BottleneckProcessor ---> :class:`~shennong_amd.features.Features`

The BUT/Phonexia bottleneck feature extractor (Silnova et al., Odyssey 2018; Fer et al., Computer Speech
and Language 2017): a voice activity detection, a 24-band HTK log-mel filterbank at 8 kHz, a Hamming-DCT
projection of a window of frames and two stacked feed-forward networks whose 80-wide bottleneck layer is
the feature.  Same parameters, properties and messages as the reference's processor/bottleneck.py (pure
numpy there); here every stage is a HIP kernel (``kernels_bottleneck.hip``): the dense layers run on the
FP32 matrix cores with bias and activation fused, and ``process_all`` is one batched launch per kernel
over all utterances.

Beyond the reference: the attribute :attr:`BottleneckProcessor.precision` (``'float32'`` by default) selects
a bfloat16 matrix-core path for the four layers that read sigmoid outputs (``W2``, ``W3``, ``W6``, ``W7``):
their activations and weights are rounded to bfloat16 (to nearest, ties to even) at the layer's input and the
products accumulated in float32; everything else is the float32 path unchanged.

Also beyond the reference: the attribute :attr:`BottleneckProcessor.resample` (``'scipy'`` by default).  With
``'kaldi'`` audio that is not at 8 kHz is uploaded at its own rate and resampled on the device by Kaldi's
ResampleWaveform (``kernels_resample.hip``; cutoff 0.99 x half the lower rate, 6 zero crossings), a whole batch
per rate in one launch, straight into the batch's 8 kHz block; the samples are converted to int16 *before*
the resampling (after it on the default path) and the resampled length is Kaldi's (22 713 samples at 16 kHz
give 11 357, the Fourier method 11 356).  With ``'scipy'`` nothing differs from before.

Weights: the three published networks *BabelMulti*, *FisherMono* and *FisherTri* are ``.npz`` files of 17
arrays that are not shipped with this package.  They are looked up under their published names in the
directory named by the environment variable ``SHENNONG_AMD_BOTTLENECK_DIR`` and then in
``shennong_amd/share/bottleneck/``.

Differences from the reference: input that is not 8 kHz int16 is resampled by this package's
:meth:`Audio.resample` (scipy's Fourier method; the reference uses sox, whose output differs); the dither
is a counter-based uniform noise keyed by the utterance's content, so a call is reproducible (the
reference draws from numpy's global generator).

>>> from shennong_amd import Audio
>>> from shennong_amd.processor.bottleneck import BottleneckProcessor
>>> audio = Audio.load('./tests/golden/test.wav')
>>> processor = BottleneckProcessor(weights='BabelMulti')     # doctest: +SKIP
>>> processor.process(audio).shape                            # doctest: +SKIP
(140, 80)
"""

import ctypes as C
import logging
import os
import threading

import numpy as np

from shennong_amd import _backend
from shennong_amd.audio import Audio
from shennong_amd.features import Features
from shennong_amd.logger import get_logger
from shennong_amd.processor.base import FeaturesProcessor

ENV_DIR = 'SHENNONG_AMD_BOTTLENECK_DIR'
_FILES = {
    'BabelMulti': 'Babel-ML17_FBANK_HL1500_SBN80_PhnStates3096',
    'FisherMono': 'FisherEnglish_FBANK_HL500_SBN80_PhnStates120',
    'FisherTri': 'FisherEnglish_FBANK_HL500_SBN80_triphones2423'}
_KEYS = ('bn_std', 'input_mean', 'b2', 'b5', 'input_std', 'W5', 'W7', 'W6', 'b6', 'b7', 'W3', 'W2', 'context',
         'b3', 'bn_mean', 'W1', 'b1')

_WIN, _SHIFT, _NFFT, _NMEL, _NBASES, _EDGE, _NDIMS, _STACK = 200, 80, 256, 24, 6, 15, 80, 5
_NIN = _NMEL * _NBASES
_MAX_CONTEXT = 64
_DITHER_SEED = 0x5EED0B0771E9EC
PRECISIONS = ('float32', 'bfloat16')
_PACKED = (2, 4, 8, 10)    # W2, W3, W6, W7 among the twelve parameters: the layers of the bfloat16 path

_LOCK = threading.Lock()
_LOADED = {}    # (name, file) -> validated host parameters
_DEVICE = {}    # (name, file, device) -> uploaded parameters
_WARNED = set()
_TABLES = {}    # device -> front-end tables; (device, context) -> projection basis


def _mel_filterbank():
    """[129, 24] float64: 24 triangular filters on the HTK mel scale between 64 and 3800 Hz for a 256-point
    transform at 8 kHz, with the edges at ``floor(f / 8000 * 256) + 1`` (reference bottleneck.py:135-179)"""
    def mel(f):
        return 1127.0 * np.log(1.0 + f / 700.0)

    nbins = _NFFT // 2 + 1
    bin_mel = mel(np.arange(nbins, dtype=np.float64) * 8000.0 / _NFFT)
    centre = np.linspace(mel(64.0), mel(3800.0), _NMEL + 2)
    index = np.floor((np.exp(centre / 1127.0) - 1.0) * 700.0 / 8000.0 * _NFFT).astype(int) + 1
    bank = np.zeros((nbins, _NMEL))
    for i in range(_NMEL):
        lo, mid, hi = index[i:i + 3]
        bank[lo:mid, i] = (centre[i] - bin_mel[lo:mid]) / (centre[i] - centre[i + 1])
        bank[mid:hi, i] = (centre[i + 2] - bin_mel[mid:hi]) / (centre[i + 2] - centre[i + 1])
    if 64.0 / 8000.0 * _NFFT + 0.5 > index[0]:
        bank[index[0], :] = 0.0
    return bank


def _front_tables():
    """The table blob of ``snf_bottleneck_fbank``: window[200] | twiddles[256 x 2] | filterbank[129 x 24]"""
    angle = -2.0 * np.pi * np.arange(_NFFT) / _NFFT
    twiddles = np.stack([np.cos(angle), np.sin(angle)], axis=1)
    return np.concatenate([np.hamming(_WIN), twiddles.reshape(-1), _mel_filterbank().reshape(-1)]).astype(np.float32)


def _context_basis(context):
    """[(2 context + 1), 6] float64: the first six rows of the orthonormal DCT-II over the window, row 0
    replaced by ``sqrt(2 / L)``, times a Hamming window (reference bottleneck.py:456-470)"""
    length = 2 * context + 1
    k = np.arange(_NBASES, dtype=np.float64)[None, :]
    t = np.arange(length, dtype=np.float64)[:, None]
    basis = np.sqrt(2.0 / length) * np.cos(np.pi * k * (2.0 * t + 1.0) / (2.0 * length))
    basis[:, 0] = np.sqrt(2.0 / length)
    return basis * np.hamming(length)[:, None]


def _validate(arrays, origin):
    """The 17 arrays of a weights file checked against each other; returns (context, float64 parameters)"""
    missing = sorted(set(_KEYS) - set(arrays))
    if missing:
        raise ValueError(f'{origin}: missing arrays {", ".join(missing)}')
    context = np.asarray(arrays['context'])
    if context.size != 1 or int(context.reshape(-1)[0]) != context.reshape(-1)[0]:
        raise ValueError(f'{origin}: array "context" must hold one integer, it has shape {context.shape}')
    context = int(context.reshape(-1)[0])
    if not 0 <= context <= _MAX_CONTEXT:
        raise ValueError(f'{origin}: array "context" must be in [0, {_MAX_CONTEXT}], it is {context}')
    p = {k: np.asarray(arrays[k], dtype=np.float64) for k in _KEYS if k != 'context'}

    def expect(name, shape):
        if p[name].shape != shape:
            raise ValueError(f'{origin}: array "{name}" has shape {p[name].shape}, expected {shape}')

    for name in ('W1', 'W2', 'W3', 'W5', 'W6', 'W7'):
        if p[name].ndim != 2:
            raise ValueError(f'{origin}: array "{name}" has shape {p[name].shape}, expected a matrix')
    expect('input_mean', (_NIN,))
    expect('input_std', (_NIN,))
    expect('W1', (_NIN, p['W1'].shape[1]))
    expect('b1', (p['W1'].shape[1],))
    expect('W2', (p['W1'].shape[1], p['W2'].shape[1]))
    expect('b2', (p['W2'].shape[1],))
    expect('W3', (p['W2'].shape[1], _NDIMS))
    expect('b3', (_NDIMS,))
    expect('bn_mean', (_STACK * _NDIMS,))
    expect('bn_std', (_STACK * _NDIMS,))
    expect('W5', (_STACK * _NDIMS, p['W5'].shape[1]))
    expect('b5', (p['W5'].shape[1],))
    expect('W6', (p['W5'].shape[1], p['W6'].shape[1]))
    expect('b6', (p['W6'].shape[1],))
    expect('W7', (p['W6'].shape[1], _NDIMS))
    expect('b7', (_NDIMS,))
    for name, value in p.items():
        if not np.all(np.isfinite(value)):
            raise ValueError(f'{origin}: array "{name}" holds non-finite values')
    return context, p


def _fold(p):
    """(X + mean) * std @ W + b = X @ (std[:, None] * W) + ((mean * std) @ W + b): the two affine
    normalisations folded into W1 / b1 and W5 / b5 in float64; the twelve float32 arrays the device takes"""
    w1 = p['input_std'][:, None] * p['W1']
    b1 = (p['input_mean'] * p['input_std']) @ p['W1'] + p['b1']
    w5 = p['bn_std'][:, None] * p['W5']
    b5 = (p['bn_mean'] * p['bn_std']) @ p['W5'] + p['b5']
    arrays = [w1, b1, p['W2'], p['b2'], p['W3'], p['b3'], w5, b5, p['W6'], p['b6'], p['W7'], p['b7']]
    return [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]


class _Network:
    """One set of weights: context, widths and the folded float32 parameters (host)"""
    def __init__(self, arrays, origin):
        self.context, p = _validate(arrays, origin)
        self.widths = (p['W1'].shape[1], p['W2'].shape[1], p['W5'].shape[1], p['W6'].shape[1])
        self.params = _fold(p)


class _DeviceNetwork:
    def __init__(self, net, device):
        self.net = net
        self.buffers = []
        for a in net.params:
            buf = _backend.DeviceBuffer(max(16, a.nbytes), device)
            buf.upload(a)
            self.buffers.append(buf)
        self.device = device
        self.pointers = (C.c_void_p * 12)(*[b.ptr for b in self.buffers])
        self.widths = (C.c_int32 * 4)(*net.widths)
        self._packed = None

    def packed_pointers(self):
        """The twelve pointers with W2, W3, W6 and W7 as packed bfloat16 images (built on first use and kept
        beside the float32 weights)"""
        with _LOCK:
            if self._packed is None:
                pointers = [b.ptr for b in self.buffers]
                images = []
                for i in _PACKED:
                    images.append(pack_weights(self.buffers[i], *self.net.params[i].shape, self.device))
                    pointers[i] = images[-1].ptr
                self._packed = (images, (C.c_void_p * 12)(*pointers))
            return self._packed[1]


def _check_precision(value):
    if value not in PRECISIONS:
        raise ValueError('invalid precision "{}", choose in "{}"'.format(value, ', '.join(PRECISIONS)))
    return value


def pack_weights(w, k, n, device):
    """The packed bfloat16 image (a DeviceBuffer) of the float32 matrix [k, n] in the DeviceBuffer `w`"""
    L = _backend.lib()
    image = _backend.DeviceBuffer(max(16, 2 * int(L.snf_packed_weights_bf16_size(k, n))), device)
    _backend.check(L.snf_pack_weights_bf16(device, _p(w), k, n, _p(image), None))
    return image


def _device_array(key, build, device):
    with _LOCK:
        buf = _TABLES.get(key)
        if buf is None:
            host = np.ascontiguousarray(build(), dtype=np.float32)
            buf = _backend.DeviceBuffer(max(16, host.nbytes), device)
            buf.upload(host)
            _TABLES[key] = buf
        return buf


def num_frames(nsamples):
    """Frames of 200 samples every 80 in `nsamples` samples"""
    return int((nsamples - _WIN) / _SHIFT + 1) if nsamples >= _WIN else 0


def _p(buf):
    return C.c_void_p(buf.ptr)


def _off(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


class BottleneckBatch:
    """The stages of one batch of 8 kHz int16 utterances on the device, each one batched launch through the C
    ABI: :meth:`vad`, :meth:`fbank`, :meth:`forward` (the tests and ``tools/time_bottleneck.py`` read the
    intermediate buffers); and all of them as one call that keeps no intermediate, :meth:`extract` (the
    pipeline's entry)"""

    def __init__(self, waves, device=None):
        device = _backend.get_device() if device is None else int(device)
        waves = [np.ascontiguousarray(w, dtype=np.int16).reshape(-1) for w in waves]
        soff = np.zeros(len(waves) + 1, dtype=np.int64)
        np.cumsum([w.shape[0] for w in waves], out=soff[1:])
        self._layout(_backend.upload_rows(waves, np.int16, device), soff, device)

    @classmethod
    def from_device(cls, block, soff, device=None):
        """The batch over 8 kHz int16 audio that is already on the device: utterance u is the samples
        ``soff[u]:soff[u + 1]`` of the DeviceBuffer `block`"""
        batch = cls.__new__(cls)
        batch._layout(block, np.ascontiguousarray(soff, dtype=np.int64), block.device if device is None else device)
        return batch

    def _layout(self, block, soff, device):
        self.device = int(device)
        self.n = soff.shape[0] - 1
        self.soff = soff
        self.frames = np.array([num_frames(n) for n in np.diff(soff)], dtype=np.int64)
        self.foff = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(self.frames, out=self.foff[1:])
        self.total_frames = int(self.foff[-1])
        self.wave = block
        self.mask = self.voiced = self.logmel = self.x = self.bn = self.out = None

    def vad(self):
        """(mask [total_frames] bool, voiced count per utterance [n] int32)"""
        self.mask = _backend.DeviceBuffer(max(16, self.total_frames), self.device)
        self.voiced = _backend.DeviceBuffer(max(16, 4 * self.n), self.device)
        _backend.check(_backend.lib().snf_bottleneck_vad(
            self.device, _p(self.wave), _off(self.soff), self.n, _p(self.mask), _p(self.voiced), None))
        counts = self.voiced.download(np.empty(self.n, dtype=np.int32))
        return counts

    def host_mask(self):
        return self.mask.download(np.empty(self.total_frames, dtype=np.uint8)).astype(bool)

    def fbank(self, dither=0.0, seed=_DITHER_SEED):
        tables = _device_array(self.device, _front_tables, self.device)
        self.logmel = _backend.DeviceBuffer(max(16, 4 * _NMEL * self.total_frames), self.device)
        _backend.check(_backend.lib().snf_bottleneck_fbank(
            self.device, _p(self.wave), _off(self.soff), self.n, _p(tables), float(dither), int(seed),
            _p(self.logmel), None))

    def host_logmel(self):
        return self.logmel.download(np.empty((self.total_frames, _NMEL), dtype=np.float32))

    def forward(self, dnet, precision='float32'):
        """Context projection and the two networks; returns the features [total rows, 80] float32 (host).
        `precision` 'bfloat16': W2, W3, W6 and W7 on the bfloat16 matrix cores"""
        _check_precision(precision)
        context = dnet.net.context
        basis = _device_array((self.device, context), lambda: _context_basis(context), self.device)
        rows = self.frames + 2 * _EDGE - 2 * context
        self.roff = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(rows, out=self.roff[1:])
        self.ooff = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(rows - 20, out=self.ooff[1:])
        r0, r1 = int(self.roff[-1]), int(self.ooff[-1])
        self.x = _backend.DeviceBuffer(max(16, 4 * _NIN * r0), self.device)
        L = _backend.lib()
        _backend.check(L.snf_bottleneck_nn_input(
            self.device, _p(self.logmel), _p(self.mask), _p(self.voiced), _off(self.foff), self.n, context,
            _p(basis), _p(self.x), None))
        self.bn = _backend.DeviceBuffer(max(16, 4 * _NDIMS * r0), self.device)
        self.out = _backend.DeviceBuffer(max(16, 4 * _NDIMS * r1), self.device)
        if precision == 'bfloat16':
            _backend.check(L.snf_bottleneck_forward_bf16(
                self.device, _p(self.x), _off(self.roff), self.n, dnet.widths, dnet.packed_pointers(), _p(self.bn),
                _p(self.out), None))
        else:
            _backend.check(L.snf_bottleneck_forward(
                self.device, _p(self.x), _off(self.roff), self.n, dnet.widths, dnet.pointers, _p(self.bn),
                _p(self.out), None))
        return self.out.download(np.empty((r1, _NDIMS), dtype=np.float32))

    def host_bn(self):
        return self.bn.download(np.empty((int(self.roff[-1]), _NDIMS), dtype=np.float32))

    def rows(self, context):
        """Output rows of every utterance: frames + 10 - 2 `context`"""
        return self.frames + 2 * _EDGE - 2 * int(context) - 20

    def extract(self, dnet, dither=0.0, precision='float32', out=None, out_offsets=None, scratch_bytes=0,
                seed=_DITHER_SEED):
        """The whole extractor in ONE call (``snf_bottleneck_extract``): VAD, front end, context projection and the
        two networks enqueued on one stream and waited for once, the intermediates in the calling thread's
        bounded scratch (`scratch_bytes`, 0 = the library's default) - the bits of :meth:`vad`, :meth:`fbank`
        and :meth:`forward` one after the other.  The rows of utterance u go to `out` (a DeviceBuffer of float32
        rows of 80; None: a new one that holds them end to end) from row ``out_offsets[u]`` on (None: end to
        end).  Returns ``(out, out_offsets, status)``: `status` [n] int32, bit 0 = no voiced frame, bit 1 = a
        value that is not finite (:func:`raise_for_status`).  Nothing is downloaded."""
        _check_precision(precision)
        context = dnet.net.context
        rows = self.rows(context)
        if out_offsets is None:
            out_offsets = np.zeros(self.n + 1, dtype=np.int64)
            np.cumsum(rows, out=out_offsets[1:])
        out_offsets = np.ascontiguousarray(out_offsets, dtype=np.int64)
        if out_offsets.shape != (self.n + 1,):
            raise ValueError(f'bottleneck: {self.n} utterances, {out_offsets.shape[0]} output offsets')
        if out is None:
            out = _backend.DeviceBuffer(max(16, 4 * _NDIMS * int(out_offsets[-1])), self.device)
        elif self.n and 4 * _NDIMS * int(out_offsets[-1]) > out.nbytes:
            raise ValueError('bottleneck: the output offsets reach past the output buffer')
        if self.n and 2 * int(self.soff[-1]) > self.wave.nbytes:
            raise ValueError('bottleneck: the sample offsets reach past the audio buffer')
        basis = _device_array((self.device, context), lambda: _context_basis(context), self.device)
        tables = _device_array(self.device, _front_tables, self.device)
        status = np.zeros(self.n, dtype=np.int32)
        bf16 = precision == 'bfloat16'
        _backend.check(_backend.lib().snf_bottleneck_extract(
            self.device, _p(self.wave), _off(self.soff), self.n, _p(tables), float(dither), int(seed), context,
            _p(basis), dnet.widths, dnet.packed_pointers() if bf16 else dnet.pointers, int(bf16), _p(out),
            _off(out_offsets), status.ctypes.data_as(C.POINTER(C.c_int32)), int(scratch_bytes), None))
        return out, out_offsets, status

    def runs(self, dnet, scratch_bytes=0):
        """First utterance of every run :meth:`extract` walks under `scratch_bytes`, then the number of utterances"""
        starts = np.zeros(self.n + 1, dtype=np.int64)
        count = int(_backend.lib().snf_bottleneck_extract_runs(
            _off(self.soff), self.n, dnet.net.context, dnet.widths, int(scratch_bytes), _off(starts)))
        if count < 0:
            _backend.check(count)
        return starts[:count + 1] if self.n else starts[:0]


def too_short_message(length, context, label=''):
    """The ValueError text for a signal of `length` samples at 8 kHz that gives no row of features; None when
    it gives some"""
    rows = num_frames(length) + 2 * _EDGE - 2 * context - 20
    if num_frames(length) >= 1 and rows >= 1:
        return None
    return 'signal{} too short: {} samples at 8 kHz give {} frames, one row of features needs {}'.format(
        label, length, num_frames(length), max(1, 2 * context + 21 - 2 * _EDGE))


def raise_for_status(status, names=None):
    """The processor's exceptions for the status words of :meth:`BottleneckBatch.extract`, the first utterance
    in order that has one: RuntimeError for an utterance without voiced frames, ValueError (the text of
    ``_backend._check_finite``) for values that are not finite"""
    for i in np.flatnonzero(status).tolist():
        if status[i] & 1:
            label = '' if names is None else ' "{}"'.format(names[i])
            raise RuntimeError('no voice detected in signal{}, failed to extract features'.format(label))
        if status[i] & 2:
            raise ValueError('data contains non-finite numbers (nan of infinity)')


def dense_layer(x, w, b, act='identity', device=None, precision='float32'):
    """``act(x @ w + b)`` on the device through ``snf_dense_layer`` (float32 host arrays in and out); with
    `precision` 'bfloat16' through ``snf_pack_weights_bf16`` and ``snf_dense_layer_bf16``: `x` and `w` rounded
    to bfloat16 on the device, float32 accumulation, bias, activation and result"""
    _check_precision(precision)
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if x.ndim != 2 or w.ndim != 2 or b.ndim != 1 or x.shape[1] != w.shape[0] or w.shape[1] != b.shape[0]:
        raise ValueError(f'dense layer: shapes {x.shape}, {w.shape}, {b.shape} do not fit')
    device = _backend.get_device() if device is None else int(device)
    bufs = []
    for a in (x, w, b):
        bufs.append(_backend.DeviceBuffer(max(16, a.nbytes), device))
        bufs[-1].upload(a)
    y = _backend.DeviceBuffer(max(16, 4 * x.shape[0] * w.shape[1]), device)
    if precision == 'bfloat16':
        image = pack_weights(bufs[1], w.shape[0], w.shape[1], device)
        _backend.check(_backend.lib().snf_dense_layer_bf16(
            device, _p(bufs[0]), x.shape[0], x.shape[1], _p(image), _p(bufs[2]), w.shape[1],
            {'identity': 0, 'sigmoid': 1}[act], _p(y), None))
    else:
        _backend.check(_backend.lib().snf_dense_layer(
            device, _p(bufs[0]), x.shape[0], x.shape[1], _p(bufs[1]), _p(bufs[2]), w.shape[1],
            {'identity': 0, 'sigmoid': 1}[act], _p(y), None))
    return y.download(np.empty((x.shape[0], w.shape[1]), dtype=np.float32))


class BottleneckProcessor(FeaturesProcessor):
    """Bottleneck features from a pre-trained neural network

    Parameters
    ----------
    weights : 'BabelMulti', 'FisherMono' or 'FisherTri'
        The pretrained weights to use for features extraction
    dither : float
        Amount of dithering, 0.0 means no dither

    Raises
    ------
    ValueError
        If the `weights` are invalid
    RuntimeError
        If no weights file can be found

    Beyond the reference, the attribute :attr:`precision` (not a constructor parameter) selects how the hidden
    layers are computed, and the attribute :attr:`resample` (not one either) where and how audio that is not at
    8 kHz is resampled.
    """
    def __init__(self, weights='BabelMulti', dither=0.1):
        super().__init__()
        self.weights = weights
        self.dither = dither
        self._precision = 'float32'
        self._resample = 'scipy'
        self._network()

    @property
    def name(self):
        return 'bottleneck'

    @property
    def dither(self):
        """Amount of dithering, 0.0 means no dither"""
        return self._dither

    @dither.setter
    def dither(self, value):
        self._dither = float(value)

    @property
    def weights(self):
        """The name of the pretrained weights used to extract the features"""
        return self._weights

    @weights.setter
    def weights(self, value):
        available = self.available_weights()
        if value not in available:
            raise ValueError('invalid weights "{}", choose in "{}"'.format(value, ', '.join(sorted(available.keys()))))
        self._weights = value

    @property
    def precision(self):
        """'float32' (default) or 'bfloat16': with 'bfloat16' the layers W2, W3, W6 and W7 round their
        activations and weights to bfloat16 and run on the bfloat16 matrix cores (float32 accumulation, bias,
        sigmoid and output); the features differ from the float32 ones by about 3e-3"""
        return self._precision

    @precision.setter
    def precision(self, value):
        self._precision = _check_precision(value)

    @property
    def resample(self):
        """'scipy' (default) or 'kaldi': how audio that is not at 8 kHz gets there.  'scipy' is
        :meth:`Audio.resample` on the host, one signal at a time, then the conversion to int16; 'kaldi'
        converts to int16 first, uploads a batch at its own rate and runs Kaldi's ResampleWaveform on the
        device (one more sample than the Fourier method for some lengths, and other values)"""
        return self._resample

    @resample.setter
    def resample(self, value):
        self._resample = _backend.check_resampler(value)

    def get_properties(self, **kwargs):
        """The processor's properties; they record the precision and the resampler when they are not the
        defaults"""
        if self._precision != 'float32':
            kwargs.setdefault('precision', self._precision)
        if self._resample != 'scipy':
            kwargs.setdefault('resample', self._resample)
        return super().get_properties(**kwargs)

    @property
    def ndims(self):
        """The dimension of extracted frames (fixed by the networks)"""
        return _NDIMS

    @property
    def sample_rate(self):
        """Processing sample frequency in Hertz (fixed by the networks)"""
        return 8000

    @property
    def frame_length(self):
        """The length of extracted frames in seconds (fixed by the networks)"""
        return 0.025

    @property
    def frame_shift(self):
        """The time shift between two consecutive frames in seconds (fixed by the networks)"""
        return 0.01

    @classmethod
    def available_weights(cls):
        """Return the pretrained weights files as a dict (name -> file)

        The files are searched in the directory named by ``SHENNONG_AMD_BOTTLENECK_DIR``, then in
        ``shennong_amd/share/bottleneck``.  Raises a RuntimeError if none of those directories exists or if
        they hold none of the files; logs a warning for every single missing file."""
        share = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'share', 'bottleneck')
        directories = [d for d in (os.environ.get(ENV_DIR), share) if d]
        existing = [d for d in directories if os.path.isdir(d)]
        if not existing:
            raise RuntimeError('directory not found: {}'.format(directories[0]))
        files = {}
        for name, stem in _FILES.items():
            for directory in existing:
                path = os.path.join(directory, stem + '.npz')
                if os.path.isfile(path):
                    files[name] = path
                    break
        if not files:
            raise RuntimeError('no weights file found in {}'.format(existing[0]))
        for name in _FILES:
            if name not in files and (name, tuple(existing)) not in _WARNED:
                # once per missing file, on the processor's logger as it is configured (get_logger would reset
                # the level a caller chose with set_logger)
                _WARNED.add((name, tuple(existing)))
                log = logging.getLogger('bottleneck')
                if not log.handlers:
                    log = get_logger('bottleneck', 'warning')
                log.warning('weights file for "%s" is unavailable', name)
        return files

    def _network(self):
        """The validated weights, loaded once per (name, file)"""
        path = self.available_weights()[self.weights]
        key = (self.weights, path)
        with _LOCK:
            net = _LOADED.get(key)
        if net is None:
            self.log.info('loading %s', os.path.basename(path))
            with np.load(path) as data:
                arrays = {k: v for k, v in data.items()}
            net = _Network(arrays, os.path.basename(path))
            with _LOCK:
                net = _LOADED.setdefault(key, net)
        return key, net

    def _device_network(self, device):
        key, net = self._network()
        with _LOCK:
            dnet = _DEVICE.get(key + (device,))
            if dnet is None:
                dnet = _DEVICE[key + (device,)] = _DeviceNetwork(net, device)
        return dnet

    def times(self, nframes):
        """(start, stop) of every output row in seconds"""
        start = np.arange(nframes) * _SHIFT
        return (1.0 / 8000) * np.vstack((start, start + _WIN)).T

    def _samples(self, signal):
        """`signal` as 8 kHz int16 samples (reference bottleneck.py:699-710)"""
        if signal.nchannels != 1:
            raise ValueError('signal must have one dimension, but it has {}'.format(signal.nchannels))
        if signal.sample_rate != 8000 or signal.dtype != np.dtype(np.int16):
            self.log.debug('resampling audio from %dHz@%db to %dHz@%db',
                           signal.sample_rate, signal.dtype.itemsize * 8, 8000, 16)
            if signal.sample_rate != 8000:
                signal = signal.resample(8000)
            signal = signal.astype(np.int16)
        return np.ascontiguousarray(signal.data).reshape(-1)

    def _samples_at_rate(self, signal):
        """`signal` as int16 samples at its own rate, and that rate (:attr:`resample` 'kaldi': the conversion
        to int16 comes before the resampling, which happens on the device)"""
        if signal.nchannels != 1:
            raise ValueError('signal must have one dimension, but it has {}'.format(signal.nchannels))
        if signal.sample_rate != 8000 or signal.dtype != np.dtype(np.int16):
            self.log.debug('resampling audio from %dHz@%db to %dHz@%db',
                           signal.sample_rate, signal.dtype.itemsize * 8, 8000, 16)
            signal = signal.astype(np.int16)
        return np.ascontiguousarray(signal.data).reshape(-1), signal.sample_rate

    def process(self, signal):
        """Computes bottleneck features on an audio `signal` (mono; resampled to 8 kHz int16 if needed)

        Returns Features of shape [nframes, 80], frame shift 10 ms, frame length 25 ms.  Raises a
        RuntimeError if no speech is detected in the signal, a ValueError if it is too short for one row."""
        return self._process_batch([signal])[0]

    def _process_batch(self, signals, names=None):
        device = _backend.get_device()
        dnet = self._device_network(device)
        context = dnet.net.context
        if self._resample == 'kaldi':
            waves, rates = zip(*[self._samples_at_rate(s) for s in signals]) if signals else ((), ())
            lengths = _backend.native_lengths(waves, rates, 8000)
        else:
            waves = [self._samples(s) for s in signals]
            lengths = [wave.shape[0] for wave in waves]

        def label(i):
            return '' if names is None else ' "{}"'.format(names[i])

        for i, length in enumerate(lengths):
            message = too_short_message(int(length), context, label(i))
            if message:
                raise ValueError(message)
        if self._resample == 'kaldi':
            batch = BottleneckBatch.from_device(*_backend.upload_resampled(waves, rates, 8000, lengths, device))
        else:
            batch = BottleneckBatch(waves, device)
        voiced = batch.vad()
        for i, count in enumerate(voiced):
            if not count:
                raise RuntimeError('no voice detected in signal{}, failed to extract features'.format(label(i)))
            self.log.debug('%d frames of speech detected (on %d total frames)', count, batch.frames[i])
        batch.fbank(self.dither)
        out = batch.forward(dnet, self._precision)
        _backend._check_finite(out)
        properties = self.get_properties()
        return [Features(out[a:b], self.times(b - a), properties, validate=False)
                for a, b in zip(batch.ooff[:-1], batch.ooff[1:])]

    def _process_all(self, utterances, **kwargs):
        if kwargs:
            raise ValueError('bottleneck features take no per-utterance argument: {}'.format(', '.join(kwargs)))
        utts = list(utterances)
        signals = [u._audio if type(u._audio) is Audio and not (u._tstart or u._tstop) else u.load_audio()
                   for u in utts]
        from shennong_amd.features import FeaturesCollection
        feats = self._process_batch(signals, names=[u.name for u in utts])
        return FeaturesCollection(zip([u.name for u in utts], feats))
