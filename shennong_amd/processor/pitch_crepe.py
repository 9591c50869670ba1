"""CREPE pitch: Audio ---> CrepePitchProcessor ---> Features ---> CrepePitchPostProcessor

The CREPE pitch tracker (Kim, Salamon, Li and Bello, "CREPE: A Convolutional Representation for Pitch
Estimation", ICASSP 2018): a network of six convolution blocks and one dense layer maps every frame of
1024 samples at 16 kHz to 360 pitch bins of 20 cents; the largest bin's value is the probability of voicing
and a local average around a bin (the largest one, or the one a Viterbi smoothing picks) is the pitch.  Same
parameters, properties and messages as the reference's processor/pitch_crepe.py (Keras and hmmlearn there);
here the framing, the network and the decoders are HIP kernels (``kernels_crepe.hip``): the convolutions run
as implicit GEMMs on the FP32 matrix cores, and ``process_all`` is one batched run over all utterances.

Beyond the reference: the attribute :attr:`CrepePitchProcessor.precision` (``'float32'`` by default) selects a
bfloat16 matrix-core path for convolution blocks 2 to 6, nine tenths of the arithmetic: their input
activations and kernels are rounded to bfloat16 (to nearest, ties to even) and the products accumulated in
float32; the ingest, block 1, the classifier, the decoders and the host tail are the float32 path unchanged.

Also beyond the reference: the attribute :attr:`CrepePitchProcessor.resample` (``'scipy'`` by default).  With
``'kaldi'`` audio that is not at 16 kHz is uploaded at its own rate and resampled on the device by Kaldi's
ResampleWaveform (``kernels_resample.hip``; cutoff 0.99 x half the lower rate, 6 zero crossings), a whole batch
per rate in one launch, straight into the batch's 16 kHz block; the samples are converted to int16 *before*
the resampling (after it on the default path) and the resampled length is Kaldi's.  The resampling of the
output rows to the row count (``scipy.signal.resample``, on the host) is another operation and stays as it is.

The pipeline's CREPE pitch entry (:mod:`shennong_amd.pipeline`) keeps everything after the decoder on the device
as well: :meth:`CrepeBatch.rows` (``snf_crepe_rows``: that row resampling and the clamp) and
:meth:`CrepeBatch.convert` (``snf_crepe_voicing_convert``: :func:`predict_voicing`, the interpolation and
:func:`pov_to_nccf` of :class:`CrepePitchPostProcessor`), ``kernels_crepe_tail.hip``.  The two processors below
keep their host tail.

Weights: the five pretrained models are not shipped with this package.  ``model-<capacity>.npz`` is looked up
in the directory named by the environment variable ``SHENNONG_AMD_CREPE_DIR`` and then in
``shennong_amd/share/crepe/``; ``tools/convert_crepe_h5.py`` writes that file from the published Keras
``model-<capacity>.h5``.

Differences from the reference: every frame is normalised on its own, as the CREPE package does (the
reference normalises in place through overlapping strided views of the signal, so a sample is shifted and
scaled once per frame that holds it), and the deviation is floored at 1e-8 as in the CREPE package, so digital
silence gives a finite activation instead of NaN; samples are taken as 16 bit integers like in every processor
of this package.  The output is float64 like the reference's.

>>> from shennong_amd import Audio
>>> from shennong_amd.processor import CrepePitchProcessor, CrepePitchPostProcessor
>>> audio = Audio.load('./tests/golden/test.wav')
>>> processor = CrepePitchProcessor(model_capacity='tiny', frame_shift=0.01)
>>> pitch = processor.process(audio)                          # doctest: +SKIP
>>> pitch.shape                                               # doctest: +SKIP
(140, 2)
>>> CrepePitchPostProcessor().process(pitch).shape            # doctest: +SKIP
(140, 3)
"""

import ctypes as C
import os
import threading

import numpy as np

from shennong_amd import _backend
from shennong_amd.audio import Audio
from shennong_amd.features import Features, FeaturesCollection
from shennong_amd.processor.base import FeaturesProcessor
from shennong_amd.processor.pitch_kaldi import KaldiPitchPostProcessor
from shennong_amd.utils import copy_properties

ENV_DIR = 'SHENNONG_AMD_CREPE_DIR'
CAPACITIES = {'tiny': 4, 'small': 8, 'medium': 16, 'large': 24, 'full': 32}
_BASE_FILTERS = (32, 4, 4, 4, 8, 16)
_WIDTHS = (512, 64, 64, 64, 64, 64)
_FRAME, _BINS, _EPSILON, _BAND = 1024, 360, 1e-3, 11
_BN = ('gamma', 'beta', 'moving_mean', 'moving_variance')
PRECISIONS = ('float32', 'bfloat16')
_PACKED = (4, 8, 12, 16, 20)    # the kernels of blocks 2 to 6 among the 26 parameters: the bfloat16 path's layers

_LOCK = threading.Lock()
_LOADED = {}    # (capacity, file) -> validated host parameters
_DEVICE = {}    # (capacity, file, device) -> uploaded parameters
_TABLES = {}    # device -> decoder tables


def filters(capacity):
    """Channels of the six convolution blocks of the model `capacity`"""
    return tuple(n * CAPACITIES[capacity] for n in _BASE_FILTERS)


def expected_shapes(capacity):
    """name -> shape of every array of ``model-<capacity>.npz`` (the Keras layer names)"""
    shapes, c_in = {}, 1
    for l, (c, w) in enumerate(zip(filters(capacity), _WIDTHS), 1):
        shapes[f'conv{l}/kernel'] = (w, 1, c_in, c)
        shapes[f'conv{l}/bias'] = (c,)
        for name in _BN:
            shapes[f'conv{l}-BN/{name}'] = (c,)
        c_in = c
    shapes['classifier/kernel'] = (4 * c_in, _BINS)
    shapes['classifier/bias'] = (_BINS,)
    return shapes


def model_path(capacity):
    """The weights file of `capacity`; raises a RuntimeError that names the path when it is not there"""
    share = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'share', 'crepe')
    candidates = [os.path.join(d, f'model-{capacity}.npz') for d in (os.environ.get(ENV_DIR), share) if d]
    for path in candidates:
        if os.path.isfile(path):
            return path
    raise RuntimeError(f'file not found: {candidates[0]}')


def _validate(arrays, capacity, origin):
    """The arrays of a weights file checked against the capacity; the 26 float32 arrays the device takes: per
    block kernel [width * C_in, C], bias, scale, shift (the inference form of the batch normalisation), then the
    classifier's kernel and bias"""
    shapes = expected_shapes(capacity)
    missing = sorted(set(shapes) - set(arrays))
    if missing:
        raise ValueError(f'{origin}: missing arrays {", ".join(missing)}')
    p = {}
    for name, shape in shapes.items():
        p[name] = np.asarray(arrays[name], dtype=np.float64)
        if p[name].shape != shape:
            raise ValueError(f'{origin}: array "{name}" has shape {p[name].shape}, expected {shape}')
        if not np.all(np.isfinite(p[name])):
            raise ValueError(f'{origin}: array "{name}" holds non-finite values')
    params = []
    for l in range(1, 7):
        variance = p[f'conv{l}-BN/moving_variance']
        if np.any(variance + _EPSILON <= 0):
            raise ValueError(f'{origin}: array "conv{l}-BN/moving_variance" must be above {-_EPSILON}')
        scale = p[f'conv{l}-BN/gamma'] / np.sqrt(variance + _EPSILON)
        shift = p[f'conv{l}-BN/beta'] - p[f'conv{l}-BN/moving_mean'] * scale
        kernel = p[f'conv{l}/kernel']
        params += [kernel.reshape(-1, kernel.shape[-1]), p[f'conv{l}/bias'], scale, shift]
    params += [p['classifier/kernel'], p['classifier/bias']]
    return [np.ascontiguousarray(a, dtype=np.float32) for a in params]


def load_model(capacity, path=None):
    """The validated float32 parameters of ``model-<capacity>.npz``, loaded once per file"""
    path = model_path(capacity) if path is None else path
    key = (capacity, path)
    with _LOCK:
        params = _LOADED.get(key)
    if params is None:
        with np.load(path) as data:
            arrays = {k: data[k] for k in data.files}
        params = _validate(arrays, capacity, os.path.basename(path))
        with _LOCK:
            params = _LOADED.setdefault(key, params)
    return key, params


class _DeviceModel:
    def __init__(self, capacity, params, device):
        self.buffers = []
        for a in params:
            buf = _backend.DeviceBuffer(max(16, a.nbytes), device)
            buf.upload(a)
            self.buffers.append(buf)
        self.pointers = (C.c_void_p * 26)(*[b.ptr for b in self.buffers])
        self.filters = (C.c_int32 * 6)(*filters(capacity))
        self.shapes = [a.shape for a in params]
        self.device = device
        self._packed = None

    def packed_pointers(self):
        """The 26 pointers with the kernels of blocks 2 to 6 as packed bfloat16 images (built on first use and
        kept beside the float32 weights)"""
        with _LOCK:
            if self._packed is None:
                pointers = [b.ptr for b in self.buffers]
                images = []
                for i in _PACKED:
                    images.append(pack_weights(self.buffers[i], *self.shapes[i], self.device))
                    pointers[i] = images[-1].ptr
                self._packed = (images, (C.c_void_p * 26)(*pointers))
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


def device_model(capacity, device, path=None):
    key, params = load_model(capacity, path)
    with _LOCK:
        model = _DEVICE.get(key + (device,))
        if model is None:
            model = _DEVICE[key + (device,)] = _DeviceModel(capacity, params, device)
    return model


def cents_mapping():
    """Cents of the 360 bins (reference pitch_crepe.py:190-191)"""
    return np.linspace(0, 7180, _BINS) + 1997.3794084376191


def decoder_tables():
    """The float64 table blob of ``snf_crepe_decode``: log transition band [360 x 23] | log start | log
    emission of the state's own symbol | of another symbol | cents of the bins (the model of reference
    pitch_crepe.py:218-235)"""
    index = np.arange(_BINS)
    transition = np.maximum(12 - np.abs(index[None, :] - index[:, None]), 0).astype(np.float64)
    transition = transition / np.sum(transition, axis=1)[:, None]
    emission = np.eye(_BINS) * 0.1 + np.ones((_BINS, _BINS)) * ((1 - 0.1) / _BINS)
    with np.errstate(divide='ignore'):
        log_transition = np.log(transition)
    band = np.full((_BINS, 2 * _BAND + 1), -np.inf)
    for d in range(2 * _BAND + 1):
        source = index - _BAND + d
        ok = (source >= 0) & (source < _BINS)
        band[index[ok], d] = log_transition[source[ok], index[ok]]
    head = [np.log(np.ones(_BINS) / _BINS)[0], np.log(emission[0, 0]), np.log(emission[0, 1])]
    return np.concatenate([band.reshape(-1), head, cents_mapping()])


def _device_tables(device):
    with _LOCK:
        buf = _TABLES.get(device)
        if buf is None:
            host = np.ascontiguousarray(decoder_tables(), dtype=np.float64)
            buf = _backend.DeviceBuffer(host.nbytes, device)
            buf.upload(host)
            _TABLES[device] = buf
        return buf


def num_frames(nsamples, hop, center=True):
    """Frames of 1024 samples every `hop` in `nsamples` samples (reference pitch_crepe.py:407-413)"""
    padded = nsamples + (_FRAME if center else 0)
    return 1 + (padded - _FRAME) // hop if padded >= _FRAME else 0


def _p(buf):
    return C.c_void_p(buf.ptr)


def _off(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


class CrepeBatch:
    """The stages of one batch of 16 kHz int16 utterances on the device, each one call through the C ABI:
    :meth:`forward` then :meth:`decode` (the tests and ``tools/time_crepe.py`` read the intermediate buffers),
    and the tail that stays on the device, :meth:`rows` then :meth:`convert` (the pipeline's CREPE entry)"""

    def __init__(self, waves, hop, center=True, device=None):
        device = _backend.get_device() if device is None else int(device)
        waves = [np.ascontiguousarray(w, dtype=np.int16).reshape(-1) for w in waves]
        soff = np.zeros(len(waves) + 1, dtype=np.int64)
        np.cumsum([w.shape[0] for w in waves], out=soff[1:])
        self._layout(_backend.upload_rows(waves, np.int16, device), soff, hop, center, device)
        self._owns_wave = True

    @classmethod
    def from_device(cls, block, soff, hop, center=True, device=None):
        """The batch over 16 kHz int16 audio that is already on the device: utterance u is the samples
        ``soff[u]:soff[u + 1]`` of the DeviceBuffer `block`"""
        batch = cls.__new__(cls)
        batch._layout(block, np.ascontiguousarray(soff, dtype=np.int64), hop, center,
                      block.device if device is None else device)
        batch._owns_wave = False   # (the caller's block)
        return batch

    def _layout(self, block, soff, hop, center, device):
        self.device = int(device)
        self.n, self.hop, self.center = soff.shape[0] - 1, int(hop), bool(center)
        self.soff = soff
        self.frames = np.array([num_frames(n, self.hop, self.center) for n in np.diff(soff)], dtype=np.int64)
        self.foff = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(self.frames, out=self.foff[1:])
        self.total_frames = int(self.foff[-1])
        self.wave = block
        self.activation = self.out = self.bins = self.resampled = self.nccf_pitch = None

    def forward(self, model, precision='float32'):
        """The activation [total_frames, 360] float32 stays on the device.  `precision` 'bfloat16': blocks 2 to 6
        on the bfloat16 matrix cores"""
        _check_precision(precision)
        self.activation = _backend.DeviceBuffer(max(16, 4 * _BINS * self.total_frames), self.device)
        L = _backend.lib()
        if precision == 'bfloat16':
            _backend.check(L.snf_crepe_forward_bf16(
                self.device, _p(self.wave), _off(self.soff), self.n, self.hop, int(self.center), model.filters,
                model.packed_pointers(), _p(self.activation), None))
        else:
            _backend.check(L.snf_crepe_forward(
                self.device, _p(self.wave), _off(self.soff), self.n, self.hop, int(self.center), model.filters,
                model.pointers, _p(self.activation), None))

    def set_activation(self, activation):
        """Replaces the network's output by a host matrix [total_frames, 360] (the decoder alone)"""
        activation = np.ascontiguousarray(activation, dtype=np.float32)
        if activation.shape != (self.total_frames, _BINS):
            raise ValueError(f'activation must have shape {(self.total_frames, _BINS)}, it has {activation.shape}')
        self.activation = _backend.DeviceBuffer(max(16, activation.nbytes), self.device)
        self.activation.upload(activation)

    def host_activation(self):
        return self.activation.download(np.empty((self.total_frames, _BINS), dtype=np.float32))

    def decode(self, viterbi=True, resident=False):
        """(confidence, Hertz) per frame [total_frames, 2] float64 (host); with `resident` nothing comes down
        (None): the rows stay on the device for :meth:`rows`"""
        tables = _device_tables(self.device)
        self.out = _backend.DeviceBuffer(max(16, 16 * self.total_frames), self.device)
        self.bins = _backend.DeviceBuffer(max(16, 8 * self.total_frames), self.device)
        _backend.check(_backend.lib().snf_crepe_decode(
            self.device, _p(self.activation), _off(self.foff), self.n, int(bool(viterbi)), _p(tables), _p(self.out),
            _p(self.bins), None))
        if resident:
            return None
        return self.out.download(np.empty((self.total_frames, 2), dtype=np.float64))

    def host_bins(self):
        """(first argmax, decoded bin) per frame, [2, total_frames] int32"""
        return self.bins.download(np.empty((2, self.total_frames), dtype=np.int32))

    # ---- the tail: decoder -> rows -> (NCCF, pitch), everything on the device -------------------------------
    def rows(self, out_counts):
        """The decoder's (confidence, Hertz) rows, which stay on the device (``decode(resident=True)``),
        resampled per utterance to `out_counts` rows by the Fourier method, confidence clamped
        (``snf_crepe_rows``); read them with :meth:`host_rows`"""
        counts = np.ascontiguousarray(out_counts, dtype=np.int64).reshape(-1)
        if counts.shape[0] != self.n:
            raise ValueError(f'{self.n} utterances, {counts.shape[0]} row counts')
        roff = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(counts, out=roff[1:])
        if self.out is None:
            raise ValueError('rows: nothing decoded yet')
        resampled = _backend.DeviceBuffer(max(16, 16 * int(roff[-1])), self.device)
        try:
            _backend.check(_backend.lib().snf_crepe_rows(
                self.device, _p(self.out), _off(self.foff), _off(roff), self.n, _p(resampled), None))
        except BaseException:
            resampled.free()
            raise
        old, self.resampled = self.resampled, resampled
        if old is not None and old is not self.out:   # (the rows of an earlier call; set_rows' block is `out` too)
            old.free(synced=True)                     # (that call returned: its stream is synchronised)
        self.roff, self.total_rows = roff, int(roff[-1])

    def set_rows(self, rows, offsets):
        """Replaces the decoder's output by the host matrix `rows` [total, 2] float64, utterance u being the
        rows ``offsets[u]:offsets[u + 1]``: both as the input of :meth:`rows` and as its result (the tail's
        kernels alone, no network)"""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if rows.ndim != 2 or rows.shape[1] != 2 or offsets.shape[0] != self.n + 1 or offsets[-1] != rows.shape[0]:
            raise ValueError(f'rows must have shape [total, 2] and {self.n + 1} offsets that end at total')
        self.foff, self.total_frames = offsets, int(offsets[-1])
        self.frames = np.diff(offsets)
        uploaded = _backend.DeviceBuffer(max(16, rows.nbytes), self.device)
        uploaded.upload(rows)
        replaced = {id(b): b for b in (self.out, self.resampled) if b is not None}
        self.out = self.resampled = uploaded
        for block in replaced.values():
            block.free(synced=True)   # (the calls that used them returned: their streams are synchronised)
        self.roff, self.total_rows = offsets, self.total_frames

    def host_rows(self):
        """The rows :meth:`rows` made, [total_rows, 2] float64"""
        return self.resampled.download(np.empty((self.total_rows, 2), dtype=np.float64))

    def convert(self):
        """The (NCCF, pitch) float32 rows the Kaldi post-processing takes, from the rows of :meth:`rows`
        (``snf_crepe_voicing_convert``): they stay on the device (:attr:`nccf_pitch`, :meth:`host_nccf_pitch`),
        the status of every utterance comes down and the first that is not 0 raises what
        :class:`CrepePitchPostProcessor` raises for such an utterance"""
        if getattr(self, 'resampled', None) is None:
            raise ValueError('convert: no rows yet')
        nccf_pitch = _backend.DeviceBuffer(max(16, 8 * self.total_rows), self.device)
        status = _backend.DeviceBuffer(max(16, 4 * self.n), self.device)
        try:
            model = voicing_model()
            _backend.check(_backend.lib().snf_crepe_voicing_convert(
                self.device, _p(self.resampled), _off(self.roff), self.n,
                model.ctypes.data_as(C.POINTER(C.c_double)), _p(nccf_pitch), _p(status), None))
            self.status = status.download(np.empty(self.n, dtype=np.int32))
        except BaseException:
            nccf_pitch.free()
            raise
        finally:
            status.free()
        old, self.nccf_pitch = getattr(self, 'nccf_pitch', None), nccf_pitch
        if old is not None:
            old.free(synced=True)
        _raise_for_status(self.status)

    def host_nccf_pitch(self):
        """The rows :meth:`convert` made, [total_rows, 2] float32"""
        return self.nccf_pitch.download(np.empty((self.total_rows, 2), dtype=np.float32))

    def release(self, synced=False):
        """Gives the batch's device blocks back - the audio too when the batch uploaded it itself, not when it
        is the caller's (:meth:`from_device`).  `synced`: every call that used them has returned, and each
        waits for its stream (see ``DeviceBuffer.free``)"""
        names = ('activation', 'out', 'bins', 'resampled', 'nccf_pitch')
        for name in names + (('wave',) if getattr(self, '_owns_wave', False) else ()):
            block = getattr(self, name, None)
            setattr(self, name, None)
            if block is not None:
                block.free(synced=synced)   # (a second free of a block held under two names is a no-op)


_STATUS_MESSAGES = {
    1: 'No voiced frames',
    2: 'Not all pitch values are positive: issue with extracted pitch or interpolation',
    3: 'f(a) and f(b) must have different signs'}


def _raise_for_status(status):
    """The exception of the first utterance whose status (``snf_crepe_voicing_convert``) is not 0: the texts of
    :meth:`CrepePitchPostProcessor._convert` and :func:`pov_to_nccf`"""
    for code in np.asarray(status).reshape(-1).tolist():
        if code:
            if code not in _STATUS_MESSAGES:
                raise RuntimeError(f'crepe conversion: unknown status {code}')
            raise ValueError(_STATUS_MESSAGES[code])


def voicing_model():
    """The float64 model ``snf_crepe_voicing_convert`` takes, with the values :func:`predict_voicing` and
    :func:`pov_to_nccf` compute: log(2 pi variance), the two means, the variance, log start, the log transition
    matrix by rows, then the range of the NCCF -> POV map"""
    variance = 0.25
    log_transition = np.log(np.array([[0.99, 0.01], [0.01, 0.99]]))
    return np.ascontiguousarray(np.concatenate([
        [np.log(2 * np.pi * variance), 0.0, 1.0, variance, np.log(0.5)], log_transition.reshape(-1),
        [_nccf_to_pov(0.0), _nccf_to_pov(1.0)]]), dtype=np.float64)


def _to_bf16_bits(a):
    """The upper halves of float32 values that bfloat16 holds exactly"""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    if (bits & np.uint32(0xFFFF)).any():
        raise ValueError('convolution: a bfloat16 source must hold values that bfloat16 represents exactly')
    return (bits >> np.uint32(16)).astype(np.uint16)


def conv_layer(x, kernel, bias, scale=None, shift=None, stride=1, pad_left=31, pool=True, sigmoid=False,
               device=None, precision='float32', source='float32', store='float32'):
    """One convolution block on the device through ``snf_crepe_conv``: `x` [frames, length, C_in], `kernel`
    [width, C_in, C_out]; ReLU and ``* scale + shift`` when `scale` is given, then the pool or the sigmoid.

    With `precision` 'bfloat16' through ``snf_pack_weights_bf16`` and ``snf_crepe_conv_bf16``: `x` and `kernel`
    rounded to bfloat16 on the device, everything after the products float32.  `source` 'bfloat16' uploads `x`
    as bfloat16 (its values must be exact in that format), `store` 'bfloat16' has the device round the result
    to bfloat16 on the way out; float32 host arrays in and out either way."""
    _check_precision(precision)
    _check_precision(source)
    _check_precision(store)
    if precision == 'float32' and (source, store) != ('float32', 'float32'):
        raise ValueError('convolution: bfloat16 source and store belong to precision "bfloat16"')
    x = np.ascontiguousarray(x, dtype=np.float32)
    kernel = np.ascontiguousarray(kernel, dtype=np.float32)
    if x.ndim != 3 or kernel.ndim != 3 or kernel.shape[1] != x.shape[2]:
        raise ValueError(f'convolution: shapes {x.shape}, {kernel.shape} do not fit')
    frames, length, c_in = x.shape
    width, _, c_out = kernel.shape
    positions = -(-length // stride)
    flags = (1 if scale is not None else 0) | (2 if pool else 0) | (4 if sigmoid else 0)
    hosts = [_to_bf16_bits(x) if source == 'bfloat16' else x, kernel, np.ascontiguousarray(bias, dtype=np.float32)]
    hosts += [np.ascontiguousarray(a, dtype=np.float32) for a in ([scale, shift] if scale is not None else [])]
    device = _backend.get_device() if device is None else int(device)
    bufs = []
    for a in hosts:
        bufs.append(_backend.DeviceBuffer(max(16, a.nbytes), device))
        bufs[-1].upload(a)
    rows = positions // 2 if pool else positions
    out = np.empty((frames, rows, c_out), dtype=np.uint16 if store == 'bfloat16' else np.float32)
    y = _backend.DeviceBuffer(max(16, out.nbytes), device)
    norm = [_p(bufs[3]), _p(bufs[4])] if scale is not None else [None, None]
    if precision == 'bfloat16':
        image = pack_weights(bufs[1], width * c_in, c_out, device)
        _backend.check(_backend.lib().snf_crepe_conv_bf16(
            device, _p(bufs[0]), PRECISIONS.index(source), frames, length, c_in, width, stride, pad_left, positions,
            _p(image), _p(bufs[2]), *norm, c_out, flags, _p(y), PRECISIONS.index(store), None))
    else:
        _backend.check(_backend.lib().snf_crepe_conv(
            device, _p(bufs[0]), frames, length, c_in, width, stride, pad_left, positions, _p(bufs[1]), _p(bufs[2]),
            *norm, c_out, flags, _p(y), None))
    y.download(out)
    return (out.astype(np.uint32) << np.uint32(16)).view(np.float32) if store == 'bfloat16' else out


class CrepePitchProcessor(FeaturesProcessor):
    """Extracts the (POV, pitch) per frame from a speech signal

    This processor uses the pre-trained CREPE model. The output will have as many rows as there are frames,
    and two columns corresponding to (POV, pitch). POV is the Probability of Voicing.

    Beyond the reference, the attribute :attr:`precision` (not a constructor parameter) selects how convolution
    blocks 2 to 6 are computed, and the attribute :attr:`resample` (not one either) where and how audio that is
    not at 16 kHz is resampled.
    """
    def __init__(self, model_capacity='full', viterbi=True, center=True,
                 frame_shift=0.01, frame_length=0.025):
        super().__init__()
        self._precision = 'float32'
        self._resample = 'scipy'
        self.model_capacity = model_capacity
        self.viterbi = viterbi
        self.center = center
        self.frame_shift = frame_shift
        self.frame_length = frame_length

    @property
    def name(self):
        return 'crepe'

    @property
    def model_capacity(self):
        """String specifying the model capacity to use: 'tiny', 'small', 'medium', 'large' or 'full' (capacity
        multipliers 4, 8, 16, 24 and 32; 'full' is the model of the paper)"""
        return self._model_capacity

    @model_capacity.setter
    def model_capacity(self, value):
        if value not in ['tiny', 'small', 'medium', 'large', 'full']:
            raise ValueError(f'Model capacity {value} is not recognized.')
        self._model_capacity = value

    @property
    def viterbi(self):
        """Whether to apply viterbi smoothing to the estimated pitch curve"""
        return self._viterbi

    @viterbi.setter
    def viterbi(self, value):
        self._viterbi = bool(value)

    @property
    def center(self):
        """Whether to center the window on the current frame: when True frame `t` is centered at
        ``audio[t * hop_length]``, when False it begins there"""
        return self._center

    @center.setter
    def center(self, value):
        self._center = bool(value)

    @property
    def frame_shift(self):
        """Frame shift in seconds for running pitch estimation"""
        return self._frame_shift

    @frame_shift.setter
    def frame_shift(self, value):
        self._frame_shift = value

    @property
    def frame_length(self):
        """Frame length in seconds"""
        return self._frame_length

    @frame_length.setter
    def frame_length(self, value):
        self._frame_length = value

    @property
    def precision(self):
        """'float32' (default) or 'bfloat16': with 'bfloat16' convolution blocks 2 to 6 round their input
        activations and kernels to bfloat16 and run on the bfloat16 matrix cores (float32 accumulation, bias,
        ReLU, normalisation and pool); the activation differs from the float32 one by about 2e-3"""
        return self._precision

    @precision.setter
    def precision(self, value):
        self._precision = _check_precision(value)

    @property
    def resample(self):
        """'scipy' (default) or 'kaldi': how audio that is not at 16 kHz gets there.  'scipy' is
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
    def sample_rate(self):
        """CREPE operates at 16kHz"""
        return 16000

    @property
    def ndims(self):
        return 2

    def times(self, nframes):
        """Returns the time label for the rows given by :func:`process`"""
        return np.vstack((
            np.arange(nframes) * self.frame_shift,
            np.arange(nframes) * self.frame_shift + self.frame_length)).T

    def _samples(self, audio):
        """`audio` as 16 kHz int16 samples (reference pitch_crepe.py:449-455)"""
        if audio.nchannels != 1:
            raise ValueError(f'audio must have one channel but has {audio.nchannels}')
        if audio.sample_rate != self.sample_rate:
            self.log.debug('resampling audio to 16 kHz')
            audio = audio.resample(self.sample_rate)
        return np.ascontiguousarray(audio.astype(np.int16).data).reshape(-1)

    def _samples_at_rate(self, audio):
        """`audio` as int16 samples at its own rate, and that rate (:attr:`resample` 'kaldi': the conversion
        to int16 comes before the resampling, which happens on the device)"""
        if audio.nchannels != 1:
            raise ValueError(f'audio must have one channel but has {audio.nchannels}')
        if audio.sample_rate != self.sample_rate:
            self.log.debug('resampling audio to 16 kHz')
        return np.ascontiguousarray(audio.astype(np.int16).data).reshape(-1), audio.sample_rate

    def _output_rows(self, nsamples):
        """Rows of the output for a signal of `nsamples` at 16 kHz (reference pitch_crepe.py:473-476)"""
        hop = np.round(self.sample_rate * self.frame_shift).astype(int)
        return 1 + int((nsamples - self.frame_length * self.sample_rate) / hop)

    def process(self, audio):
        """Extracts the (POV, pitch) from a given speech ``audio`` using CREPE (mono; resampled to 16 kHz if
        needed).  Returns Features of shape [nframes, 2]: the network's frames, one every `frame_shift` over the
        (padded) signal, are brought to the row count `frame_shift` and `frame_length` define by the Fourier
        method, like the reference does."""
        return self._process_batch([audio])[0]

    def _process_batch(self, signals, names=None):
        import scipy.signal
        if self._resample == 'kaldi':
            waves, rates = zip(*[self._samples_at_rate(s) for s in signals]) if signals else ((), ())
            lengths = _backend.native_lengths(waves, rates, self.sample_rate)
        else:
            waves = [self._samples(s) for s in signals]
            lengths = [wave.shape[0] for wave in waves]
        hop = int(self.sample_rate * self.frame_shift)
        if hop < 1:
            raise ValueError(f'frame_shift must be at least one sample at 16 kHz, it is {self.frame_shift}')
        for i, length in enumerate(lengths):
            if num_frames(length, hop, self.center) < 1 or self._output_rows(length) < 1:
                label = '' if names is None else ' "{}"'.format(names[i])
                raise ValueError(f'audio{label} too short: {length} samples at 16 kHz')
        device = _backend.get_device()
        model = device_model(self.model_capacity, device)
        if self._resample == 'kaldi':
            batch = CrepeBatch.from_device(
                *_backend.upload_resampled(waves, rates, self.sample_rate, lengths, device), hop, self.center)
        else:
            batch = CrepeBatch(waves, hop, self.center, device)
        batch.forward(model, self._precision)
        raw = batch.decode(self.viterbi)
        properties = self.get_properties()
        feats = []
        for length, a, b in zip(lengths, batch.foff[:-1], batch.foff[1:]):
            data = scipy.signal.resample(raw[a:b], self._output_rows(length))
            # hack needed because resample confidence
            data[data[:, 0] < 1e-2, 0] = 0
            data[data[:, 0] > 1, 0] = 1
            feats.append(Features(data, self.times(data.shape[0]), properties=properties))
        return feats

    def _process_all(self, utterances, **kwargs):
        if kwargs:
            raise ValueError('crepe pitch takes no per-utterance argument: {}'.format(', '.join(kwargs)))
        utts = list(utterances)
        signals = [u._audio if type(u._audio) is Audio and not (u._tstart or u._tstop) else u.load_audio()
                   for u in utts]
        feats = self._process_batch(signals, names=[u.name for u in utts])
        return FeaturesCollection(zip([u.name for u in utts], feats))


def _nccf_to_pov(x):
    """From normalized cross correlation to probability of voicing (Ghahremani et al., "A pitch extraction
    algorithm tuned for automatic speech recognition", ICASSP 2014)"""
    y = -5.2 + 5.4 * np.exp(7.5 * (x - 1)) + 4.8 * x - 2 * np.exp(-10 * x) + 4.2 * np.exp(20 * (x - 1))
    return 1 / (1 + np.exp(-y))


def pov_to_nccf(pov):
    """The NCCF in [0, 1] whose probability of voicing is `pov`: 0 and 1 map to themselves, anything between by
    bisection of the increasing map above (64 halvings of [0, 1]; the reference calls scipy.optimize.bisect per
    frame).  Raises a ValueError, like that call, for a value outside the map's range."""
    pov = np.asarray(pov, dtype=np.float64)
    fixed = (pov == 0) | (pov == 1)
    if np.any(~fixed & ((pov <= _nccf_to_pov(0.0)) | (pov >= _nccf_to_pov(1.0)))):
        raise ValueError('f(a) and f(b) must have different signs')
    lo, hi = np.zeros(pov.shape), np.ones(pov.shape)
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        below = _nccf_to_pov(mid) < pov
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return np.where(fixed, pov, 0.5 * (lo + hi))


def predict_voicing(confidence):
    """Most likely voiced (1) / unvoiced (0) state per frame under the reference's two-state model: Gaussian
    emissions of mean 0 and 1 and variance 0.25, self transition 0.99, uniform start (reference
    pitch_crepe.py:256-291); float64 log domain, first index on ties"""
    confidence = np.asarray(confidence, dtype=np.float64).reshape(-1)
    n = confidence.shape[0]
    if n == 0:
        return np.zeros(0, dtype=int)
    means, variance = np.array([0.0, 1.0]), 0.25
    log_emission = -0.5 * (np.log(2 * np.pi * variance) + (confidence[:, None] - means[None, :]) ** 2 / variance)
    log_transition = np.log(np.array([[0.99, 0.01], [0.01, 0.99]]))
    lattice = np.empty((n, 2))
    lattice[0] = np.log(0.5) + log_emission[0]
    for t in range(1, n):
        lattice[t] = (lattice[t - 1][:, None] + log_transition).max(axis=0) + log_emission[t]
    states = np.empty(n, dtype=int)
    states[-1] = int(np.argmax(lattice[-1]))
    for t in range(n - 2, -1, -1):
        states[t] = int(np.argmax(lattice[t] + log_transition[:, states[t + 1]]))
    return states


class CrepePitchPostProcessor(KaldiPitchPostProcessor):
    """Processes the raw (POV, pitch) computed by the CrepePitchProcessor

    Converts the POV into the NCCF the Kaldi post-processing expects, replaces the pitch of the frames the
    voicing model calls unvoiced by interpolated values, and hands the (NCCF, pitch) pair to
    :class:`KaldiPitchPostProcessor` (the same device kernel).
    """
    name = 'crepe postprocessing'

    def __init__(self, pitch_scale=2.0, delta_pitch_scale=10.0,
                 delta_pitch_noise_stddev=0.005,
                 normalization_left_context=75, normalization_right_context=75,
                 delta_window=2, delay=0,
                 add_pov_feature=True, add_normalized_log_pitch=True,
                 add_delta_pitch=True, add_raw_log_pitch=False):
        super().__init__(
            pitch_scale=pitch_scale,
            delta_pitch_scale=delta_pitch_scale,
            delta_pitch_noise_stddev=delta_pitch_noise_stddev,
            normalization_left_context=normalization_left_context,
            normalization_right_context=normalization_right_context,
            delta_window=delta_window,
            delay=delay,
            add_pov_feature=add_pov_feature,
            add_normalized_log_pitch=add_normalized_log_pitch,
            add_delta_pitch=add_delta_pitch,
            add_raw_log_pitch=add_raw_log_pitch)

    def get_properties(self, features):
        properties = copy_properties(features.properties)
        properties['crepe'][self.name] = self.get_params()
        properties['pipeline'][0]['columns'] = [0, self.ndims - 1]
        return properties

    def _convert(self, crepe_pitch):
        """The (NCCF, pitch) input of the Kaldi post-processing (reference pitch_crepe.py:572-606)"""
        to_remove = predict_voicing(crepe_pitch.data[:, 0]) == 0
        if np.all(to_remove):
            raise ValueError('No voiced frames')
        data = np.array(crepe_pitch.data[:, 1], dtype=np.float64)
        keep = np.where(~to_remove)[0]
        first, last = keep[0], keep[-1]
        first_value, last_value = data[first], data[last]
        data[to_remove] = np.interp(np.where(to_remove)[0], keep, data[keep])
        data[:first] = first_value
        data[last:] = last_value
        if not np.all(data > 0):
            raise ValueError('Not all pitch values are positive: issue with extracted pitch or interpolation')
        nccf = pov_to_nccf(crepe_pitch.data[:, 0])
        return Features(np.ascontiguousarray(np.vstack((nccf, data)).T, dtype=np.float32), crepe_pitch.times, crepe_pitch.properties, validate=False)

    def _process_batch(self, raw_pitches):
        for raw in raw_pitches:
            self._check(raw)
        return super()._process_batch([self._convert(raw) for raw in raw_pitches])
