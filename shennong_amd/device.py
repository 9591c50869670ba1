"""Features that stay on the GPU: device-resident collections, their DLPack export and padded batches

An extension with no counterpart in the reference, which returns numpy arrays.  ``process_all`` and
``extract_features`` end in a download into page-locked host memory; a consumer that trains or evaluates a
model on the same MI355X then uploads the same rows again.  ``FeaturesProcessor.process_all_device`` and
``pipeline.extract_features_device`` skip that download and return a :class:`DeviceFeaturesCollection`:

    feats = processor.process_all_device(utterances)       # name -> DeviceFeatures, rows in HBM
    feats['utt1'].shape, feats['utt1'].times                # metadata as on the host, made when read
    batch = feats.padded(dtype='bfloat16', left=1, right=1, subsample=3)   # [B, T, 3 dim] + lengths, one kernel
    x = torch.from_dlpack(batch)                            # zero copy (see `shares_hip_runtime_with_torch`)
    feats.to_host()                                         # the FeaturesCollection the host call returns

Ownership.  A collection owns its block(s) of HBM; every :class:`DeviceFeatures` is a row-block view that
keeps its block alive, and so does every DLPack export until the consumer's tensor dies.  A block goes back to
the device pool only through the waiting form of ``DeviceBuffer.free``: a consumer framework calls the DLPack
deleter without synchronising its own streams, so the device is idle before the memory is handed out again.

Streams.  Every block is complete when the call that made it returns (one wait at its end), so the `stream`
argument of ``__dlpack__`` needs no action: there is nothing left to order the consumer's stream behind.
"""

import os

import numpy as np

from shennong_amd import _backend, _dlpack
from shennong_amd.features import Features, FeaturesCollection

_NUMPY_OF = {'float32': np.float32, 'float16': np.float16, 'bfloat16': np.uint16, 'int32': np.int32}


def mapped_hip_runtimes():
    """The distinct ``libamdhip64`` files mapped into this process (real paths, sorted)"""
    found = set()
    try:
        with open('/proc/self/maps') as maps:
            for line in maps:
                fields = line.split(None, 5)   # (address, permissions, offset, device, inode, path)
                path = fields[5].strip() if len(fields) == 6 else ''
                if os.path.basename(path).startswith('libamdhip64'):
                    found.add(os.path.realpath(path))
    except OSError:   # pragma: nocover (no procfs)
        pass
    return sorted(found)


def shares_hip_runtime_with_torch():
    """``(shared, paths)``: whether torch and libshennong_hip.so run on ONE HIP runtime in this process, and the
    ``libamdhip64`` files that are mapped once both are loaded.  The torch wheels bring a runtime of their own;
    which one libshennong_hip.so binds to depends on what was loaded first: after
    ``import torch`` the library resolves its ``libamdhip64.so.7`` to the copy torch has already mapped (one
    runtime, pointers can be shared); loaded before torch, it has the system's runtime and torch then maps its
    own beside it (two runtimes: a pointer of one means nothing to the other).  Needs no device.  Without torch
    the answer is ``(False, paths)``."""
    try:
        import torch  # noqa: F401
    except ImportError:
        _backend.lib()
        return False, mapped_hip_runtimes()
    _backend.lib()
    paths = mapped_hip_runtimes()
    return len(paths) == 1, paths


def _to_torch(array):
    try:
        import torch
    except ImportError:
        raise RuntimeError('torch is not installed') from None
    shared, paths = shares_hip_runtime_with_torch()
    if not shared:
        raise RuntimeError(
            'torch and libshennong_hip.so do not share one HIP runtime in this process (mapped: {}): a device '
            'pointer of one is not valid in the other.  Import torch before shennong_amd loads its library, or '
            'copy through the host (to_host)'.format(', '.join(paths) or 'none'))
    return torch.from_dlpack(array)


class _Block:
    """One device block of a collection.  `buffer` is the DeviceBuffer until the collection is released; exports
    hold the DeviceBuffer itself, whose last reference gives the memory back (DeviceBuffer.__del__: the waiting
    free)."""
    __slots__ = ('buffer', 'names', 'dim', 'foff')

    def __init__(self, buffer, names, dim, foff):
        self.buffer, self.names, self.dim, self.foff = buffer, names, int(dim), foff

    def alive(self):
        buffer = self.buffer
        if buffer is None or not buffer.ptr:
            raise RuntimeError('the device block has been released')
        return buffer


class DeviceArray:
    """A row-major array in HBM: `shape`, `dtype` (a name: 'float32', 'float16', 'bfloat16', 'int32'), `ptr`,
    `device`, and the DLPack protocol.  Keeps its block alive."""
    __slots__ = ('_block', '_offset', 'shape', 'dtype')

    def __init__(self, block, offset, shape, dtype):
        self._block, self._offset = block, int(offset)
        self.shape, self.dtype = tuple(int(x) for x in shape), dtype

    @property
    def ptr(self):
        """Device address of the first element"""
        return self._block.alive().ptr + self._offset

    @property
    def device(self):
        return self._block.alive().device

    def __dlpack_device__(self):
        return (_dlpack.kDLROCM, self.device)

    def __dlpack__(self, stream=None):
        """A ``dltensor`` capsule over these elements (kDLROCM).  `stream` needs no action: the block was
        complete when the call that made it returned."""
        buffer = self._block.alive()
        return _dlpack.export(buffer.ptr + self._offset, self.shape, self.dtype, _dlpack.kDLROCM, buffer.device,
                              owner=buffer)

    def torch(self):
        """``torch.from_dlpack(self)``; RuntimeError when torch runs on another HIP runtime than the library"""
        return _to_torch(self)

    def numpy(self):
        """A host copy (bfloat16 comes back as its uint16 bit patterns: numpy has no such type)"""
        out = np.empty(self.shape, dtype=_NUMPY_OF[self.dtype])
        if out.size:
            buffer = self._block.alive()
            _backend.bind_device(buffer.device)
            _backend.check(_backend.lib().snf_memcpy_d2h(out.ctypes.data, buffer.ptr + self._offset, out.nbytes))
        return out


class DeviceFeatures(DeviceArray):
    """The features of one utterance in HBM: a row-block view of its collection's block with the `times` and
    `properties` of the host object (made when first read, like there)"""
    __slots__ = ('_shared', '_host_shape', '_meta')

    def __init__(self, block, row0, nframes, shared, host_shape):
        # (one of these per utterance of a corpus: plain assignments)
        self._block, self._offset = block, 4 * row0 * block.dim
        self.shape, self.dtype = (nframes, block.dim), 'float32'
        self._shared, self._host_shape, self._meta = shared, host_shape, None

    # (what the host call reports: an utterance without frames has Kaldi's (0, 0) matrix there)
    nframes = property(lambda self: self.shape[0])
    ndims = property(lambda self: self._host_shape[1])

    def _host_meta(self):
        if self._meta is None:
            self._meta = Features._of_batch(None, *self._shared)
        return self._meta

    times = property(lambda self: self._host_meta().times, doc='The times of the rows, as on the host')
    properties = property(lambda self: self._host_meta().properties, doc='How the features were made')

    def to_host(self):
        """The :class:`Features` the host call returns for this utterance"""
        data = self.numpy() if self.shape[0] else np.zeros(self._host_shape, dtype=np.float32)
        return Features._of_batch(data, *self._shared)


class DeviceBatch:
    """A padded batch in HBM (``DeviceFeaturesCollection.padded``): `data` [B, T, D'] and `lengths` [B] int32
    (:class:`DeviceArray`), `names` the utterances in batch order.  Exports like its `data`."""
    def __init__(self, data, lengths, names, times, subsample, offset):
        self.data, self.lengths, self.names = data, lengths, list(names)
        self._times, self._subsample, self._offset = times, subsample, offset

    shape = property(lambda self: self.data.shape)
    dtype = property(lambda self: self.data.dtype)

    def times_of(self, name):
        """The times of the frames kept of utterance `name` (rows offset, offset + subsample, ...)"""
        return self._times[name][self._offset::self._subsample].copy()

    def __dlpack__(self, stream=None):
        return self.data.__dlpack__(stream)

    def __dlpack_device__(self):
        return self.data.__dlpack_device__()

    def torch(self):
        """`data` as a torch tensor (``batch.lengths.torch()`` for the lengths)"""
        return self.data.torch()


class DeviceFeaturesCollection(dict):
    """``name -> DeviceFeatures`` in input order; owns the device block(s) the rows lie in (one per sample rate
    of the corpus: one, nearly always)"""
    @classmethod
    def _build(cls, template, blocks):
        """`template`: the host collection of the call with placeholder data (shapes, shared times and
        properties); `blocks`: ``(DeviceBuffer, names in row order, dim)`` per block"""
        self = cls()
        self._blocks = []
        made = {}
        for buffer, names, dim in blocks:
            hosts = [template[name] for name in names]
            shapes = [host._data.shape for host in hosts]
            counts = [shape[0] for shape in shapes]
            rows = np.zeros(len(names) + 1, dtype=np.int64)
            np.cumsum(counts, out=rows[1:])
            block = _Block(buffer, list(names), dim, rows)
            self._blocks.append(block)
            for name, host, row0, count, shape in zip(names, hosts, rows[:-1].tolist(), counts, shapes):
                made[name] = DeviceFeatures(block, row0, count, host._shared, shape)
        for name in template:
            self[name] = made[name]
        return self

    @classmethod
    def from_host(cls, collection, device=None):
        """The host :class:`FeaturesCollection` `collection` (features read from a file, say) as a device
        collection in ONE block, uploaded once (``_backend.upload_rows``); ``to_host()`` of the result gives equal
        Features.  ValueError, before any device work, for utterances of different `ndims` and for data that is
        not a float32 matrix."""
        names = list(collection)
        for name in names:
            data = collection[name].data
            if not isinstance(data, np.ndarray) or data.ndim != 2 or data.dtype != np.float32:
                raise ValueError(f'utterance "{name}": data must be a float32 matrix [nframes, ndims]')
        dims = sorted({collection[name].ndims for name in names if collection[name].nframes})
        if len(dims) > 1:
            raise ValueError('utterances have different ndims: {}'.format(dims))
        dim = dims[0] if dims else (collection[names[0]].ndims if names else 0)
        template = FeaturesCollection()
        for name in names:
            host = collection[name]
            shape = host.data.shape
            placeholder = np.broadcast_to(np.float32(0), shape) if shape[0] else np.zeros(shape, dtype=np.float32)
            template[name] = Features._of_batch(placeholder, host._times_view(), host.properties, None)
        mats = [collection[name].data for name in names if collection[name].nframes]
        buffer = _backend.upload_rows(mats, np.float32, device)
        return cls._build(template, [(buffer, names, dim)])

    def _alive(self):
        for block in self._blocks:
            block.alive()

    def to_host(self):
        """The :class:`FeaturesCollection` the host call returns, bit for bit (one download per block; the
        matrices are row-block views of it, as there)"""
        self._alive()
        out = {}
        for block in self._blocks:
            rows = int(block.foff[-1])
            host = _backend.result_array((rows, block.dim), np.float32)
            if host.size:
                block.buffer.download(host)
            for name, a, b in zip(block.names, block.foff[:-1].tolist(), block.foff[1:].tolist()):
                feats = self[name]
                data = host[a:b] if b > a or feats._host_shape[1] == block.dim else \
                    np.zeros(feats._host_shape, dtype=np.float32)
                out[name] = Features._of_batch(data, *feats._shared)
        return FeaturesCollection((name, out[name]) for name in self)

    def padded(self, dtype='float32', left=0, right=0, subsample=1, offset=0, pad_value=0.0, max_frames=None):
        """The collection as ONE padded tensor in HBM, made by one kernel (snf_collate_padded):

            data[b, j, (k + left) * dim + d] = rows_b[clamp(offset + j * subsample + k, 0, T_b - 1), d]   j < n_b
            data[b, j, :] = pad_value                                                                        j >= n_b
            lengths[b] = n_b = number of frames offset, offset + subsample, ... below T_b

        k in [-left, right] (Kaldi's splice-feats over the frames subsample-feats keeps), cast to `dtype`
        ('float32', 'float16', 'bfloat16': to nearest even).  T is `max_frames`, or the largest n_b.  Returns a
        :class:`DeviceBatch`.  ValueError for utterances of different `ndims`, for a collection in several blocks
        (utterances of several sample rates), and for invalid arguments."""
        self._alive()
        if len({block.dim for block in self._blocks}) > 1:
            raise ValueError('utterances have different ndims: {}'.format(
                sorted({block.dim for block in self._blocks})))
        if len(self._blocks) > 1:
            raise ValueError('the utterances lie in {} device blocks (one per sample rate): a padded batch is '
                             'made of one block'.format(len(self._blocks)))
        if dtype not in _backend.COLLATE_TYPES:
            raise ValueError('invalid dtype "{}", choose in "{}"'.format(dtype, ', '.join(_backend.COLLATE_TYPES)))
        left, right, subsample, offset = int(left), int(right), int(subsample), int(offset)
        if left < 0 or right < 0:
            raise ValueError('left and right contexts must not be negative')
        if subsample < 1 or not 0 <= offset < subsample:
            raise ValueError('subsample must be at least 1 and offset in [0, subsample)')
        names = self._blocks[0].names if self._blocks else []
        dim = self._blocks[0].dim if self._blocks else 0
        foff = self._blocks[0].foff if self._blocks else np.zeros(1, dtype=np.int64)
        frames = np.diff(foff)
        counts = np.where(frames <= offset, 0, (frames - offset + subsample - 1) // subsample)
        longest = int(counts.max()) if counts.size else 0
        t_max = longest if max_frames is None else int(max_frames)
        if t_max < longest:
            raise ValueError(f'max_frames is {t_max} but an utterance keeps {longest} frames')
        width = dim * (left + 1 + right)
        device = self._blocks[0].buffer.device if self._blocks else None
        itemsize = _dlpack.ITEMSIZE[dtype]
        data = _backend.DeviceBuffer(max(len(names) * t_max * width * itemsize, 16), device)
        lengths = _backend.DeviceBuffer(max(4 * len(names), 16), device)
        try:
            if names:
                _backend.collate_padded(self._blocks[0].buffer.ptr, dim, foff, dtype, left, right, subsample, offset,
                                        pad_value, t_max, data.ptr, lengths.ptr, device=device)
        except BaseException:
            data.free()
            lengths.free()
            raise
        shape = (len(names), t_max, width)
        return DeviceBatch(DeviceArray(_Block(data, names, width, None), 0, shape, dtype),
                           DeviceArray(_Block(lengths, names, 1, None), 0, (len(names),), 'int32'),
                           names, {name: self[name]._shared[0] for name in names}, subsample, offset)

    def release(self):
        """Gives the blocks back to the device pool (after waiting for the device).  Afterwards every export,
        `padded` and `to_host` raise.  A block that a DLPack consumer still holds goes back when that consumer
        lets go of it."""
        for block in self._blocks:
            block.buffer = None
