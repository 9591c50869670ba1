"""Linear VTLN: the model, fMLLR statistics and their device computation.

- :class:`LinearVtln` restates [KALDI-UPSTREAM] transform/lvtln.{h,cc} ``LinearVtln``: one float32 matrix
  ``A_c`` [D, D] and one warp per class, a default class, and ``logdets[c] = log|det A_c|`` (float64 here).
- :class:`FmllrStats` holds Kaldi's ``AffineXformStats``: ``beta``, ``K`` [D, D+1], ``G`` [D, D+1, D+1]
  (float64).
- The device functions wrap the ``snf_fmllr_accumulate`` / ``snf_vtln_gram`` / ``snf_vtln_gram_rows`` /
  ``snf_lvtln_select`` / ``snf_affine_apply_segments`` kernels (``csrc/kernels_vtln.hip``, whose header states the math).

Binary layout (Kaldi binary mode, the ``\\0B`` marker first when a whole file), as read from upstream
``LinearVtln::Write`` / ``Read`` without a Kaldi build to confirm it::

    <LinearVtln> <int32 num_classes>
    per class: <Transform> <float matrix A_c> <Warp> <float warp>
    <DefaultClass> <int32 default_class> </LinearVtln>

``logdets`` are recomputed on read.  A legacy file that ends right after the classes (``</LinearVtln>``
with no ``<DefaultClass>``) gets ``default_class = (num_classes + 1) // 2``.

Readings followed (``LinearVtln::ComputeTransform``):

- the aux function of a class is ``FmllrAuxFuncDiagGmm(W, stats) + (logdet_scale - 1) * beta * logdets[c]``
  with W the composed transform, so the log-determinant of ``A_c`` enters as
  ``logdet_scale * beta * logdets[c]`` (at 'none' and 'offset' that is the whole log-determinant term);
- the objectives are float64 on the float64 composed transform (Kaldi rounds it to float first).
"""

import ctypes as C
import io
import struct

import numpy as np

from shennong_amd import _backend
from shennong_amd.serializers import KaldiBinaryReader, write_kaldi_object, write_kaldi_token


NORM_TYPES = {'none': 0, 'offset': 1, 'diag': 2}
# segments per snf_fmllr_accumulate call: the statistics buffer stays below this many bytes
STATS_BYTES_BOUND = 256 << 20


def _logdet(A):
    sign, value = np.linalg.slogdet(np.asarray(A, dtype=np.float64))
    return float(value) if sign != 0 else float('-inf')


class LinearVtln:
    """[KALDI-UPSTREAM] transform/lvtln.h LinearVtln(dim, num_classes, default_class)"""

    def __init__(self, dim, num_classes, default_class):
        dim, num_classes, default_class = int(dim), int(num_classes), int(default_class)
        if num_classes < 0 or (num_classes and not 0 <= default_class < num_classes):
            raise ValueError(f'default class {default_class} out of range for {num_classes} classes')
        self.A = [np.eye(dim, dtype=np.float32) for _ in range(num_classes)]
        self.warps = [1.0] * num_classes
        self.logdets = [_logdet(a) for a in self.A]
        self.default_class = default_class
        self._dim = dim

    def dim(self):
        return self._dim

    def num_classes(self):
        return len(self.A)

    def set_transform(self, c, A):
        A = np.asarray(A, dtype=np.float32)
        if A.shape != (self._dim, self._dim):
            raise ValueError(f'transform must be {self._dim} x {self._dim}, it is {A.shape}')
        self.A[c] = A.copy()
        self.logdets[c] = _logdet(self.A[c])

    def get_transform(self, c):
        return self.A[c].copy()

    def set_warp(self, c, w):
        self.warps[c] = float(np.float32(w))

    def get_warp(self, c):
        return self.warps[c]

    def write(self, stream):
        """Kaldi binary form (the module's layout), without the ``\\0B`` marker"""
        write_kaldi_token(stream, '<LinearVtln>')
        stream.write(b'\4' + struct.pack('<i', self.num_classes()))
        for A, w in zip(self.A, self.warps):
            write_kaldi_token(stream, '<Transform>')
            write_kaldi_object(stream, A)
            write_kaldi_token(stream, '<Warp>')
            stream.write(b'\4' + struct.pack('<f', w))
        write_kaldi_token(stream, '<DefaultClass>')
        stream.write(b'\4' + struct.pack('<i', self.default_class))
        write_kaldi_token(stream, '</LinearVtln>')

    def read(self, stream):
        """Reads the rest of `stream` (binary, after the ``\\0B`` marker)"""
        blob = stream.read()
        reader = KaldiBinaryReader(blob, 0)
        reader.expect('<LinearVtln>')
        num_classes = reader._int()
        A, warps = [], []
        for _ in range(num_classes):
            reader.expect('<Transform>')
            A.append(np.array(reader.object(), dtype=np.float32))
            reader.expect('<Warp>')
            if blob[reader.pos:reader.pos + 1] != b'\4':
                raise ValueError('bad float size marker in Kaldi binary object')
            warps.append(float(struct.unpack('<f', blob[reader.pos + 1:reader.pos + 5])[0]))
            reader.pos += 5
        tok = reader.token()
        if tok == '<DefaultClass>':
            default_class = reader._int()
            reader.expect('</LinearVtln>')
        elif tok == '</LinearVtln>':
            default_class = (num_classes + 1) // 2
        else:
            raise ValueError(f'expected token <DefaultClass> or </LinearVtln>, got {tok}')
        self._dim = A[0].shape[0] if A else 0
        self.A, self.warps = A, warps
        self.logdets = [_logdet(a) for a in A]
        self.default_class = default_class
        return self

    def to_bytes(self):
        stream = io.BytesIO()
        stream.write(b'\0B')
        self.write(stream)
        return stream.getvalue()

    @classmethod
    def from_bytes(cls, blob):
        if blob[:2] != b'\0B':
            raise ValueError('not a binary Kaldi file')
        return cls(0, 0, 0).read(io.BytesIO(blob[2:]))


class FmllrStats:
    """[KALDI-UPSTREAM] transform/fmllr-diag-gmm.h AffineXformStats: beta, K [D, D+1], G [D, D+1, D+1]"""

    def __init__(self, dim):
        self.beta = 0.0
        self.K = np.zeros((dim, dim + 1), dtype=np.float64)
        self.G = np.zeros((dim, dim + 1, dim + 1), dtype=np.float64)

    def dim(self):
        return self.K.shape[0]

    @classmethod
    def from_device_layout(cls, S):
        """From one segment's [U, D+1] rows of snf_fmllr_accumulate"""
        S = np.asarray(S, dtype=np.float64)
        V = S.shape[1]
        D = V - 1
        st = cls(D)
        st.G = S[:D * V].reshape(D, V, V).copy()
        st.K = S[D * V:D * V + D].copy()
        st.beta = float(S[D * V + D, D])
        return st


# ---- device side -----------------------------------------------------------------------------------------
def _vp(x):
    return C.c_void_p(x.ptr) if x is not None else None


def stats_rows(dim):
    return dim * (dim + 1) + dim + 1


def segments_per_call(dim, bound=STATS_BYTES_BOUND):
    return max(1, bound // (8 * stats_rows(dim) * (dim + 1)))


def fmllr_accumulate(block, dgmm, dsel, dpost, num_gselect, offsets, first=0, last=None):
    """Statistics of segments ``first .. last`` (frames ``offsets[s] .. offsets[s+1]`` of `block`): a
    DeviceBuffer [S, U, D+1] float64 (see FmllrStats.from_device_layout)"""
    offsets = np.asarray(offsets, dtype=np.int64)
    last = len(offsets) - 1 if last is None else last
    D = block.dim
    a, b = int(offsets[first]), int(offsets[last])
    rel = np.ascontiguousarray(offsets[first:last + 1] - a)
    S = last - first
    out = _backend.DeviceBuffer(8 * max(1, S * stats_rows(D) * (D + 1)), block.device)
    _backend.check(_backend.lib().snf_fmllr_accumulate(
        block.device, C.c_void_p(block.frames.ptr + 4 * a * D), b - a, D,
        C.c_void_p(dsel.ptr + 4 * a * num_gselect), C.c_void_p(dpost.ptr + 4 * a * num_gselect), int(num_gselect),
        C.c_void_p(dgmm.means_invvars.ptr), C.c_void_p(dgmm.inv_vars.ptr), dgmm.num_gauss,
        rel.ctypes.data_as(C.c_void_p), S, C.c_void_p(out.ptr), None))
    return out


def download_stats(buf, S, dim):
    return buf.download(np.empty((S, stats_rows(dim), dim + 1), dtype=np.float64))


class DeviceLvtln:
    """The classes of a :class:`LinearVtln` in HBM: A [C, D, D] and logdets [C], float64 (uploaded once)"""

    def __init__(self, lvtln, device=None):
        self.dim, self.num_classes, self.default_class = lvtln.dim(), lvtln.num_classes(), lvtln.default_class
        A = np.stack([np.asarray(a, np.float64) for a in lvtln.A]) if self.num_classes else np.zeros((1, 1, 1))
        self.A = _backend.DeviceBuffer(A.nbytes, device)
        self.A.upload(A)
        ld = np.asarray(lvtln.logdets if self.num_classes else [0.0], np.float64)
        self.logdets = _backend.DeviceBuffer(ld.nbytes, device)
        self.logdets.upload(ld)
        self.device = self.A.device

    def select(self, stats_buf, S, norm_type, logdet_scale):
        """(objf [S, C] float64, class [S] int32, impr [S], count [S] float64, transforms DeviceBuffer
        [S, D, D+1] float32)"""
        D, Cn = self.dim, self.num_classes
        objf = _backend.DeviceBuffer(8 * max(1, S * Cn), self.device)
        cls = _backend.DeviceBuffer(4 * max(1, S), self.device)
        impr = _backend.DeviceBuffer(8 * max(1, S), self.device)
        count = _backend.DeviceBuffer(8 * max(1, S), self.device)
        trans = _backend.DeviceBuffer(4 * max(1, S * D * (D + 1)), self.device)
        _backend.check(_backend.lib().snf_lvtln_select(
            self.device, _vp(stats_buf), S, D, _vp(self.A), _vp(self.logdets), Cn, NORM_TYPES[norm_type],
            float(logdet_scale), self.default_class, _vp(objf), _vp(cls), _vp(impr), _vp(count), _vp(trans), None))
        return (objf.download(np.empty((S, Cn), np.float64)), cls.download(np.empty(S, np.int32)),
                impr.download(np.empty(S, np.float64)), count.download(np.empty(S, np.float64)), trans)


def vtln_gram(dx, dy, nframes, dim, dweights=None, device=None):
    """sum_f w_f z_f z_f^T, z = [x | 1 | y], float64 [2D+1, 2D+1] (x, y: DeviceBuffers [F, D] float32)"""
    V = 2 * dim + 1
    out = _backend.DeviceBuffer(8 * V * V, device)
    _backend.check(_backend.lib().snf_vtln_gram(
        out.device, _vp(dx), _vp(dy), _vp(dweights), int(nframes), int(dim), _vp(out), None))
    return out.download(np.empty((V, V), np.float64))


def upload_row_list(block, row, device=None):
    """The (block, row) list of :func:`vtln_gram_rows` in HBM: (DeviceBuffer int32 [F], DeviceBuffer int64 [F])"""
    block = np.ascontiguousarray(block, dtype=np.int32)
    row = np.ascontiguousarray(row, dtype=np.int64)
    if block.shape != row.shape or block.ndim != 1:
        raise ValueError('block and row lists must be 1-D and of the same length')
    dblock = _backend.DeviceBuffer(block.nbytes, device)
    drow = _backend.DeviceBuffer(row.nbytes, dblock.device)
    if block.size:
        dblock.upload(block)
        drow.upload(row)
    return dblock, drow


def vtln_gram_rows(x_blocks, y_blocks, dblock, drow, nframes, dim, dweights=None):
    """:func:`vtln_gram` over rows gathered on the device: frame f is row ``row[f]`` of block ``block[f]`` of
    `x_blocks` and of `y_blocks` (lists of DeviceBuffers [rows, D] float32, same shapes in both lists;
    ``dblock`` / ``drow`` from :func:`upload_row_list`, every pair in range - the caller checks it).  Bit for
    bit what vtln_gram gives on the rows gathered on the host, in the same order."""
    if len(x_blocks) != len(y_blocks) or not x_blocks:
        raise ValueError('x and y need the same, non-zero number of blocks')
    V = 2 * dim + 1
    device = x_blocks[0].device
    out = _backend.DeviceBuffer(8 * V * V, device)
    pointers = []
    for blocks in (x_blocks, y_blocks):
        table = np.asarray([b.ptr for b in blocks], dtype=np.uint64)
        pointers.append(_backend.DeviceBuffer(table.nbytes, device))
        pointers[-1].upload(table)
    _backend.check(_backend.lib().snf_vtln_gram_rows(
        device, _vp(pointers[0]), _vp(pointers[1]), _vp(dblock), _vp(drow), _vp(dweights), int(nframes),
        int(dim), _vp(out), None))
    for table in pointers:
        table.free(synced=True)
    return out.download(np.empty((V, V), np.float64))


def affine_apply_segments(block, offsets, dtrans, out=None):
    """y_f = W_s x_f + b_s on the device: a DeviceBuffer [F, D] float32 (`dtrans`: [S, D, D+1] float32)"""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    D = block.dim
    out = out if out is not None else _backend.DeviceBuffer(4 * max(1, block.nframes * D), block.device)
    _backend.check(_backend.lib().snf_affine_apply_segments(
        block.device, C.c_void_p(block.frames.ptr), block.nframes, D, offsets.ctypes.data_as(C.c_void_p),
        len(offsets) - 1, _vp(dtrans), C.c_void_p(out.ptr), None))
    return out
