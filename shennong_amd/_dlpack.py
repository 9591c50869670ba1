"""DLPack export of a buffer the package owns, built on ctypes (no compiled extension, no framework).

The unversioned protocol: a ``DLManagedTensor`` in a PyCapsule named ``dltensor``.  A consumer
(``torch.from_dlpack``, ``np.from_dlpack``...) renames the capsule to ``used_dltensor`` and calls the struct's
deleter when its own tensor dies; a capsule nobody consumed calls the deleter when it is collected.  Either
way the deleter runs once and drops ONE reference on `owner`, the Python object that keeps the memory alive.

`data` is the address of the first element itself and `byte_offset` is 0 (torch ignores the alignment rule
that byte_offset exists for, and a row block of an odd `dim` starts at a 4-byte aligned address anyway);
strides are given, in elements.  The device type is an argument: kDLROCM for HBM, kDLCPU for a host buffer -
which is how this module is tested without a GPU.
"""

import ctypes as C
import threading

kDLCPU = 1
kDLROCM = 10

# (code, bits) of DLDataType; lanes is always 1
DTYPES = {'float32': (2, 32), 'float16': (2, 16), 'bfloat16': (4, 16), 'int32': (0, 32)}
ITEMSIZE = {'float32': 4, 'float16': 2, 'bfloat16': 2, 'int32': 4}


class DLDevice(C.Structure):
    _fields_ = [('device_type', C.c_int32), ('device_id', C.c_int32)]


class DLDataType(C.Structure):
    _fields_ = [('code', C.c_uint8), ('bits', C.c_uint8), ('lanes', C.c_uint16)]


class DLTensor(C.Structure):
    _fields_ = [('data', C.c_void_p), ('device', DLDevice), ('ndim', C.c_int32), ('dtype', DLDataType),
                ('shape', C.POINTER(C.c_int64)), ('strides', C.POINTER(C.c_int64)), ('byte_offset', C.c_uint64)]


class DLManagedTensor(C.Structure):
    pass


_DELETER = C.CFUNCTYPE(None, C.POINTER(DLManagedTensor))
DLManagedTensor._fields_ = [('dl_tensor', DLTensor), ('manager_ctx', C.c_void_p), ('deleter', _DELETER)]

_NAME = b'dltensor'
_USED = b'used_dltensor'

# address of a live DLManagedTensor -> (the struct, its shape and strides arrays, owner): what the struct
# points to, kept alive until its deleter runs
_LIVE = {}
_LOCK = threading.Lock()
STATS = {'exported': 0, 'deleted': 0}   # (tests: every export is deleted exactly once)


@_DELETER
def _delete(managed):
    address = C.addressof(managed.contents)
    with _LOCK:
        entry = _LIVE.pop(address, None)
        if entry is not None:
            STATS['deleted'] += 1
    del entry   # (the owner's reference goes here, outside the lock: its __del__ may export or delete)


_capsule_destructor_type = C.CFUNCTYPE(None, C.c_void_p)
_api = C.pythonapi
_new = _api.PyCapsule_New
_new.restype = C.py_object
_new.argtypes = [C.c_void_p, C.c_char_p, _capsule_destructor_type]
# (the capsule is passed as a bare address: inside its destructor it has no references left to count)
_is_valid = _api.PyCapsule_IsValid
_is_valid.restype = C.c_int
_is_valid.argtypes = [C.c_void_p, C.c_char_p]
_get_pointer = _api.PyCapsule_GetPointer
_get_pointer.restype = C.c_void_p
_get_pointer.argtypes = [C.c_void_p, C.c_char_p]


@_capsule_destructor_type
def _capsule_destructor(capsule):
    # a consumed capsule was renamed: its consumer calls the deleter
    if _is_valid(capsule, _NAME):
        managed = C.cast(_get_pointer(capsule, _NAME), C.POINTER(DLManagedTensor))
        managed.contents.deleter(managed)


def export(address, shape, dtype, device_type, device_id, owner, strides=None):
    """A ``dltensor`` capsule over `shape` elements of `dtype` (a key of DTYPES) at `address`, row-major unless
    `strides` (in elements) says otherwise.  `owner` stays referenced until the deleter has run."""
    if dtype not in DTYPES:
        raise ValueError(f'no DLPack data type for "{dtype}", choose in {sorted(DTYPES)}')
    shape = [int(x) for x in shape]
    if strides is None:
        strides, step = [], 1
        for extent in reversed(shape):
            strides.insert(0, step)
            step *= max(extent, 1)
    strides = [int(x) for x in strides]
    if len(strides) != len(shape):
        raise ValueError('one stride per dimension is required')
    ndim = len(shape)
    c_shape = (C.c_int64 * max(ndim, 1))(*shape)
    c_strides = (C.c_int64 * max(ndim, 1))(*strides)
    managed = DLManagedTensor()
    tensor = managed.dl_tensor
    tensor.data = C.c_void_p(int(address))
    tensor.device = DLDevice(int(device_type), int(device_id))
    tensor.ndim = ndim
    code, bits = DTYPES[dtype]
    tensor.dtype = DLDataType(code, bits, 1)
    tensor.shape = C.cast(c_shape, C.POINTER(C.c_int64))
    tensor.strides = C.cast(c_strides, C.POINTER(C.c_int64))
    tensor.byte_offset = 0
    managed.manager_ctx = None
    managed.deleter = _delete
    key = C.addressof(managed)
    with _LOCK:
        _LIVE[key] = (managed, c_shape, c_strides, owner)
        STATS['exported'] += 1
    try:
        return _new(key, _NAME, _capsule_destructor)
    except BaseException:
        with _LOCK:
            _LIVE.pop(key, None)
            STATS['exported'] -= 1
        raise


def managed_tensor(capsule):
    """The DLManagedTensor of a capsule that was not consumed (tests and diagnostics: read, do not delete)"""
    if not _is_valid(id(capsule), _NAME):
        raise ValueError('not a live "dltensor" capsule')
    address = _get_pointer(id(capsule), _NAME)
    return C.cast(address, C.POINTER(DLManagedTensor)).contents


def live():
    """Exports whose deleter has not run yet"""
    with _LOCK:
        return len(_LIVE)
