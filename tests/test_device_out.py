"""Device-resident results, the parts that need no GPU: the host-only entry point and the argument checks of the
collate call, the DLPack export over a host buffer (kDLCPU), the checker's roundings against torch's, and the
HIP runtime probe."""

import ctypes as C
import gc
import os
import weakref

import numpy as np
import pytest

import collate_np
from conftest import ROOT
from shennong_amd import _abi, _backend, _dlpack, device


def test_num_out_matches_formula():
    for frames in (0, 1, 2, 3, 7):
        for subsample in (1, 2, 3):
            for offset in range(subsample):
                want = len(range(offset, frames, subsample))
                assert collate_np.num_out(frames, subsample, offset) == want
                assert _backend.collate_num_out(frames, subsample, offset) == want, (frames, subsample, offset)
    for bad in ((-1, 1, 0), (3, 0, 0), (3, 2, 2), (3, 2, -1)):
        with pytest.raises(ValueError):
            _backend.collate_num_out(*bad)


def _refused(foff=(0, 3, 10), dim=13, dtype='float32', left=0, right=0, subsample=1, offset=0, t_max=7,
             d_out=4096, d_lengths=8192, d_in=16384):
    """The pointers are made up: a refusal comes back before any of them is used"""
    with pytest.raises(ValueError) as err:
        _backend.collate_padded(d_in, dim, np.asarray(foff, dtype=np.int64), dtype, left, right, subsample, offset,
                                0.0, t_max, d_out, d_lengths, device=0)
    return str(err.value)


def test_collate_refusals_before_any_device_use():
    assert 't_max is 6' in _refused(t_max=6)
    assert 't_max is 3' in _refused(t_max=3, subsample=2)          # (ceil(7 / 2) = 4 frames are kept)
    assert 'subsample' in _refused(subsample=0)
    assert 'subsample' in _refused(subsample=2, offset=2)
    assert 'subsample' in _refused(offset=-1)
    assert 'context' in _refused(left=-1)
    assert 'context' in _refused(right=-1)
    assert 'dim' in _refused(dim=0)
    assert 'decrease' in _refused(foff=(0, 5, 3))
    assert 'negative' in _refused(foff=(-1, 5, 7))
    assert '16-byte aligned' in _refused(d_out=4100)
    assert 'null buffer' in _refused(d_out=0)
    # 2 x 2^20 x 1024 elements = 2^31: one more than 32-bit indices reach
    assert '2^31' in _refused(foff=(0, 1, 2), dim=1024, t_max=1 << 20)
    assert '2^31' in _refused(foff=(0, 1, 2), dim=1 << 16, left=1 << 15, right=0, t_max=1)
    with pytest.raises(ValueError):
        _backend.collate_padded(16384, 13, np.array([0, 3], dtype=np.int64), 'float64', 0, 0, 1, 0, 0.0, 3, 4096, 8192)
    lib = _backend.lib()
    rc = lib.snf_collate_padded(0, 16384, 13, np.array([0, 3], dtype=np.int64).ctypes.data_as(
        C.POINTER(C.c_int64)), 1, 0, 0, 1, 0, 3, 0.0, 3, 4096, 8192, None)
    assert rc == _abi.SNF_E_INVALID and b'out_type' in lib.snf_last_error()


def test_collate_without_device_fails_loudly():
    if _backend.device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(RuntimeError) as err:
        _backend.collate_padded(16384, 13, np.array([0, 3], dtype=np.int64), 'float32', 0, 0, 1, 0, 0.0, 3, 4096, 8192,
                                device=0)
    assert 'no HIP device' in str(err.value)


def test_exports_are_declared():
    header = open(os.path.join(ROOT, 'include', 'shennong_amd.h')).read()
    for name in ('snf_collate_num_out', 'snf_collate_padded'):
        assert name + '(' in header and name in _backend.EXPORTS and hasattr(_backend.lib(), name)
    assert 'no reference call behind it' in header and 'splice-feats' in header and 'subsample-feats' in header


# ---- DLPack over a host buffer ----------------------------------------------------------------------------------
class _Owner:
    """Keeps a numpy array alive; exports it as kDLCPU"""
    def __init__(self, array, dtype=None):
        self.array = array
        self.dtype = dtype or array.dtype.name

    def __dlpack__(self, stream=None):
        return _dlpack.export(self.array.ctypes.data, self.array.shape, self.dtype, _dlpack.kDLCPU, 0, owner=self)

    def __dlpack_device__(self):
        return (_dlpack.kDLCPU, 0)


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
def test_dlpack_numpy_zero_copy_and_owner_lifetime(dtype):
    source = np.arange(3 * 7, dtype=dtype).reshape(3, 7) / 3
    owner = _Owner(source)
    alive = weakref.ref(owner)
    before = dict(_dlpack.STATS)
    got = np.from_dlpack(owner)
    assert got.dtype == dtype and got.shape == (3, 7) and np.array_equal(got, source)
    assert got.ctypes.data == source.ctypes.data                   # zero copy
    assert _dlpack.STATS['exported'] == before['exported'] + 1
    del owner, source
    gc.collect()
    assert alive() is not None and _dlpack.STATS['deleted'] == before['deleted']   # the consumer keeps it alive
    assert float(got[2, 6]) == float(dtype(20) / dtype(3))
    del got
    gc.collect()
    assert alive() is None                                        # one reference dropped, the last one
    assert _dlpack.STATS['deleted'] == before['deleted'] + 1     # ... by one call of the deleter


def test_dlpack_unconsumed_capsule_deletes_once():
    owner = _Owner(np.zeros((2, 2), dtype=np.float32))
    alive = weakref.ref(owner)
    before = dict(_dlpack.STATS)
    live = _dlpack.live()
    capsule = owner.__dlpack__()
    assert _dlpack.live() == live + 1
    del owner
    gc.collect()
    assert alive() is not None
    del capsule
    gc.collect()
    assert alive() is None and _dlpack.live() == live
    assert _dlpack.STATS['deleted'] == before['deleted'] + 1


@pytest.mark.parametrize('dtype, code, bits', [('bfloat16', 4, 16), ('int32', 0, 32), ('float16', 2, 16),
                                               ('float32', 2, 32)])
def test_dlpack_struct_fields(dtype, code, bits):
    raw = np.zeros((5, 4, 6), dtype=np.uint16 if bits == 16 else np.int32)
    owner = _Owner(raw[1:, :, ::1], dtype=dtype)
    capsule = _dlpack.export(owner.array.ctypes.data, owner.array.shape, dtype, _dlpack.kDLROCM, 3, owner=owner)
    managed = _dlpack.managed_tensor(capsule)
    tensor = managed.dl_tensor
    assert tensor.data == raw.ctypes.data + raw.strides[0] and tensor.byte_offset == 0
    assert (tensor.device.device_type, tensor.device.device_id) == (10, 3)
    assert (tensor.dtype.code, tensor.dtype.bits, tensor.dtype.lanes) == (code, bits, 1)
    assert tensor.ndim == 3
    assert [tensor.shape[i] for i in range(3)] == [4, 4, 6]
    assert [tensor.strides[i] for i in range(3)] == [24, 6, 1]   # in elements
    assert not managed.manager_ctx and managed.deleter
    with pytest.raises(ValueError):
        _dlpack.export(0, (1,), 'float64', _dlpack.kDLCPU, 0, owner=None)
    capsule2 = _dlpack.export(raw.ctypes.data, (5, 4), dtype, _dlpack.kDLCPU, 0, owner=owner, strides=(24, 6))
    other = _dlpack.managed_tensor(capsule2).dl_tensor
    assert [other.strides[i] for i in range(2)] == [24, 6] and other.device.device_type == 1


# ---- the checker's roundings ------------------------------------------------------------------------------------
def _rounding_values():
    rng = np.random.default_rng(5)
    values = collate_np.special_rows(np.zeros(64, dtype=np.float32))
    return np.concatenate([values, -values, rng.standard_normal(4096).astype(np.float32) * 37,
                           rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)])


def test_checker_bfloat16_rounding_is_torchs():
    torch = pytest.importorskip('torch')
    x = _rounding_values()
    want = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = collate_np.round_bf16(x)
    assert collate_np.same_bits(got, want, 'bfloat16')
    assert np.isnan(x).sum() > 2 and (np.abs(x[np.isfinite(x)]) < 1.2e-38).sum() > 2   # NaN and subnormals are there
    # the ties: 1 + 2^-8 lies half way between 1 and 1 + 2^-7 and goes to the even one
    assert collate_np.round_bf16(np.float32([1.00390625, 1.01171875, -1.00390625])).tolist() == [0x3F80, 0x3F82, 0xBF80]


def test_checker_float16_rounding_is_ieee():
    torch = pytest.importorskip('torch')
    x = _rounding_values()
    want = torch.tensor(x).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    assert collate_np.same_bits(collate_np.round_f16(x), want, 'float16')
    assert collate_np.round_f16(np.float32([65519.9, 65520.0, -70000.0])).tolist() == [0x7BFF, 0x7C00, 0xFC00]


def test_checker_collate_small_case():
    rows = np.arange(5 * 2, dtype=np.float32).reshape(5, 2)   # utterances of 2 and 3 frames
    out, lengths = collate_np.collate(rows, [0, 2, 5], 'float32', 1, 1, 2, 0, -1.0, 3)
    out = out.view(np.float32)
    assert lengths.tolist() == [1, 2]
    assert out[0, 0].tolist() == [0, 1, 0, 1, 2, 3] and (out[0, 1:] == -1).all()
    assert out[1, 0].tolist() == [4, 5, 4, 5, 6, 7] and out[1, 1].tolist() == [6, 7, 8, 9, 8, 9]
    assert (out[1, 2] == -1).all()


# ---- runtime probe, entry points --------------------------------------------------------------------------------
def test_shares_hip_runtime_with_torch_needs_no_device():
    shared, paths = device.shares_hip_runtime_with_torch()
    assert isinstance(shared, bool) and isinstance(paths, list)
    assert all(os.path.basename(p).startswith('libamdhip64') and os.path.isabs(p) for p in paths)
    assert len(paths) >= 1 and shared == (len(paths) == 1)
    assert paths == device.mapped_hip_runtimes()


def test_process_all_device_names_the_pipeline_for_other_processors():
    from shennong_amd.processor.base import FeaturesProcessor
    from shennong_amd.utterances import Utterances

    class Other(FeaturesProcessor):
        name, ndims = 'other', 1

        def process(self, signal):   # pragma: nocover
            raise AssertionError('not reached')

    with pytest.raises(NotImplementedError) as err:
        Other().process_all_device(Utterances([('a', os.path.join(ROOT, 'tests', 'golden', 'test.wav'))]))
    assert 'extract_features_device' in str(err.value)


def test_extract_features_device_refuses_a_corpus_beyond_one_batch(monkeypatch):
    from shennong_amd import pipeline
    from shennong_amd.utterances import Utterances
    monkeypatch.setattr(pipeline, '_too_large_for_one_batch', lambda *args, **kwargs: True)
    utts = Utterances([('a', os.path.join(ROOT, 'tests', 'golden', 'test.wav'), 'spk')])
    with pytest.raises(ValueError) as err:
        pipeline.extract_features_device(pipeline.get_default_config('mfcc'), utts)
    assert 'extract_features_streamed' in str(err.value)
