"""Device-resident results on the GPU: the collate kernel against its numpy statement (tests/collate_np.py), bit
for bit; the device entry points against the host calls they shadow, bit for bit; the DLPack export read back
through ctypes; release; and the torch hand-over where torch shares the library's HIP runtime."""

import ctypes as C
import gc

import numpy as np
import pytest

import collate_np
from shennong_amd import Audio, _dlpack, device, pipeline, synth
from shennong_amd.processor import (EnergyProcessor, FilterbankProcessor, KaldiPitchProcessor, MfccProcessor,
                                    PlpProcessor, SpectrogramProcessor)
from shennong_amd.utils import dict_equal
from shennong_amd.utterances import Utterances

pytestmark = pytest.mark.gpu

FRAMES = [0, 1, 2, 7, 19]   # utterance starts are then unaligned for every odd dim
ITEM = {'float32': (4, np.uint32), 'float16': (2, np.uint16), 'bfloat16': (2, np.uint16)}


def _poisoned(backend, nbytes):
    """A device buffer that comes out of the pool, hence full of NaN bit patterns (the `gpu` fixture)"""
    backend.DeviceBuffer(nbytes).free()
    block = backend.DeviceBuffer(nbytes)
    probe = np.zeros(min(nbytes, 16), dtype=np.uint8)
    block.download(probe)
    assert (probe == 0xFF).all()
    return block


def _rows(dim, frames, seed):
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((sum(frames), dim)) * 9).astype(np.float32)
    return collate_np.special_rows(rows)


# (dim, frames, dtype, left, right, subsample, offset, pad_value, whole pad rows): together they cover every dim,
# subsample 1 / 2 / 3 with an offset beyond the short utterances, the three contexts (5 + 3 is wider than every
# utterance but one: both clamps act on one frame), the three types, the three pad values, max_frames None and
# larger, B = 1, and totals that are no multiple of 4 (float32) or 8 (the narrow types): a narrow last chunk
CASES = [
    (1, FRAMES, 'float32', 0, 0, 1, 0, 0.0, 0),            # 95 elements: narrow last chunk of 3 floats
    (13, FRAMES, 'bfloat16', 0, 0, 1, 0, 0.0, 0),          # 1235 elements: narrow last chunk of 3 halves
    (13, FRAMES, 'bfloat16', 1, 1, 2, 1, -1.5, 3),
    (40, FRAMES, 'float16', 5, 3, 3, 2, float('nan'), 0),  # offset 2 is beyond the utterances of 0, 1, 2 frames
    (40, FRAMES, 'float32', 1, 1, 2, 0, -1.5, 0),
    (257, FRAMES, 'float32', 5, 3, 1, 0, float('nan'), 2),
    (257, FRAMES, 'bfloat16', 0, 0, 3, 0, 0.0, 0),
    (257, FRAMES, 'float16', 1, 1, 1, 0, -1.5, 1),
    (13, [7], 'float16', 1, 1, 1, 0, -1.5, 0),             # B = 1; 273 elements
    (13, [0, 0], 'float32', 0, 0, 1, 0, 0.0, 0),           # nothing but lengths (t_max = 0)
]


@pytest.mark.parametrize('dim, frames, dtype, left, right, subsample, offset, pad_value, extra', CASES)
def test_collate_matches_numpy_statement(gpu, dim, frames, dtype, left, right, subsample, offset, pad_value, extra):
    rows = _rows(dim, frames, seed=dim + left + subsample)
    foff = np.zeros(len(frames) + 1, dtype=np.int64)
    np.cumsum(frames, out=foff[1:])
    longest = max(collate_np.num_out(t, subsample, offset) for t in frames)
    t_max = longest + extra
    want, want_lengths = collate_np.collate(rows, foff, dtype, left, right, subsample, offset, pad_value, t_max)
    itemsize, bits = ITEM[dtype]
    d_in = gpu.DeviceBuffer(max(rows.nbytes, 16))
    if rows.size:
        d_in.upload(rows)
    d_out = _poisoned(gpu, max(want.size * itemsize, 16))
    d_lengths = _poisoned(gpu, 4 * len(frames))
    gpu.collate_padded(d_in.ptr, dim, foff, dtype, left, right, subsample, offset, pad_value, t_max, d_out.ptr,
                       d_lengths.ptr)
    got = d_out.download(np.zeros(want.shape, dtype=bits)) if want.size else np.zeros(want.shape, dtype=bits)
    got_lengths = d_lengths.download(np.zeros(len(frames), dtype=np.int32))
    for block in (d_in, d_out, d_lengths):
        block.free()
    assert np.array_equal(got_lengths, want_lengths)
    assert collate_np.same_bits(got, want, dtype), (
        'first differences at', np.argwhere(got != want)[:5].tolist())
    if np.isnan(pad_value) and extra and dtype == 'float32':
        assert np.isnan(got.view(np.float32)[0, -1]).all()   # (a whole pad row of the requested NaN)


def test_collate_on_a_stream_returns_before_the_wait(gpu):
    """With a stream the call enqueues and returns; two calls in a row on one stream take two table slots"""
    dim, frames = 40, FRAMES
    rows = _rows(dim, frames, seed=3)
    foff = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    d_in = gpu.DeviceBuffer(rows.nbytes)
    d_in.upload(rows)
    stream = C.c_void_p()
    gpu.check(gpu.lib().snf_stream_create(C.byref(stream)))
    outs = []
    try:
        for subsample in (1, 2):
            t_max = collate_np.num_out(19, subsample, 0)
            d_out, d_len = _poisoned(gpu, 5 * t_max * dim * 2), _poisoned(gpu, 20)
            gpu.collate_padded(d_in.ptr, dim, foff, 'bfloat16', 0, 0, subsample, 0, 0.0, t_max, d_out.ptr, d_len.ptr,
                               stream=stream.value)
            outs.append((subsample, t_max, d_out, d_len))
        gpu.check(gpu.lib().snf_stream_synchronize(stream))
        for subsample, t_max, d_out, d_len in outs:
            want, want_lengths = collate_np.collate(rows, foff, 'bfloat16', 0, 0, subsample, 0, 0.0, t_max)
            assert collate_np.same_bits(d_out.download(np.zeros(want.shape, np.uint16)), want, 'bfloat16')
            assert np.array_equal(d_len.download(np.zeros(5, np.int32)), want_lengths)
    finally:
        gpu.lib().snf_stream_synchronize(stream)
        gpu.lib().snf_stream_destroy(stream)
        for _, _, d_out, d_len in outs:
            d_out.free()
            d_len.free()
        d_in.free()


# ---- processors: process_all_device(...).to_host() == process_all(...) ------------------------------------------
@pytest.fixture(scope='module')
def audios(audio):
    waves = synth.ragged_utterances(11, 6, min_s=0.2, max_s=0.9)
    return [audio] + [Audio(np.ascontiguousarray(w), 16000) for w in waves]


def _equal_collections(got, want):
    assert list(got) == list(want)
    for name in want:
        assert got[name].data.dtype == np.float32 and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name].data.view(np.uint32), want[name].data.view(np.uint32)), name
        assert got[name] == want[name], name   # (times and properties as well)


PROCESSORS = {
    'filterbank': lambda: FilterbankProcessor(num_bins=40, dither=0),
    'mfcc': lambda: MfccProcessor(dither=0),
    'plp': lambda: PlpProcessor(dither=0),
    'spectrogram': lambda: SpectrogramProcessor(dither=0),
    'energy': lambda: EnergyProcessor(dither=0),
    'pitch': lambda: KaldiPitchProcessor(),
}


@pytest.mark.parametrize('route', ['memory', 'pinned'])
@pytest.mark.parametrize('kind', sorted(PROCESSORS))
def test_process_all_device_equals_process_all(gpu, audios, kind, route):
    proc = PROCESSORS[kind]()
    utts = Utterances([('utt%d' % i, a) for i, a in enumerate(audios)])
    if route == 'pinned':
        utts = utts.pin()
    want = proc.process_all(utts)
    if kind == 'pitch':
        _equal_collections(proc.process_all(utts), want)   # (the host call repeats itself bit for bit)
    resident = proc.process_all_device(utts)
    assert isinstance(resident, device.DeviceFeaturesCollection) and list(resident) == list(want)
    for name in want:
        assert resident[name].nframes == want[name].nframes and resident[name].ndims == want[name].ndims
        assert resident[name].dtype == 'float32'
    _equal_collections(resident.to_host(), want)
    one = resident['utt3']
    assert one.to_host() == want['utt3']
    assert np.array_equal(one.times, want['utt3'].times) and dict_equal(one.properties, want['utt3'].properties)
    resident.release()


def test_process_all_device_keeps_kaldis_empty_matrix(gpu, audios):
    """An utterance shorter than one window has the (0, 0) matrix on the host, and so has the device result"""
    proc = MfccProcessor(dither=0)
    short = Audio(np.zeros(100, dtype=np.int16), 16000)
    utts = Utterances([('a', audios[1]), ('short', short), ('b', audios[2])])
    want = proc.process_all(utts)
    assert want['short'].shape == (0, 0)
    resident = proc.process_all_device(utts)
    _equal_collections(resident.to_host(), want)
    assert resident['short'].to_host() == want['short']
    batch = resident.padded()
    assert batch.shape == (3, max(f.nframes for f in want.values()), 13)
    assert batch.lengths.numpy().tolist() == [want[n].nframes for n in ('a', 'short', 'b')]


@pytest.mark.parametrize('route', ['memory', 'pinned'])
def test_process_all_device_large_batch_route(gpu, route):
    """From 32 MiB of audio on, a batch goes up in pieces on two streams (Plan._run_large): the resident call takes
    the same route without its downloads.  362 ragged utterances of ~3 s: 4 pieces."""
    waves = synth.utterances(7, 362, nsamples=48000 + 6 * 16)
    utts = Utterances([('utt%03d' % i, Audio(np.ascontiguousarray(w[:48000 + 16 * (i % 7)]), 16000, validate=False))
                       for i, w in enumerate(waves)])
    assert 2 * sum(48000 + 16 * (i % 7) for i in range(362)) >= gpu._LARGE_BATCH_BYTES
    if route == 'pinned':
        utts = utts.pin()
    proc = FilterbankProcessor(num_bins=40, dither=0)
    want = proc.process_all(utts)
    resident = proc.process_all_device(utts)
    _equal_collections(resident.to_host(), want)
    resident.release()


# ---- pipeline ---------------------------------------------------------------------------------------------------
def test_extract_features_device_equals_extract_features(gpu, audios):
    config = pipeline.get_default_config('mfcc', with_pitch='kaldi', with_cmvn=True, with_delta=True)
    utts = Utterances([('utt%d' % i, audios[i + 1], 'spk%d' % (i % 2)) for i in range(4)])
    want = pipeline.extract_features(config, utts)
    resident = pipeline.extract_features_device(config, utts)
    _equal_collections(resident.to_host(), want)
    name = 'utt2'
    assert resident[name].shape == want[name].shape == (want[name].nframes, 42)
    assert dict_equal(resident[name].properties, want[name].properties)
    # the padded batch of a pipeline result against the checker fed with the host rows
    batch = resident.padded(dtype='bfloat16', left=1, right=1, subsample=3, pad_value=-1.5)
    rows = np.concatenate([want[n].data for n in batch.names])
    foff = np.concatenate([[0], np.cumsum([want[n].nframes for n in batch.names])])
    ref, lengths = collate_np.collate(rows, foff, 'bfloat16', 1, 1, 3, 0, -1.5, batch.shape[1])
    assert batch.names == list(want) and batch.shape == ref.shape and batch.dtype == 'bfloat16'
    assert collate_np.same_bits(batch.data.numpy(), ref, 'bfloat16')
    assert np.array_equal(batch.lengths.numpy(), lengths)
    assert np.array_equal(batch.times_of(name), want[name].times[0::3])
    assert batch.times_of(name).shape[0] == lengths[batch.names.index(name)]
    with pytest.raises(ValueError):
        resident.padded(max_frames=batch.shape[1] - 1, subsample=3)
    with pytest.raises(ValueError):
        resident.padded(subsample=2, offset=2)


# ---- DLPack, release, torch -------------------------------------------------------------------------------------
def _resident_fbank(audios, count=4):
    proc = FilterbankProcessor(num_bins=13, dither=0)
    utts = Utterances([('utt%d' % i, a) for i, a in enumerate(audios[:count])])
    return proc.process_all(utts), proc.process_all_device(utts)


def test_dlpack_export_of_one_utterance(gpu, audios):
    want, resident = _resident_fbank(audios)
    block = resident._blocks[0]
    one = resident['utt2']
    row0 = want['utt0'].nframes + want['utt1'].nframes
    assert one.ptr == block.buffer.ptr + 4 * 13 * row0 and one.device == gpu.get_device()
    assert one.__dlpack_device__() == (10, gpu.get_device())
    capsule = one.__dlpack__()
    tensor = _dlpack.managed_tensor(capsule).dl_tensor
    assert (tensor.device.device_type, tensor.device.device_id) == (10, gpu.get_device())
    assert tensor.data == one.ptr and tensor.byte_offset == 0
    assert (tensor.dtype.code, tensor.dtype.bits, tensor.dtype.lanes) == (2, 32, 1)
    assert tensor.ndim == 2 and [tensor.shape[0], tensor.shape[1]] == list(want['utt2'].shape)
    assert [tensor.strides[0], tensor.strides[1]] == [13, 1]
    rows = np.zeros(want['utt2'].shape, dtype=np.float32)
    gpu.check(gpu.lib().snf_memcpy_d2h(rows.ctypes.data, tensor.data, rows.nbytes))
    assert np.array_equal(rows.view(np.uint32), want['utt2'].data.view(np.uint32))
    # the capsule keeps the block alive beyond its collection, and gives it back when it goes
    address = block.buffer.ptr
    live = _dlpack.live()
    del resident, one, block, tensor
    gc.collect()
    assert not any(b[1] == address for b in gpu.DEVICE_POOL._free.get(gpu.get_device(), []))
    del capsule
    gc.collect()
    assert _dlpack.live() == live - 1
    assert any(b[1] == address for b in gpu.DEVICE_POOL._free.get(gpu.get_device(), []))


def test_release_ends_every_export(gpu, audios):
    _, resident = _resident_fbank(audios)
    one = resident['utt1']
    batch = resident.padded(dtype='float16')
    address = resident._blocks[0].buffer.ptr
    resident.release()
    assert any(b[1] == address for b in gpu.DEVICE_POOL._free.get(gpu.get_device(), []))
    for call in (one.__dlpack__, resident.padded, resident.to_host, one.to_host, lambda: one.ptr):
        with pytest.raises(RuntimeError):
            call()
    assert batch.data.numpy().shape == batch.shape   # (a batch made earlier owns its own memory)


def test_torch_takes_the_blocks_without_a_copy(gpu, audios):
    """Everything here is also checked without torch by the tests above"""
    shared, paths = device.shares_hip_runtime_with_torch()
    if not shared:
        with pytest.raises(RuntimeError) as err:
            _resident_fbank(audios, 2)[1]['utt1'].torch()
        assert all(p in str(err.value) for p in paths)
        print('torch and libshennong_hip.so are on different HIP runtimes:', paths)
        pytest.skip('torch does not share the HIP runtime of libshennong_hip.so: ' + ', '.join(paths))
    import torch
    want, resident = _resident_fbank(audios)
    one = resident['utt2']
    address = resident._blocks[0].buffer.ptr
    tensor = one.torch()
    assert tensor.data_ptr() == one.ptr and tensor.dtype == torch.float32 and tuple(tensor.shape) == one.shape
    assert np.array_equal(tensor.cpu().numpy(), want['utt2'].data)
    batch = resident.padded(dtype='bfloat16')
    assert batch.torch().dtype == torch.bfloat16 and batch.lengths.torch().dtype == torch.int32
    del resident, one, batch
    gc.collect()
    assert np.array_equal(tensor.cpu().numpy(), want['utt2'].data)   # survives its collection
    del tensor
    gc.collect()
    assert any(b[1] == address for b in gpu.DEVICE_POOL._free.get(gpu.get_device(), []))
