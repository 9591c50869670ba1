"""FramedOneHotProcessor on the device (snf_framed_onehot, csrc/kernels_onehot.hip) against the reference's rows
(tests/golden/reference_onehot.npz) and the numpy statement of the rule (tests/onehot_np.py): every frame of
every case, bit for bit - the rows are boolean, there is no tolerance."""

import ctypes as C

import numpy as np
import pytest

import onehot_cases
import onehot_np
from shennong_amd import _abi, window
from shennong_amd.alignment import Alignment
from shennong_amd.features import FeaturesCollection
from shennong_amd.processor import FramedOneHotProcessor, MfccProcessor

pytestmark = pytest.mark.gpu


def statement_winners(alignment, processor):
    token2index = processor._token2index(alignment)
    ids = np.array([token2index[p] for p in alignment.tokens])
    table = window.window(processor.frame.samples_per_frame, type=processor.window_type,
                          blackman_coeff=processor.blackman_coeff)
    return onehot_np.framed_winners(
        float(alignment.onsets[0]), np.asarray(alignment.offsets, dtype=np.float64), ids, processor.sample_rate,
        processor.frame.samples_per_frame, processor.frame.samples_per_shift, table)


def test_every_case_equals_reference_and_statement(gpu):
    """One batch per distinct parameter set (process_all); the reference and the statement on every frame"""
    groups = {}
    for case, item, ali, params in onehot_cases.framed_cases():
        groups.setdefault(case, (params, []))[1].append((item, ali))
    frames = 0
    for case, (params, members) in groups.items():
        processor = FramedOneHotProcessor(**params)
        got = processor.process_all({item: ali for item, ali in members})
        assert isinstance(got, FeaturesCollection) and list(got) == [item for item, _ in members]
        for item, ali in members:
            want = onehot_cases.expected(case, item)
            data = got[item].data
            assert data.dtype == bool and data.shape == want.shape, (case, item, data.shape, want.shape)
            differ = np.flatnonzero((data != want).any(axis=1))
            assert differ.size == 0, (case, item, differ[:8])
            assert np.array_equal(np.argmax(data, axis=1), statement_winners(ali, processor)), (case, item)
            assert np.all(data.sum(axis=1) == 1)
            frames += want.shape[0]
    ref = onehot_cases.fixture()
    assert frames == sum(v.shape[0] for k, v in ref.items() if k.endswith('|winner') and not k.startswith('plain'))


def test_features(gpu):
    alignments = onehot_cases.collection()
    ali = alignments['S01F1522_0010']
    assert ali.duration() == pytest.approx(0.7)
    processor = FramedOneHotProcessor()
    feat = processor.process(ali)
    assert feat.dtype == bool and feat.shape == (68, len(ali.get_tokens_inventory())) and feat.is_valid()
    assert feat.times.dtype == np.float64 and feat.times.shape == (68, 2)
    assert np.array_equal(feat.times, onehot_cases.fixture()['default|S01F1522_0010|times'])
    assert np.array_equal(feat.times, processor.frame.boundaries(68) / processor.sample_rate)
    assert ali.duration() - processor.frame_length <= feat.times[-1, -1] <= ali.duration() + processor.frame_length
    assert processor.tokens is None
    assert set(feat.properties['onehot']) == {'tokens', 'sample_rate', 'frame_shift', 'frame_length', 'window_type',
                                             'blackman_coeff', 'token2index'}
    assert feat.properties['onehot']['tokens'] == sorted(ali.get_tokens_inventory())
    assert feat.properties['onehot']['token2index'] == {p: i for i, p in enumerate(sorted(set(ali.tokens)))}
    assert feat.properties['pipeline'] == [{'name': 'onehot', 'columns': [0, feat.shape[1] - 1]}]
    everything = alignments.get_tokens_inventory()
    wide = FramedOneHotProcessor(tokens=everything).process(ali)
    assert wide.shape == (68, 32)
    columns = [sorted(everything).index(p) for p in sorted(ali.get_tokens_inventory())]
    assert np.array_equal(wide.data[:, columns], feat.data)
    low = FramedOneHotProcessor(sample_rate=1000).process(
        Alignment(np.asarray([[0, 1], [1, 2]]), np.asarray(['a', 'b'])))
    assert low.dtype == bool and low.nframes == processor.frame.__class__(sample_rate=1000).nframes(2000)
    assert np.array_equal(low.times, onehot_cases.fixture()['rate1000|literal|times'])


def test_compare_mfcc(gpu, audio):
    ali = Alignment.from_list([(0, 1, 'a'), (1, audio.duration, 'b')])
    feat = FramedOneHotProcessor(frame_shift=0.01).process(ali)
    mfcc = MfccProcessor(frame_shift=0.01).process(audio)
    assert feat.shape == (140, 2)
    assert feat.times == pytest.approx(mfcc.times)
    assert FramedOneHotProcessor(frame_shift=0.02).process(ali).shape == (70, 2)
    assert FramedOneHotProcessor(frame_shift=0.02, frame_length=0.05).process(ali).shape == (69, 2)


def test_process_all_equals_process(gpu):
    """The rows of an alignment are the same bits alone and in the batch, over its own inventory and over the
    collection's"""
    alignments = onehot_cases.collection()
    for tokens in (None, alignments.get_tokens_inventory()):
        processor = FramedOneHotProcessor(tokens=tokens)
        batch = processor.process_all(alignments)
        assert list(batch) == list(alignments)
        for item, ali in alignments.items():
            alone = processor.process(ali)
            assert alone.data.tobytes() == batch[item].data.tobytes() and alone.shape == batch[item].shape, item
            assert np.array_equal(alone.times, batch[item].times)
            assert alone.properties == batch[item].properties
            assert np.all(batch[item].data.sum(axis=1) == 1)
    synthetic = {f'{i:03d}': a for i, a in enumerate(onehot_cases.synthetic())}
    processor = FramedOneHotProcessor(window_type='rectangular')
    forward = processor.process_all(synthetic)
    backward = processor.process_all({k: synthetic[k] for k in reversed(list(synthetic))})
    for item in list(synthetic)[::9]:
        alone = processor.process(synthetic[item])
        assert alone.data.tobytes() == forward[item].data.tobytes() == backward[item].data.tobytes(), item
    with pytest.raises(ValueError):
        processor.process_all(synthetic, njobs=0)


def test_c_abi_ragged_batch(gpu):
    """snf_framed_onehot called directly: a ragged batch with an alignment shorter than one frame (no rows) and an
    empty one; the int32 winners agree with the dense rows, the padding between alignments is zero"""
    synthetic = onehot_cases.synthetic()
    short = [a for a in synthetic if int(a.duration() * 16000) < 400]
    assert short
    batch = [synthetic[0], short[0], synthetic[150], Alignment.from_list([]), synthetic[199], synthetic[3]]
    length, shift, rate = 400, 160, 16000.0
    maps = [{p: i for i, p in enumerate(sorted(set(a.tokens)))} for a in batch]
    widths = np.array([len(m) for m in maps], dtype=np.int32)
    seg_off = np.cumsum([0] + [a.tokens.shape[0] for a in batch]).astype(np.int64)
    onset0 = np.array([a.onsets[0] if a.tokens.shape[0] else 0.0 for a in batch], dtype=np.float64)
    offsets = np.concatenate([np.asarray(a.offsets, dtype=np.float64) for a in batch if a.tokens.shape[0]])
    ids = np.array([m[p] for a, m in zip(batch, maps) for p in a.tokens], dtype=np.int32)
    nsamples = np.array([int(a.duration() * rate) for a in batch], dtype=np.int64)
    nframes = np.array([onehot_np.num_frames(int(n), length, shift) for n in nsamples], dtype=np.int64)
    assert nframes[1] == 0 and nframes[3] == 0 and nframes[0] > 0
    row_off = np.cumsum([0] + [(int(f) * int(w) + 15) // 16 * 16 for f, w in zip(nframes, widths)]).astype(np.int64)
    total = int(nframes.sum())
    d_winner = gpu.DeviceBuffer(4 * total)
    d_rows = gpu.DeviceBuffer(int(row_off[-1]))
    gpu.check(gpu.lib().snf_memset(C.c_void_p(d_rows.ptr), 0xFF, int(row_off[-1])))
    p64, p32, pf64 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ms = C.c_float(-1.0)

    def call(frames, rows_at=None):
        return gpu.lib().snf_framed_onehot(
            gpu.get_device(), rate, length, shift, _abi.WINDOW_TYPES['povey'], 0.42, len(batch),
            seg_off.ctypes.data_as(p64), onset0.ctypes.data_as(pf64), offsets.ctypes.data_as(pf64),
            ids.ctypes.data_as(p32), nsamples.ctypes.data_as(p64), frames.ctypes.data_as(p64),
            widths.ctypes.data_as(p32), (row_off if rows_at is None else rows_at).ctypes.data_as(p64),
            C.c_void_p(d_winner.ptr), C.c_void_p(d_rows.ptr), C.byref(ms), None)

    gpu.check(call(nframes))
    assert ms.value > 0
    winners = d_winner.download(np.empty(total, dtype=np.int32))
    rows = d_rows.download(np.empty(int(row_off[-1]), dtype=np.uint8))
    assert set(np.unique(rows)) <= {0, 1}
    frame_off = np.cumsum([0] + list(nframes))
    table = window.window(length)
    for a, ali in enumerate(batch):
        frames, width = int(nframes[a]), int(widths[a])
        mine = winners[frame_off[a]:frame_off[a + 1]]
        block = rows[row_off[a]:row_off[a + 1]]
        dense = block[:frames * width].reshape(frames, width)
        assert not block[frames * width:].any()
        assert np.all(dense.sum(axis=1) == 1)
        if frames:
            assert np.array_equal(np.argmax(dense, axis=1).astype(np.int32), mine)
            want = onehot_np.framed_winners(float(ali.onsets[0]), np.asarray(ali.offsets), [maps[a][p] for p in ali.tokens],
                                            rate, length, shift, table)
            assert np.array_equal(mine, want), a
    # what the kernels index with is refused on the host
    too_many = nframes.copy()
    too_many[0] += 1
    unaligned = row_off.copy()
    unaligned[1:] += 8
    for rc in (call(too_many), call(nframes, unaligned)):
        with pytest.raises(ValueError):
            gpu.check(rc)
    d_winner.free()
    d_rows.free()


def test_winners_match_rows(gpu):
    """The winners the batch path reads back are the set column of every row"""
    synthetic = onehot_cases.synthetic()
    processor = FramedOneHotProcessor(window_type='hamming')
    record = {}
    feats = processor._process_batch(synthetic, timing=record)
    assert record['kernel_ms'] > 0
    assert np.array_equal(record['winners'], np.concatenate([np.argmax(f.data, axis=1) for f in feats if f.nframes]))
