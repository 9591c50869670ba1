"""Where everything lies in the batches of tests/long_frame_cases.py, without a GPU: every feature that the
grid-stride walk of the long-frame kernels could mishandle sits on trip 1 and again on trip 2, the pairs that
split are decided by the reference alone (no energy ratio within a factor 2 of the kernel's threshold), and the
host mirror of the walk agrees with the launchers it was read from."""

import os
import re

import numpy as np
import pytest

import long_frame_cases as lf
from oracle import oracle as orc
from shennong_amd import _backend
from shennong_amd.processor import FilterbankProcessor, MfccProcessor

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'shennong_amd', 'csrc')
BATCHES = [(rate, snip) for _, rate, _, _ in lf.MULTI_TRIP_CASES for snip in (True, False)]


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_walk_constants_are_the_launchers():
    """256 workgroups of kLongWaves waves, a stride of gridDim.x * kLongWaves, a split beyond kSplitRatio"""
    assert re.search(r'constexpr int kLongWaves = %d;' % lf.LONG_WAVES, _source('device_fft1024.h'))
    for name in ('kernels_fbank1024x2.hip', 'kernels_fbank2048.hip'):
        text = _source(name)
        assert 'if (blocks > %d) blocks = %d;' % (lf.MAX_BLOCKS, lf.MAX_BLOCKS) in text
        assert 'const int64_t stride = static_cast<int64_t>(gridDim.x) * kLongWaves;' in text
        assert 'int64_t g = static_cast<int64_t>(blockIdx.x) * kLongWaves + wid;' in text
    pair = _source('kernels_fbank1024x2.hip')
    assert 'constexpr float kSplitRatio = %.1ff;' % lf.SPLIT_RATIO in pair
    assert 'split = hi > split_ratio * lo;' in pair
    assert lf.STRIDE == 4096
    assert lf.RATIO_MARGIN == (lf.SPLIT_RATIO / 2, lf.SPLIT_RATIO * 2)
    assert lf.stride_of(5) == 16 and lf.stride_of(4096) == 4096 and lf.stride_of(4097) == 4096
    assert lf.stride_of(4080) == 4080 and lf.stride_of(4081) == 4096
    assert lf.trip_of(np.array([0, 4095, 4096, 8192]), 9000).tolist() == [0, 0, 1, 2]


def test_pair_table_mirror():
    utt, frame_a, has_b = lf.pair_table([3, 1, 0, 4, 2], skipped=[False, False, False, False, True])
    assert utt.tolist() == [0, 0, 1, 3, 3]
    assert frame_a.tolist() == [0, 2, 3, 4, 6]
    assert has_b.tolist() == [True, False, False, True, True]
    assert lf.frame_table([2, 0, 3]).tolist() == [0, 0, 2, 2, 2]


@pytest.mark.parametrize('kernel, sample_rate, win_len, nj', lf.MULTI_TRIP_CASES)
def test_geometry_of_the_cases(kernel, sample_rate, win_len, nj):
    frame = MfccProcessor(sample_rate=sample_rate)._build_options().frame
    assert lf.geometry(sample_rate) == (orc.window_shift(frame), orc.window_size(frame), orc.padded_window_size(frame))
    assert lf.geometry(sample_rate)[1] == win_len and lf.expected_nj(kernel, win_len) == nj
    assert lf.unit_of(sample_rate) == ('pairs' if kernel == 'fbank1024x2_kernel' else 'frames')


@pytest.mark.parametrize('sample_rate, snip_edges', BATCHES)
def test_every_feature_lies_on_trip_one_and_on_trip_two(sample_rate, snip_edges):
    waves, warps = lf.multi_trip_batch(sample_rate, snip_edges)
    labels = lf.batch_labels(sample_rate, snip_edges)
    frame = MfccProcessor(sample_rate=sample_rate, snip_edges=snip_edges)._build_options().frame
    counts = lf.frame_counts(waves, sample_rate, snip_edges)
    assert counts.tolist() == [orc.num_frames(frame, len(w)) for w in waves]
    assert 150 <= len(waves) <= 250 and len(warps) == len(waves) == len(labels)
    # one launch
    assert 2 * sum(len(w) for w in waves) < _backend._LARGE_BATCH_BYTES
    utt, row = lf.unit_table(waves, sample_rate, snip_edges)
    n = len(utt)
    assert 2 * lf.STRIDE < n < 3 * lf.STRIDE and n % lf.LONG_WAVES != 0
    assert lf.stride_of(n) == lf.STRIDE
    trip = lf.trip_of(np.arange(n), n)
    assert set(trip.tolist()) == {0, 1, 2}
    skipped = lf.left_out(waves, sample_rate, snip_edges)
    # (without snip_edges an utterance of one frame is shorter than a window: the generic kernel's)
    assert all(labels[u] == 'one_frame' for u in np.nonzero(skipped)[0]) and skipped.any() == (not snip_edges)
    first_unit = {}
    for i, u in enumerate(utt.tolist()):
        first_unit.setdefault(u, i)
    for name in lf.FEATURES:
        where = [u for u, label in enumerate(labels) if label == name]
        if name == 'one_frame' and not snip_edges:
            # (no unit of its own: it lies between utterances of the later trips all the same)
            units = [first_unit[u + 1] for u in where]
        else:
            units = [first_unit[u] for u in where]
        assert any(lf.STRIDE <= i < 2 * lf.STRIDE for i in units), name
        assert any(i >= 2 * lf.STRIDE for i in units), name
    by_label = lambda name: [u for u, label in enumerate(labels) if label == name]   # noqa: E731
    assert all(counts[u] % 2 == 0 for u in by_label('even') + by_label('split_tail'))
    assert all(counts[u] % 2 == 1 for u in by_label('odd') + by_label('last_odd'))
    assert all(counts[u] == 1 for u in by_label('one_frame')) and all(counts[u] == 3 for u in by_label('three_frames'))
    # neighbouring utterances with different warps behind both seams, all three warps on every trip
    for lo in (lf.STRIDE, 2 * lf.STRIDE):
        us = sorted(set(utt[lo:lo + 600].tolist()))
        assert {warps[u] for u in us} == set(lf.WARPS)
        assert any(warps[a] != warps[b] for a, b in zip(us, us[1:]))
    # a wave meets another warp (and another utterance) on each of its trips
    w_of = np.array(warps)[utt]
    third = n - 2 * lf.STRIDE
    changes = (w_of[:third] != w_of[lf.STRIDE:lf.STRIDE + third]) & \
        (w_of[lf.STRIDE:lf.STRIDE + third] != w_of[2 * lf.STRIDE:])
    assert changes.sum() > 100
    # the last pair of the table is a single frame
    assert labels[-1] == 'last_odd' and utt[-1] == len(waves) - 1
    if lf.unit_of(sample_rate) == 'pairs':
        has_b = lf.pair_table(counts, skipped)[2]
        assert not has_b[-1]
        # a single frame follows a pair and a pair a single frame in the same seat, on the later trips
        for lo in (lf.STRIDE, 2 * lf.STRIDE):
            assert (~has_b[lo:]).sum() >= 5
    trips = lf.row_trips(waves, sample_rate, snip_edges)
    assert (trips >= 0).sum() == counts[~skipped].sum() and (trips == -1).sum() == counts[skipped].sum()


@pytest.mark.parametrize('sample_rate, snip_edges', [b for b in BATCHES if lf.unit_of(b[0]) == 'pairs'])
def test_split_pairs_are_decided_by_the_reference(sample_rate, snip_edges):
    waves, _ = lf.multi_trip_batch(sample_rate, snip_edges)
    labels = lf.batch_labels(sample_rate, snip_edges)
    counts = lf.frame_counts(waves, sample_rate, snip_edges)
    skipped = lf.left_out(waves, sample_rate, snip_edges)
    utt, frame_a, has_b = lf.pair_table(counts, skipped)
    split, ratio = lf.split_pairs(waves, sample_rate, snip_edges)
    assert split.shape == utt.shape
    # the margin: a float32 rounding of the energies cannot move a pair across the threshold
    assert not lf.in_margin(ratio).any(), ratio[lf.in_margin(ratio)]
    assert not split[~has_b].any()
    n = len(utt)
    trip = lf.trip_of(np.arange(n), n)
    first = np.concatenate([[0], np.cumsum(counts)])
    for t in (1, 2):
        on = split & (trip == t)
        # every quiet-beside-loud signal splits on this trip, the fillers never do
        assert {labels[u] for u in utt[on]} == {'unequal0', 'unequal1', 'unequal2', 'unequal3', 'split_tail'}
        # a split pair whose frame b is the last frame of its utterance (snip_edges = False: a reflected one)
        tails = [i for i in np.nonzero(on)[0] if frame_a[i] + 2 == first[utt[i] + 1]]
        assert any(labels[utt[i]] == 'split_tail' for i in tails)
        # ... and one whose frame b is an inner frame (the replay carries no flag)
        assert len(tails) < on.sum()
    assert not split[[labels[u] in ('filler', 'even', 'odd', 'three_frames', 'last_odd') for u in utt]].any()


def test_windowed_energies_are_the_oracles():
    """the float64 framing that predicts the splits against the C oracle's ExtractWindow + ProcessWindow, on the
    frames of a signal with reflected edges and a quiet stretch"""
    for sample_rate, snip_edges in ((22050, False), (32000, True)):
        wave = lf.split_tail_signal(8, sample_rate, snip_edges, seed=3)
        frame = MfccProcessor(sample_rate=sample_rate, snip_edges=snip_edges, dither=0)._build_options().frame
        energies = lf.windowed_energies(wave, sample_rate, snip_edges)
        assert energies.shape == (8,)
        for f in range(8):
            window, _ = orc.extract_window(frame, wave, f)
            np.testing.assert_allclose(energies[f], (window.astype(np.float64) ** 2).sum(), rtol=1e-4)
        ratios = lf.pair_ratios(wave, sample_rate, snip_edges)
        assert (ratios[:3] < lf.RATIO_MARGIN[0]).all() and ratios[3] > 2 * lf.RATIO_MARGIN[1]


def test_probes_change_trip_when_the_batch_is_rotated():
    for sample_rate, snip_edges in BATCHES:
        waves, _ = lf.multi_trip_batch(sample_rate, snip_edges)
        labels = lf.batch_labels(sample_rate, snip_edges)
        picked = lf.probes(sample_rate, snip_edges)
        assert 8 <= len(picked) <= 10 and len(set(picked)) == len(picked)
        assert {'unequal0', 'unequal3', 'split_tail', 'one_frame'} <= {labels[i] for i in picked}
        by = len(waves) // 3
        order = lf.rotated(list(range(len(waves))), by)
        turned = [waves[i] for i in order]
        skipped = lf.left_out(waves, sample_rate, snip_edges)

        def place(batch, index):
            utt, _ = lf.unit_table(batch, sample_rate, snip_edges)
            first = int(np.searchsorted(utt, index))
            return int(lf.trip_of(first, len(utt))), first % lf.STRIDE
        for i in picked:
            if skipped[i]:
                continue
            before, after = place(waves, i), place(turned, order.index(i))
            assert before[0] >= 1 and before[0] != after[0] and before[1] != after[1], (labels[i], before, after)


def test_window_and_bank_cases():
    cases = lf.window_cases()
    assert [lf.expected_nj('fbank1024x2_kernel', w) for w in cases['fbank1024x2_kernel']] == [9, 9, 9, 9, 13, 13, 16, 16, 16]
    assert [w // 8 for w in cases['fbank1024x2_kernel'][:3]] == [64, 64, 65]          # n_full: one piece a lane, two
    assert {w % 8 for w in cases['fbank1024x2_kernel']} >= {0, 1, 7}
    assert [lf.expected_nj('fbank2048_kernel', w) for w in cases['fbank2048_kernel']] == [9, 9, 10, 10, 16, 16, 16]
    for kernel, wins in cases.items():
        for win_len in wins + ((lf.BANK_WINDOWS[kernel],) if kernel in lf.BANK_WINDOWS else ()):
            proc = FilterbankProcessor(sample_rate=lf.SEAM_RATE, frame_length=lf.frame_length_for(win_len))
            frame = proc._build_options().frame
            assert orc.window_size(frame) == win_len
            assert orc.padded_window_size(frame) == (1024 if win_len <= 1024 else 2048)
            for snip_edges in (True, False):
                waves, warps = lf.seam_batch(win_len, snip_edges)
                frame.snip_edges = snip_edges
                assert [orc.num_frames(frame, len(w)) for w in waves] == [35, 36, 1] and warps == [0.9, 1.0, 1.15]
