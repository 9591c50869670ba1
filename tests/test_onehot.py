"""shennong_amd.processor.onehot on the host: the parameters, refusals and literals of the reference's
test/processor/test_onehot.py, OneHotProcessor against the reference's rows, and the numpy statement of the
framed rule (tests/onehot_np.py) against the reference on every frame of every case of
tests/golden/reference_onehot.npz.  The framed processor itself runs on the device: tests/test_onehot_gpu.py."""

import numpy as np
import pytest

import onehot_cases
import onehot_np
from shennong_amd import _backend, window
from shennong_amd.alignment import Alignment
from shennong_amd.frames import Frames
from shennong_amd.processor import FramedOneHotProcessor, MfccProcessor, OneHotProcessor
from shennong_amd.processor import onehot


@pytest.fixture(scope='module')
def alignments():
    return onehot_cases.collection()


def statement_rows(alignment, params):
    """The rows of FramedOneHotProcessor(**params).process(alignment) by the numpy statement"""
    processor = FramedOneHotProcessor(**params)
    token2index = processor._token2index(alignment)
    ids = np.array([token2index[p] for p in alignment.tokens])
    table = window.window(processor.frame.samples_per_frame, type=processor.window_type,
                          blackman_coeff=processor.blackman_coeff)
    return onehot_np.framed_onehot(
        float(alignment.onsets[0]), np.asarray(alignment.offsets, dtype=np.float64), ids, len(token2index),
        processor.sample_rate, processor.frame.samples_per_frame, processor.frame.samples_per_shift, table)


@pytest.mark.parametrize('params', [{'tokens': ['a', 'b', 'c']}, {'tokens': None}])
def test_params(params):
    assert params == OneHotProcessor(**params).get_params()
    assert params == OneHotProcessor().set_params(**params).get_params()


def test_params_framed():
    params = {'tokens': ['a', 'b', 'c'], 'sample_rate': 2, 'frame_shift': 10, 'frame_length': 25,
              'window_type': 'blackman', 'blackman_coeff': 0.5}
    assert params == FramedOneHotProcessor(**params).get_params()
    assert params == FramedOneHotProcessor().set_params(**params).get_params()
    defaults = FramedOneHotProcessor().get_params()
    assert defaults == {'tokens': None, 'sample_rate': 16000, 'frame_shift': 0.01, 'frame_length': 0.025,
                        'window_type': 'povey', 'blackman_coeff': 0.42}
    assert FramedOneHotProcessor().name == OneHotProcessor().name == 'onehot'
    assert FramedOneHotProcessor(tokens='cabbage').tokens == ['a', 'b', 'c', 'e', 'g']


def test_base(alignments):
    class Base(onehot._OneHotBase):
        def process(self, signal):
            return signal

    ali = alignments['S01F1522_0001']
    with pytest.raises(ValueError) as err:
        Base(tokens=[])._tokens_set(ali)
    assert 'following tokens are in alignment but not defined in the onehot features processor' in str(err.value)
    base = Base()
    assert base._tokens_set(ali) == ali.get_tokens_inventory()
    with pytest.raises(ValueError) as err:
        base.ndims
    assert str(err.value) == 'onehot tokens are not defined, cannot know their dimension'
    extra = ali.get_tokens_inventory()
    extra.add('!!')
    base = Base(tokens=extra)
    assert '!!' in base._tokens_set(ali)
    assert '!!' not in ali.get_tokens_inventory()
    assert base.ndims == len(extra)


def test_bad_tokens(alignments):
    phones = alignments.get_tokens_inventory()
    phones.remove('SIL')
    for processor in (OneHotProcessor(tokens=phones), FramedOneHotProcessor(tokens=phones)):
        with pytest.raises(ValueError) as err:   # (raised before anything reaches the device)
            processor.process(alignments['S01F1522_0001'])
        assert 'not defined in the onehot features processor: [' in str(err.value) and 'SIL' in str(err.value)


def test_simple(alignments):
    ali1 = alignments['S01F1522_0001']
    phones1 = ali1.get_tokens_inventory()
    everything = alignments.get_tokens_inventory()
    processor = OneHotProcessor(tokens=phones1)
    feat1 = processor.process(ali1)
    assert processor.ndims == feat1.ndims == len(phones1)
    assert feat1.shape == (ali1.tokens.shape[0], len(phones1))
    assert feat1.dtype == bool
    assert all(feat1.data.sum(axis=1) == 1)
    assert np.array_equal(feat1.times, ali1.times)
    assert set(feat1.properties['onehot'].keys()) == {'token2index', 'tokens'}
    assert feat1.properties['pipeline'] == [{'name': 'onehot', 'columns': [0, len(phones1) - 1]}]
    feat2 = OneHotProcessor(tokens=everything).process(ali1)
    assert feat2.shape == (ali1.tokens.shape[0], len(everything))
    assert all(feat2.data.sum(axis=1) == 1)
    assert np.array_equal(feat1.times, feat2.times)
    feat3 = OneHotProcessor(tokens=everything).process(alignments['S01F1522_0002'])
    assert feat3.shape == (alignments['S01F1522_0002'].tokens.shape[0], len(everything))
    assert feat2.shape[1] == feat3.shape[1] and feat1.shape[1] < feat3.shape[1]
    # without tokens: those of the alignment, recorded in the properties; the processor keeps none
    processor = OneHotProcessor()
    feat4 = processor.process(ali1)
    assert processor.tokens is None
    assert feat4.properties['onehot']['tokens'] == sorted(phones1)
    assert feat4.properties['onehot']['token2index'] == {p: i for i, p in enumerate(sorted(phones1))}
    assert np.array_equal(feat4.data, feat1.data)


def test_onehot_equals_reference(alignments):
    everything = alignments.get_tokens_inventory()
    for item, ali in alignments.items():
        assert np.array_equal(OneHotProcessor().process(ali).data, onehot_cases.expected('plain', item)), item
        assert np.array_equal(OneHotProcessor(tokens=everything).process(ali).data,
                              onehot_cases.expected('plain_all', item)), item


def test_compare_mfcc(audio):
    """The frame grid is the MFCC's for the same duration: 140, 70 and 69 frames of the reference's
    test_compare_mfcc (the rows themselves: tests/test_onehot_gpu.py)"""
    ali = Alignment.from_list([(0, 1, 'a'), (1, audio.duration, 'b')])
    for params, nframes in (({'frame_shift': 0.01}, 140), ({'frame_shift': 0.02}, 70),
                            ({'frame_shift': 0.02, 'frame_length': 0.05}, 69)):
        processor = FramedOneHotProcessor(**params)
        nsamples = int(ali.duration() * processor.sample_rate)
        assert processor.frame.nframes(nsamples) == nframes
        times = processor.frame.boundaries(nframes) / processor.sample_rate
        assert times.dtype == np.float64 and times.shape == (nframes, 2)
        assert times == pytest.approx(MfccProcessor(**params).times(nframes))
        assert statement_rows(ali, params).shape == (nframes, 2)


def test_sample_rate_too_low():
    ali = Alignment(np.asarray([[0, 1], [1, 2]]), np.asarray(['a', 'b']))
    with pytest.raises(ValueError) as err:
        FramedOneHotProcessor(sample_rate=2).process(ali)
    assert 'sample rate too low' in str(err.value)
    assert Frames(sample_rate=1000).nframes(2000) == onehot_cases.expected('rate1000', 'literal').shape[0]


def test_no_cpu_path(alignments):
    if _backend.device_count() > 0:
        pytest.skip('a GPU is visible')
    for call in (lambda: FramedOneHotProcessor().process(alignments['S01F1522_0010']),
                 lambda: FramedOneHotProcessor().process_all(alignments)):
        with pytest.raises(RuntimeError) as err:
            call()
        assert 'no HIP device' in str(err.value)
    with pytest.raises(RuntimeError) as err:
        empty = np.zeros(1, dtype=np.int64)
        _backend.check(_backend.lib().snf_framed_onehot(
            0, 16000.0, 400, 160, 2, 0.42, 0, empty.ctypes.data_as(onehot.C.POINTER(onehot.C.c_int64)), None, None,
            None, None, None, None, None, None, None, None, None))
    assert 'no HIP device' in str(err.value)


def test_statement_equals_reference():
    """tests/onehot_np.py against the reference's rows: every frame of every case, none left out (boolean, so
    there is no tolerance)"""
    cases = onehot_cases.framed_cases()
    assert len(cases) == 4 * 34 + 5 + 1 + 3 * len(onehot_cases.synthetic()) and len(onehot_cases.synthetic()) >= 200
    frames = 0
    for case, item, ali, params in cases:
        want = onehot_cases.expected(case, item)
        got = statement_rows(ali, params)
        assert got.shape == want.shape, (case, item, got.shape, want.shape)
        assert np.array_equal(got, want), (case, item, np.flatnonzero((got != want).any(axis=1))[:8])
        frames += want.shape[0]
    ref = onehot_cases.fixture()
    assert frames == sum(v.shape[0] for k, v in ref.items() if k.endswith('|winner') and not k.startswith('plain'))
    assert onehot_cases.expected('window_povey', 'S01F1522_0010').shape == (68, 7)
    first = FramedOneHotProcessor().frame
    assert np.array_equal(ref['default|S01F1522_0010|times'], first.boundaries(68) / first.sample_rate)
    low = FramedOneHotProcessor(sample_rate=1000).frame
    assert np.array_equal(ref['rate1000|literal|times'],
                          low.boundaries(ref['rate1000|literal|times'].shape[0]) / low.sample_rate)


def test_synthetic_set_has_the_hard_frames():
    """The synthetic set holds what the real file does not: exact ties (decided by first appearance), frames
    whose two halves differ in the last bits only, a token that comes back within a frame"""
    table = window.window(400, type='povey')
    ties = close = recurring = 0
    for ali in onehot_cases.synthetic():
        ids = np.unique(ali.tokens, return_inverse=True)[1]
        sampled = onehot_np.sample_ids(float(ali.onsets[0]), ali.offsets, ids, 16000)
        for f in range(onehot_np.num_frames(sampled.shape[0], 400, 160)):
            frame = sampled[f * 160:f * 160 + 400]
            runs = frame[np.concatenate(([True], frame[1:] != frame[:-1]))]
            if runs.shape[0] < 2:
                continue
            recurring += len(set(runs)) < runs.shape[0]
            counts = sorted((int((frame == t).sum()) for t in set(frame)), reverse=True)
            ties += counts[0] == counts[1]               # equal weights under the rectangular window
            weights = sorted((float(onehot_np.sequential_sum(table[frame == t])) for t in set(frame)), reverse=True)
            close += weights[0] - weights[1] <= 4e-5     # within a few float32 ulps of sums near 100
    assert ties >= 40 and close >= 40 and recurring >= 40, (ties, close, recurring)
