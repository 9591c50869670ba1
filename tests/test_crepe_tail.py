"""The CREPE pitch entry of the pipeline and the tail behind it, without a device: the float64 statement of the
row resampling (tests/crepe_tail_f64.py) against scipy, the configuration layer, and how CrepeBatch.convert turns
the status vector of ``snf_crepe_voicing_convert`` into the host path's exceptions."""

import numpy as np
import pytest
import scipy.signal

import crepe_tail_f64 as tail
from shennong_amd import pipeline
from shennong_amd.processor import CrepePitchPostProcessor, CrepePitchProcessor
from shennong_amd.processor import pitch_crepe


@pytest.mark.parametrize('N,M', tail.PAIRS + [tail.LONG_PAIR])
def test_direct_sum_is_scipy_resample(N, M):
    """Bound 16 N 2^-52 max|column|: N rounded terms, each with |D| / N <= 1, and a factor 16 over one rounding
    per term for the cosines and the sum over k (measured: 30 times under it)"""
    x = tail.decoder_like_rows(N, 1000 * N + M)
    want = scipy.signal.resample(x, M)
    got = tail.resample_rows(x, M)
    assert got.shape == want.shape == (M, 2)
    if M == N:
        assert np.array_equal(got, x)
    for column in range(2):
        bound = 16 * N * 2.0 ** -52 * np.abs(x[:, column]).max()
        err = np.abs(got[:, column] - want[:, column]).max()
        print('(%d, %d) column %d: error %.3g, bound %.3g, ratio %.3g' % (N, M, column, err, bound, err / bound))
        assert err <= bound, (N, M, column, err, bound)


def test_crepe_pitch_config_layout():
    entry = pipeline.get_crepe_pitch_config()
    assert list(entry)[0] == 'processor' and entry['processor'] == 'crepe'
    params = CrepePitchProcessor().get_params()
    assert set(params) >= {'frame_length', 'frame_shift', 'model_capacity', 'viterbi', 'center'}
    assert {k: v for k, v in entry.items() if k not in ('processor', 'postprocessing')} == \
        {k: v for k, v in params.items() if k not in ('frame_length', 'frame_shift', 'sample_rate')}
    assert entry['postprocessing'] == CrepePitchPostProcessor().get_params()
    # a fresh dictionary every time: the caller edits it
    entry['postprocessing']['delay'] = 3
    assert pipeline.get_crepe_pitch_config()['postprocessing']['delay'] == 0


def crepe_config():
    config = pipeline.get_default_config('mfcc', with_delta=True)
    config['pitch'] = pipeline.get_crepe_pitch_config()
    return config


def test_init_config_takes_the_crepe_entry():
    """(fails on the parent commit: 'only the kaldi pitch processor is available in this backend')"""
    config = pipeline._init_config(crepe_config())
    assert config['pitch']['processor'] == 'crepe'
    # as YAML text, and without the 'postprocessing' entry, which is added like for Kaldi
    short = crepe_config()
    del short['pitch']['postprocessing']
    text = pipeline._get_config_to_yaml(short, comments=False)
    assert 'processor: crepe' in text and pipeline._init_config(text)['pitch']['postprocessing'] == {}


@pytest.mark.parametrize('where', ['pitch', 'postprocessing'])
def test_init_config_refuses_an_unknown_crepe_parameter(where):
    config = crepe_config()
    (config['pitch'] if where == 'pitch' else config['pitch']['postprocessing'])['no_such_parameter'] = 1
    with pytest.raises(ValueError, match='error in configuration.*no_such_parameter'):
        pipeline._init_config(config)
    config = crepe_config()
    config['pitch']['model_capacity'] = 'huge'
    with pytest.raises(ValueError, match='error in configuration.*huge'):
        pipeline._init_config(config)


def test_init_config_info_line(caplog):
    import logging
    from shennong_amd.logger import get_logger
    log = get_logger('pipeline', 'info')
    log.propagate = True
    try:
        with caplog.at_level(logging.INFO):
            pipeline._init_config(crepe_config(), log=log)
            assert 'crepe pitch' in caplog.text and 'kaldi pitch' not in caplog.text
            caplog.clear()
            pipeline._init_config(pipeline.get_default_config('mfcc', with_pitch='kaldi'), log=log)
            assert 'kaldi pitch' in caplog.text
    finally:
        log.propagate = False


def test_default_config_still_refuses_crepe():
    with pytest.raises(ValueError, match='crepe pitch is not available in this backend'):
        pipeline.get_default_config('mfcc', with_pitch='crepe')
    assert 'get_crepe_pitch_config' in pipeline.get_default_config.__doc__


def test_crepe_memory_is_counted():
    """1440 bytes of activation per network frame and the smaller blocks beside it: 100 frames a second"""
    config = crepe_config()
    assert pipeline._CREPE_BYTES_PER_FRAME >= 1440
    copy = 2 * 16000 * 3600   # the 16 kHz copy of audio at another rate
    assert pipeline._crepe_bytes_per_hour(config) == 360000 * pipeline._CREPE_BYTES_PER_FRAME + copy
    config['mfcc']['frame_shift'] = 0.005
    assert pipeline._crepe_bytes_per_hour(config) == 720000 * pipeline._CREPE_BYTES_PER_FRAME + copy
    assert pipeline._crepe_bytes_per_hour(pipeline.get_default_config('mfcc', with_pitch='kaldi')) == 0
    assert pipeline._crepe_bytes_per_hour(pipeline.get_default_config('mfcc')) == 0


class _FakeBuffer:
    def __init__(self, nbytes, device=None):
        self.ptr, self.nbytes, self.device, self.freed = 4096, nbytes, 0, False

    def download(self, array):
        array[...] = _FakeBackend.status[:array.shape[0]]
        return array

    def free(self, synced=False):
        self.freed = True


class _FakeLib:
    @staticmethod
    def snf_crepe_voicing_convert(*args):
        _FakeBackend.calls.append(args)
        return 0


class _FakeBackend:
    """What CrepeBatch.convert touches of shennong_amd._backend, with the status vector injected"""
    status, calls = None, []
    DeviceBuffer = _FakeBuffer

    @staticmethod
    def lib():
        return _FakeLib

    @staticmethod
    def check(rc):
        assert rc == 0


def fake_batch(monkeypatch, status):
    monkeypatch.setattr(pitch_crepe, '_backend', _FakeBackend)
    _FakeBackend.status, _FakeBackend.calls = np.asarray(status, dtype=np.int32), []
    batch = pitch_crepe.CrepeBatch.__new__(pitch_crepe.CrepeBatch)
    batch.device, batch.n = 0, len(status)
    batch.roff = np.arange(len(status) + 1, dtype=np.int64) * 5
    batch.total_rows = int(batch.roff[-1])
    batch.resampled = _FakeBuffer(16 * batch.total_rows)
    return batch


@pytest.mark.parametrize('status,message', [
    ([0, 1, 2], 'No voiced frames'),
    ([0, 0, 2, 1], 'Not all pitch values are positive: issue with extracted pitch or interpolation'),
    ([3, 0, 0], r'f\(a\) and f\(b\) must have different signs'),
    ([0, 3, 1], r'f\(a\) and f\(b\) must have different signs')])
def test_convert_raises_for_the_first_bad_utterance(monkeypatch, status, message):
    batch = fake_batch(monkeypatch, status)
    with pytest.raises(ValueError, match='^' + message + '$'):
        batch.convert()
    assert len(_FakeBackend.calls) == 1 and batch.status.tolist() == status
    assert not batch.nccf_pitch.freed   # (the rows of the good utterances can still be read)


def test_convert_passes_a_clean_status(monkeypatch):
    batch = fake_batch(monkeypatch, [0, 0])
    batch.convert()
    assert batch.status.tolist() == [0, 0] and batch.nccf_pitch.nbytes == 8 * 10
    batch = fake_batch(monkeypatch, [0, 7])
    with pytest.raises(RuntimeError, match='unknown status 7'):
        batch.convert()


def test_the_messages_are_the_host_path_s():
    """The three texts, raised by the host functions themselves"""
    from shennong_amd import Features
    post, times = CrepePitchPostProcessor(), CrepePitchProcessor().times(4)

    def host(rows):
        with pytest.raises(ValueError) as err:
            post._convert(Features(np.asarray(rows, dtype=np.float64), times, validate=False))
        return str(err.value)
    messages = pitch_crepe._STATUS_MESSAGES
    assert host([[0.0, 100.0]] * 4) == messages[1]
    assert host([[0.9, 100.0], [0.9, 0.0], [0.9, 100.0], [0.9, 100.0]]) == messages[2]
    assert host([[0.9, 100.0], [0.99995, 100.0], [0.9, 100.0], [0.9, 100.0]]) == messages[3]


def test_voicing_model_is_the_host_functions():
    model = pitch_crepe.voicing_model()
    assert model.shape == (11,) and model.dtype == np.float64
    assert model[0] == np.log(2 * np.pi * 0.25) and model[4] == np.log(0.5)
    assert model[5] == model[8] == np.log(0.99) and model[6] == model[7] == np.log(0.01)
    assert model[9] == pitch_crepe._nccf_to_pov(0.0) and model[10] == pitch_crepe._nccf_to_pov(1.0)
    assert model[9] < 1e-3 and 0.9998 < model[10] < 0.99995
