"""The opt-in Kaldi resampler on the host: output counts against the oracle, the `resample` attribute of the two
network processors, the argument checks of ``Audio.resample(backend='kaldi')`` and the refusal of a rate pair
whose phase table does not fit - all before any device is needed."""

import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from shennong_amd import Audio, _abi, _backend
from test_bottleneck import weights_dir, write_weights  # noqa: F401  (fixture)
from test_crepe import write_weights as write_crepe_weights

# (rate_in, rate_out) of the GPU checks (tests/test_resample_gpu.py)
RATE_PAIRS = [(16000, 8000), (8000, 16000), (32000, 8000), (48000, 16000), (44100, 8000), (44100, 16000),
              (22050, 16000), (11025, 8000), (8000, 44100)]


def cutoff(rate_in, rate_out):
    """ResampleWaveform's filter cutoff, as the float Kaldi's BaseFloat holds"""
    return np.float32(0.99 * 0.5 * min(rate_in, rate_out))


@pytest.mark.parametrize('rate_in,rate_out', RATE_PAIRS)
def test_num_out_equals_oracle(rate_in, rate_out):
    for n in (0, 1, 2, 3, 37, 1000, 1001, 22713):
        want = len(orc.linear_resample(np.zeros(n, dtype=np.float32), rate_in, rate_out, cutoff(rate_in, rate_out), 6))
        assert _backend.resample_num_out(rate_in, rate_out, n) == want, n


def test_num_out_known_answers():
    assert _backend.resample_num_out(16000, 8000, 22713) == 11357   # (the Fourier method: int(22713 / 2) = 11356)
    assert _backend.resample_num_out(16000, 8000, 22712) == 11356
    assert _backend.resample_num_out(8000, 16000, 11357) == 22714
    assert _backend.resample_num_out(16000, 16000, 5) == 5
    for bad in ((0, 8000, 5), (8000, -1, 5), (8000, 16000, -1), (1 << 23, 8000, 5)):
        with pytest.raises(ValueError):
            _backend.resample_num_out(*bad)


def test_refusals_before_any_device():
    """Equal rates, an unknown kind and a rate pair over the LDS limit are refused whether or not a device is
    there; the message of the last names the pair and both sizes"""
    L = _backend.lib()
    soff = (C.c_int64 * 2)(0, 0)
    start = (C.c_int64 * 1)(0)

    def call(rate_in, rate_out, kind=0):
        return L.snf_linear_resample(0, rate_in, rate_out, kind, None, soff, 1, None, start, None)

    assert call(16000, 16000) == _abi.SNF_E_INVALID
    assert 'both rates are 16000 Hz' in L.snf_last_error().decode()
    assert call(16000, 8000, kind=2) == _abi.SNF_E_INVALID
    assert call(44100, 16001) == _abi.SNF_E_INVALID
    message = L.snf_last_error().decode()
    # 16 001 phases of (first, count, 35 weights) 32-bit words; a chunk of 256 outputs spans 737 inputs
    assert message == ('resample 44100 -> 16001 Hz: the phase table (16001 phases, 2368148 bytes) and the staged '
                       'span (2948 bytes) do not fit in the 65536 bytes of LDS of a workgroup'), message
    with pytest.raises(ValueError, match='44100 -> 16001 Hz'):
        _backend.check(call(44100, 16001))
    # empty batches need no device either
    assert L.snf_linear_resample(0, 16000, 8000, 0, None, soff, 0, None, start, None) == _abi.SNF_OK
    assert call(16000, 8000) == _abi.SNF_OK    # one utterance of no samples


def test_audio_backend_checks():
    mono = Audio(np.zeros(100, dtype=np.int16), 16000)
    with pytest.raises(ValueError) as err:
        mono.resample(8000, backend='a_bad_one')
    assert str(err.value) == 'backend must be sox or scipy, it is a_bad_one'
    for data in (np.zeros(100, dtype=np.float64), np.zeros(100, dtype=np.int32),
                 np.zeros((100, 2), dtype=np.int16), np.zeros((100, 2), dtype=np.float32)):
        with pytest.raises(ValueError) as err:
            Audio(data, 16000).resample(8000, backend='kaldi')
        assert 'mono int16 or float32' in str(err.value) and 'backend="scipy"' in str(err.value)
    with pytest.raises(ValueError, match='resampling at 0 failed'):
        mono.resample(0, backend='kaldi')
    assert mono.resample(16000, backend='kaldi') is mono
    # the default is the Fourier method, as before
    assert mono.resample(8000).nsamples == 50
    assert 'kaldi' in Audio.resample.__doc__


def check_attribute(proc, name, params):
    assert proc.resample == 'scipy'
    assert proc.get_params() == params
    default = proc.get_properties()
    assert default[name] == params
    for bad in ('sox', 'Kaldi', 'fourier', None, 8000):
        with pytest.raises(ValueError) as err:
            proc.resample = bad
        assert 'scipy' in str(err.value) and 'kaldi' in str(err.value)
        assert proc.resample == 'scipy'
    proc.resample = 'kaldi'
    assert proc.resample == 'kaldi'
    assert proc.get_params() == params
    props = proc.get_properties()
    assert props[name] == dict(params, resample='kaldi')
    assert props['pipeline'] == default['pipeline']
    with pytest.raises(ValueError, match='invalid parameter resample'):
        proc.set_params(resample='scipy')
    assert proc.resample == 'kaldi'
    with pytest.raises(TypeError):
        type(proc)(resample='kaldi')
    proc.resample = 'scipy'
    assert proc.get_properties() == default


def test_bottleneck_attribute(weights_dir):  # noqa: F811
    from shennong_amd.processor import BottleneckProcessor
    write_weights(weights_dir)
    proc = BottleneckProcessor(dither=0)
    check_attribute(proc, 'bottleneck', {'weights': 'BabelMulti', 'dither': 0.0})
    proc.precision, proc.resample = 'bfloat16', 'kaldi'
    assert proc.get_properties()['bottleneck'] == {'weights': 'BabelMulti', 'dither': 0.0, 'precision': 'bfloat16',
                                                   'resample': 'kaldi'}


def test_crepe_attribute(tmp_path, monkeypatch):
    from shennong_amd.processor import CrepePitchProcessor
    monkeypatch.setenv('SHENNONG_AMD_CREPE_DIR', str(tmp_path))
    write_crepe_weights(tmp_path, 'tiny', 11)
    proc = CrepePitchProcessor(model_capacity='tiny')
    check_attribute(proc, 'crepe', {'model_capacity': 'tiny', 'viterbi': True, 'center': True, 'frame_shift': 0.01,
                                    'frame_length': 0.025})


def test_too_short_uses_the_resampled_length(tmp_path, monkeypatch):
    """The 'too short' check of the device path counts Kaldi's output samples, before anything is uploaded"""
    from shennong_amd.processor import CrepePitchProcessor
    monkeypatch.setenv('SHENNONG_AMD_CREPE_DIR', str(tmp_path))
    write_crepe_weights(tmp_path, 'tiny', 11)
    proc = CrepePitchProcessor(model_capacity='tiny')
    proc.resample = 'kaldi'
    with pytest.raises(ValueError) as err:
        proc.process(Audio(np.zeros(100, dtype=np.int16), 8000))
    assert str(err.value) == 'audio too short: 200 samples at 16 kHz'
