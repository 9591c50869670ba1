#!/usr/bin/env python
"""Generates tests/golden/reference_bottleneck.npz: the outputs of the reference's OWN bottleneck extractor
(shennong/processor/bottleneck.py `BottleneckProcessor.process` and the functions it calls, pure numpy /
scipy) with dither 0 and synthetic weights in the published files' format (tests/bottleneck_f64.py
`make_weights(seed, hidden, context)`: no weight array is stored, the tests regenerate them).

Run where a checkout of the reference is available (never on the GPU box):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_bottleneck.py <reference dir>

Per case the fixture holds the reference's 80-wide first-stage output and final features, per signal the
int16 input, the reference's VAD mask and its log-mel matrix before the mean subtraction (all float64).  The generator checks the conditions the tests rely on: the smallest |posterior of component 0 - 0.3| over the frames of every signal
is at least 1e-3 (so float64 EM in another summation order cannot flip a frame and the tests demand the mask
exactly), and every signal has voiced and unvoiced frames.  No reference source goes into the fixture.
"""
import logging
import os
import sys
from unittest import mock

import numpy as np
import scipy.io.wavfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bottleneck_f64 as f64  # noqa: E402

sys.path.insert(0, HERE)
import kaldi_shim  # noqa: E402

# (the reference's package imports every processor; the pykaldi modules they need are stand-ins that the
# bottleneck extractor never calls)
kaldi_shim.install()
for name in ['sox', 'pydub', 'kaldi.feat.fbank', 'kaldi.feat.mfcc', 'kaldi.feat.spectrogram', 'kaldi.feat.pitch',
             'kaldi.transform', 'kaldi.transform.cmvn', 'kaldi.ivector', 'kaldi.gmm', 'kaldi.util',
             'kaldi.util.table', 'kaldi.util.io', 'kaldi.transform.lvtln', 'kaldi.transform.mllr',
             'kaldi.gmm.am', 'kaldi.gmm.full', 'h5features', 'json_tricks', 'tensorflow', 'tensorflow.keras',
             'tensorflow.keras.layers', 'tensorflow.keras.models', 'hmmlearn', 'hmmlearn.hmm', 'joblib',
             'pkg_resources', 'yaml', 'kaldi.ivector.plda', 'kaldi.gmm.diag']:
    if name not in sys.modules:
        try:
            __import__(name)
        except Exception:  # noqa
            sys.modules[name] = mock.MagicMock()
if len(sys.argv) != 2:
    sys.exit('usage: make_golden_bottleneck.py <directory of the reference checkout>')
sys.path.insert(0, sys.argv[1])

from shennong.processor import bottleneck as ref  # noqa: E402

# (signal, seed, hidden, context)
CASES = [
    ('wav_h500_c5', 'wav', 11, 500, 5),
    ('wav_h1500_c5', 'wav', 12, 1500, 5),
    ('wav_h200_c15', 'wav', 13, 200, 15),
    ('synth_h96_c5', 'synth', 14, 96, 5),
]
MARGIN = 1e-3


def main():
    rate, wav = scipy.io.wavfile.read(os.path.join(HERE, 'test.8k.wav'))
    assert rate == 8000 and wav.dtype == np.int16
    signals = {'wav': wav, 'synth': f64.synthetic_signal()}
    log = logging.getLogger('make_golden_bottleneck')
    out = {}
    for key, samples in signals.items():
        out['input_' + key] = samples
        post = f64.vad_posterior(samples)
        margin = float(np.abs(post - 0.3).min())
        mask = ref._compute_vad(samples, log, win_length=200, win_overlap=120)
        assert np.array_equal(mask, post < 0.3), key
        assert margin >= MARGIN, (key, margin)
        assert mask.any() and not mask.all(), key
        out['margin_' + key] = np.array(margin)
        print(key, 'frames', mask.size, 'voiced', int(mask.sum()), 'margin %.3g' % margin)
    window = np.hamming(200)
    bank = ref._mel_fbank_mx(window.size, 8000, numchans=24, lofreq=64.0, hifreq=3800.0)
    for name, key, seed, hidden, context in CASES:
        samples = signals[key]
        weights = f64.make_weights(seed, hidden, context)
        proc = ref.BottleneckProcessor.__new__(ref.BottleneckProcessor)
        ref.BottleneckProcessor._loaded_weights['BabelMulti'] = weights
        proc._weights, proc._dither = 'BabelMulti', 0.0
        proc._logger = log
        audio = mock.MagicMock()
        audio.sample_rate, audio.dtype, audio.data = 8000, np.dtype(np.int16), samples
        with mock.patch.object(ref.BottleneckProcessor, 'get_properties', lambda self: {}), \
                mock.patch.object(ref, 'Features', lambda data, times, props: (data, times)):
            final, times = proc.process(audio)
        # the stages, by the reference's own functions on the same input
        mask = ref._compute_vad(samples, log, win_length=200, win_overlap=120)
        fea = ref._fbank_htk(samples, window, 120, bank)
        centred = fea - np.mean(fea[mask], axis=0)
        padded = np.r_[np.repeat(centred[[0]], 15, axis=0), centred, np.repeat(centred[[-1]], 15, axis=0)]
        again, first = ref._create_nn_extract_st_BN(ref._preprocess_nn_input(padded, context, context), weights, 2)
        assert np.array_equal(np.asarray(final), again), name
        out['vad_' + key] = mask                                   # (the same for every case of a signal)
        out['logmel_' + key] = np.asarray(fea, dtype=np.float64)
        out['bn_' + name] = np.asarray(first, dtype=np.float64)
        out['out_' + name] = np.asarray(final, dtype=np.float64)
        assert np.array_equal(np.asarray(times), f64.times(len(final))), name
        out['case_' + name] = np.array([seed, hidden, context])
        out['signal_' + name] = np.array(key)
        print(name, 'out', np.asarray(final).shape, 'range %.3g .. %.3g' % (final.min(), final.max()))
    dst = os.path.join(HERE, 'reference_bottleneck.npz')
    np.savez_compressed(dst, **out)
    print('wrote', dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
