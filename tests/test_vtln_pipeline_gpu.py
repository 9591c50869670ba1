"""GPU checks of VTLN training through the pipeline: snf_vtln_gram_rows against snf_vtln_gram on the rows
gathered on the host, the device-resident mapping sweep against the host round trip it replaces (bit for
bit), and extract_features / extract_features_streamed with a 'vtln' entry against precomputed warps"""

import os

import numpy as np
import pytest
import scipy.io.wavfile

from shennong_amd import Utterances, _backend, pipeline
from shennong_amd import lvtln as LV
from shennong_amd.processor import vtln as vtln_module
from shennong_amd.processor.ubm import DiagUbmProcessor
from shennong_amd.processor.vtln import VtlnProcessor

pytestmark = pytest.mark.gpu

UBM = {'num_gauss': 4, 'num_iters_init': 1, 'num_iters': 1, 'num_frames': 100, 'vad': {'energy_threshold': 0}}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('D', [13, 39, 64])
def test_gram_rows_equals_gram_on_gathered_rows(gpu, D, weighted):
    rng = np.random.RandomState(D + weighted)
    sizes = [3000, 1700]                    # two blocks
    xs = [(rng.randn(n, D) * 2 + 0.5).astype(np.float32) for n in sizes]
    ys = [(rng.randn(n, D) + 1).astype(np.float32) for n in sizes]
    F = 5000                                # more than two 2 048-frame items
    block = rng.randint(0, 2, F).astype(np.int32)
    row = np.asarray([rng.randint(0, sizes[b]) for b in block], np.int64)
    w = rng.rand(F).astype(np.float32) if weighted else None
    dxb = [_backend.upload_rows([x], np.float32) for x in xs]
    dyb = [_backend.upload_rows([y], np.float32) for y in ys]
    dblock, drow = LV.upload_row_list(block, row)
    dw = _backend.upload_rows([w], np.float32) if weighted else None
    got = LV.vtln_gram_rows(dxb, dyb, dblock, drow, F, D, dw)
    gx = np.stack([xs[b][r] for b, r in zip(block, row)])
    gy = np.stack([ys[b][r] for b, r in zip(block, row)])
    want = LV.vtln_gram(_backend.upload_rows([gx], np.float32), _backend.upload_rows([gy], np.float32), F, D, dw)
    assert same_bits(got, want)
    # a single item, and a prefix of the list
    for n in (1, 2048, 2049):
        want = LV.vtln_gram(_backend.upload_rows([gx[:n]], np.float32), _backend.upload_rows([gy[:n]], np.float32),
                            n, D, dw)
        assert same_bits(LV.vtln_gram_rows(dxb, dyb, dblock, drow, n, D, dw), want), n


def test_gram_rows_no_frames(gpu):
    D = 13
    dxb = [_backend.upload_rows([np.ones((4, D), np.float32)], np.float32)]
    dblock, drow = LV.upload_row_list(np.zeros(0, np.int32), np.zeros(0, np.int64))
    got = LV.vtln_gram_rows(dxb, dxb, dblock, drow, 0, D)
    assert got.shape == (2 * D + 1, 2 * D + 1) and not got.any()


def reference_corpus(tmp_path, wav_file, by_speaker):
    """the corpus of test_vtln_gpu.test_process_reference: 16 kHz int16, float32 and 8 kHz audio"""
    rate, data = scipy.io.wavfile.read(wav_file)
    f32 = str(tmp_path / 'test.f32.wav')
    scipy.io.wavfile.write(f32, rate, (data / 2 ** 15).astype(np.float32))
    wav8 = os.path.join(os.path.dirname(wav_file), 'test.8k.wav')
    return Utterances([('utt1', wav_file, 'spk1', 0, 1.2), ('utt2', f32, 'spk1', 0.1, 1.4),
                       ('utt3', wav8, 'spk2', 0, 1.3)] if by_speaker else
                      [('utt1', wav_file, 0, 1.2), ('utt2', f32, 0.1, 1.4), ('utt3', wav8, 0, 1.3)])


def synth_corpus(tmp_path, speakers=3, per=3):
    from shennong_amd import synth
    rows = []
    for s in range(speakers):
        for u, w in enumerate(synth.utterances(7 * s, per, nsamples=20000 + 3000 * s)):
            path = str(tmp_path / f's{s}_{u}.wav')
            scipy.io.wavfile.write(path, 16000, w)
            rows.append((f's{s}_u{u}', path, f'spk{s}'))
    return Utterances(rows)


def trained(utts, by_speaker, monkeypatch, device):
    monkeypatch.setattr(vtln_module, '_sweep_on_device', lambda u: device)
    proc = VtlnProcessor(min_warp=0.95, max_warp=1.05, num_iters=2, by_speaker=by_speaker)
    proc.ubm = dict(UBM)
    warps = proc.process(utts)
    return proc, warps


@pytest.mark.parametrize('corpus', ['reference', 'synth'])
@pytest.mark.parametrize('by_speaker', [True, False])
def test_sweep_equals_host_path(gpu, tmp_path, wav_file, monkeypatch, by_speaker, corpus):
    utts = reference_corpus(tmp_path, wav_file, by_speaker) if corpus == 'reference' else synth_corpus(tmp_path)
    if corpus == 'synth' and not by_speaker:
        utts = Utterances([(u.name, u.audio_file) for u in utts])
    old, old_warps = trained(utts, by_speaker, monkeypatch, False)
    new, new_warps = trained(utts, by_speaker, monkeypatch, True)
    assert old.lvtln.num_classes() == new.lvtln.num_classes() == 11
    assert not same_bits(new.lvtln.A[0], new.lvtln.A[10])
    for c in range(old.lvtln.num_classes()):
        assert same_bits(old.lvtln.A[c], new.lvtln.A[c]), c
        assert old.lvtln.get_warp(c) == new.lvtln.get_warp(c)
    assert same_bits(np.asarray(old.lvtln.logdets), np.asarray(new.lvtln.logdets))
    assert old_warps == new_warps
    assert sorted(old.transforms) == sorted(new.transforms)
    for key in old.transforms:
        assert same_bits(old.transforms[key], new.transforms[key]), key


def test_sweep_uploads_the_audio_once(gpu, tmp_path, wav_file):
    """the unwarped pass uploads the audio and downloads its features; the 11 warped passes borrow the audio
    and leave their features in HBM"""
    utts = reference_corpus(tmp_path, wav_file, True)
    features = VtlnProcessor().features
    features.pop('sliding_window_cmvn')
    config = pipeline._init_config(features)
    one = pipeline.RunStats()
    pipeline._extract_features(config, utts, None, pipeline.get_logger('test', 'error'), stats=one)
    assert one.bytes_up > 0 and one.bytes_down > 0
    ubm = DiagUbmProcessor(**UBM)
    ubm.process(utts)
    proc = VtlnProcessor(min_warp=0.95, max_warp=1.05)
    proc.lvtln = LV.LinearVtln(ubm.gmm.dim(), 11, 5)
    stats = pipeline.RunStats()
    orig = proc._base_transforms(utts, ubm, 11, stats=stats)
    assert sorted(orig) == ['utt1', 'utt2', 'utt3']
    assert stats.bytes_up == one.bytes_up
    assert stats.bytes_down == one.bytes_down
    assert stats.batches == 12
    assert all(np.isfinite(a).all() for a in proc.lvtln.A)


def pipeline_config():
    config = pipeline.get_default_config('mfcc', with_cmvn=True, with_delta=True)
    config['mfcc']['dither'] = 0
    vt = VtlnProcessor(min_warp=0.95, max_warp=1.05, num_iters=1)
    vt.ubm = dict(UBM)
    config['vtln'] = vt.get_params()
    return config


def test_extract_features_with_vtln_entry(gpu, tmp_path, wav_file):
    utts = reference_corpus(tmp_path, wav_file, True)
    config = pipeline_config()
    got = pipeline.extract_features(config, utts)
    warps = VtlnProcessor(**config['vtln']).process(utts)
    plain = {k: v for k, v in config.items() if k != 'vtln'}
    want = pipeline.extract_features(plain, utts, warps=warps)
    assert list(got) == list(want)
    for name in want:
        assert same_bits(got[name].data, want[name].data), name
        assert got[name].properties['mfcc']['vtln_warp'] == warps[name]
    # the reference's simple shape, from a YAML string
    text = pipeline._get_config_to_yaml(plain, comments=False) + (
        'vtln:\n  features: default\n  min_warp: 0.95\n  max_warp: 1.05\n  num_iters: 1\n'
        '  ubm:\n    features: default\n    num_gauss: 4\n    num_iters_init: 1\n    num_iters: 1\n'
        '    num_frames: 100\n    vad: {energy_threshold: 0}\n')
    got = pipeline.extract_features(text, utts)
    simple = pipeline._init_config(text)['vtln']
    warps = VtlnProcessor(**simple).process(utts)
    want = pipeline.extract_features(plain, utts, warps=warps)
    for name in want:
        assert same_bits(got[name].data, want[name].data), name


def test_extract_features_streamed_with_vtln_entry(gpu, tmp_path, wav_file):
    utts = synth_corpus(tmp_path)
    config = pipeline_config()
    got = {}
    n = pipeline.extract_features_streamed(config, utts, got.update, max_batch_duration=2.0)
    assert n == len(utts)
    warps = VtlnProcessor(**config['vtln']).process(utts)
    plain = {k: v for k, v in config.items() if k != 'vtln'}
    want = pipeline.extract_features(plain, utts, warps=warps)
    assert sorted(got) == sorted(want)
    for name in want:
        assert same_bits(got[name].data, want[name].data), name
