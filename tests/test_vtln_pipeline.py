"""Host logic of VTLN training through the pipeline configuration (a 'vtln' entry), with the device pipeline
and the trainer replaced by stand-ins: configuration handling, training exactly once, the refusals, and the
row list of the device-resident mapping sweep"""

import logging
import os

import numpy as np
import pytest
import yaml

from conftest import GOLDEN
from shennong_amd import Utterances, distributed, pipeline
from shennong_amd.features import Features, FeaturesCollection
from shennong_amd.logger import get_logger
from shennong_amd.processor import vtln as vtln_module
from shennong_amd.processor.vtln import VtlnProcessor

WAV = os.path.join(GOLDEN, 'test.wav')

SIMPLE_YAML = '''
mfcc:
  num_ceps: 13
  dither: 0
vtln:
  by_speaker: true
  features: default
  logdet_scale: 0.0
  max_warp: 1.25
  min_warp: 0.85
  norm_type: offset
  num_iters: 15
  subsample: 5
  warp_step: 0.01
  ubm:
    features: default
    num_gauss: 64
    num_iters: 4
    num_iters_init: 20
'''


@pytest.fixture()
def utterances():
    return Utterances([('utt1', WAV, 'spk1'), ('utt2', WAV, 'spk1'), ('utt3', WAV, 'spk2')])


def vtln_config(features='mfcc'):
    config = pipeline.get_default_config(features)
    config['vtln'] = VtlnProcessor(min_warp=0.95, max_warp=1.05, ubm={'num_gauss': 4}).get_params()
    return config


@pytest.mark.parametrize('features', ['mfcc', 'filterbank', 'plp'])
def test_init_config_accepts_vtln(features, capsys):
    log = get_logger('test', 'info')
    config = pipeline._init_config(vtln_config(features), log=log)
    assert 'vtln' in config and features in config
    assert 'with vtln by speaker' in capsys.readouterr().err
    config = vtln_config(features)
    config['vtln']['by_speaker'] = False
    pipeline._init_config(config, log=log)
    assert 'with vtln by utterance' in capsys.readouterr().err


def test_init_config_refuses_vtln_with_spectrogram():
    with pytest.raises(ValueError, match='spectrogram features do not support VTLN'):
        pipeline._init_config(vtln_config('spectrogram'))


def test_reference_simple_yaml(tmp_path):
    """the 'simple' shape the reference's config command writes: features: default under vtln and vtln.ubm"""
    for source in (SIMPLE_YAML, str(tmp_path / 'config.yaml')):
        (tmp_path / 'config.yaml').write_text(SIMPLE_YAML)
        config = pipeline._init_config(source)
        assert config['vtln']['features'] == 'default'
        assert config['vtln']['ubm']['features'] == 'default'
        proc = VtlnProcessor(**config['vtln'])
        assert 'mfcc' in proc.features and 'sliding_window_cmvn' in proc.features
        assert proc.ubm['num_gauss'] == 64
    # a full entry, as get_params() gives it, goes through YAML and back
    config = vtln_config()
    text = yaml.safe_dump(yaml.safe_load(pipeline._get_config_to_yaml(config, comments=False)))
    assert pipeline._init_config(text)['vtln']['ubm']['num_gauss'] == 4


def test_vtln_entry_and_warps_refused(utterances):
    for run in (lambda c, w: pipeline.extract_features(c, utterances, warps=w),
                lambda c, w: pipeline.extract_features_streamed(c, utterances, lambda f: None, warps=w)):
        with pytest.raises(ValueError) as err:
            run(vtln_config(), {'utt1': 1.0, 'utt2': 1.0, 'utt3': 1.0})
        assert 'warps are given but "vtln" processor already defined in the configuration' in str(err.value)


def test_vtln_entry_bad_keys(utterances):
    config = vtln_config()
    config['vtln']['bad_key'] = 1
    with pytest.raises(TypeError):
        pipeline.extract_features(config, utterances)


@pytest.fixture()
def stand_ins(monkeypatch):
    """VtlnProcessor.process and the device pipeline replaced: records the training calls (with the log level
    of the processor) and the warps / configuration every extraction gets"""
    record = {'train': [], 'extract': []}

    def process(self, utterances, ubm=None, group_by='utterance', njobs=1):
        record['train'].append((self.log.getEffectiveLevel(), self.min_warp, njobs))
        return {u.name: 0.9 + 0.01 * i for i, u in enumerate(utterances)}

    def fake(config, utterances, warps, log, tolerance=2, stats_hook=None, stats_only=False, **kwargs):
        utts = list(utterances)
        if stats_only:
            return [u.speaker for u in utts], np.ones((len(utts), 2, 3))
        record['extract'].append((sorted(config), dict(warps) if warps else None, [u.name for u in utts]))
        out = FeaturesCollection({u.name: Features(np.full((2, 3), warps[u.name] if warps else 1.0, np.float32),
                                                   np.arange(2) * 0.01) for u in utts})
        return (out, lambda: None) if kwargs.get('defer') else out

    monkeypatch.setattr(VtlnProcessor, 'process', process)
    monkeypatch.setattr(pipeline, '_extract_features', fake)
    return record


@pytest.mark.parametrize('too_large', [False, True])
def test_extract_features_trains_once(utterances, stand_ins, monkeypatch, too_large):
    if too_large:
        monkeypatch.setattr(pipeline, '_too_large_for_one_batch', lambda u: True)
        monkeypatch.setattr(pipeline, 'default_batch_duration', lambda depth=1: 1.0)
    want = {'utt1': 0.9, 'utt2': 0.91, 'utt3': 0.92}
    got = pipeline.extract_features(vtln_config(), utterances, log=get_logger('test', 'debug'))
    assert stand_ins['train'] == [(logging.DEBUG, 0.95, 1)]
    assert stand_ins['extract'] and all(keys == ['mfcc'] and warps == {n: want[n] for n in names}
                                        for keys, warps, names in stand_ins['extract'])
    assert [n for _, _, names in stand_ins['extract'] for n in names] == ['utt1', 'utt2', 'utt3']
    assert {n: float(f.data[0, 0]) for n, f in got.items()} == pytest.approx(want)


def test_extract_features_streamed_trains_once(utterances, stand_ins):
    out = {}
    config = vtln_config()
    config['cmvn'] = {'by_speaker': True, 'with_vad': True}
    n = pipeline.extract_features_streamed(config, utterances, out.update, max_batch_duration=1.0, njobs=2,
                                           log=get_logger('test', 'error'))
    assert n == 3 and sorted(out) == ['utt1', 'utt2', 'utt3']
    assert stand_ins['train'] == [(logging.ERROR, 0.95, 2)]
    assert all(keys == ['cmvn', 'mfcc'] for keys, _, _ in stand_ins['extract'])
    assert float(out['utt3'].data[0, 0]) == pytest.approx(0.92)


def test_sharded_entry_points_refuse_vtln(utterances, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for run in (lambda c: distributed.extract_features_sharded(c, utterances),
                lambda c: distributed.extract_features_streamed_sharded(c, utterances, lambda f: None)):
        with pytest.raises(ValueError) as err:
            run(vtln_config())
        assert 'sharded pipeline' in str(err.value) and 'precomputed warps' in str(err.value)


def test_get_default_config_with_vtln_still_refused():
    for with_vtln in ('simple', 'full'):
        with pytest.raises(ValueError, match='not available in this backend'):
            pipeline.get_default_config('mfcc', with_vtln=with_vtln)


@pytest.mark.parametrize('subsample', [1, 3, 5, 50])
def test_sweep_rows_equal_trim_then_subsample(subsample):
    """the (block, row) list of the device sweep gathers the rows trim(vad) + [::subsample] keeps, in order:
    two blocks (two sample rates, the utterances interleaved), all-false masks, fewer kept rows than the step"""
    rng = np.random.RandomState(subsample)
    lengths = [40, 7, 0, 25, 3, 60, 12]
    rate_of = [0, 1, 0, 1, 1, 0, 1]
    names = [f'u{i}' for i in range(len(lengths))]
    feats = {n: rng.randn(m, 4).astype(np.float32) for n, m in zip(names, lengths)}
    vad = {n: rng.rand(m) < 0.6 for n, m in zip(names, lengths)}
    vad['u1'][:] = False
    vad['u4'][:] = [False, True, False]
    # blocks as the device pipeline lays them out: one per rate, the utterances of that rate in index order
    blocks, layout = [], {}
    for b in (0, 1):
        mine = [n for n, r in zip(names, rate_of) if r == b]
        first = np.concatenate([[0], np.cumsum([lengths[names.index(n)] for n in mine])])
        for n, f in zip(mine, first):
            layout[n] = (b, int(f))
        blocks.append(np.concatenate([feats[n] for n in mine]))
    block, row = vtln_module.sweep_rows(names, vad, subsample, layout)
    assert block.dtype == np.int32 and row.dtype == np.int64
    gathered = np.stack([blocks[b][r] for b, r in zip(block, row)]) if block.size else np.zeros((0, 4))
    coll = FeaturesCollection({n: Features(feats[n], np.arange(len(feats[n])) * 0.01, validate=False)
                               for n in names})
    trimmed = coll.trim(vad)
    want = np.concatenate([trimmed[n].data[::subsample] for n in names])
    np.testing.assert_array_equal(gathered, want)
    assert vtln_module.sweep_rows([], {}, subsample, {})[0].size == 0


def test_sweep_waves_lend_without_giving_back():
    class Buffer:
        def __init__(self, nbytes):
            self.nbytes, self.ptr, self.device, self.freed = nbytes, 1234, 0, 0

        def free(self, synced=False):
            self.freed += 1

    waves = pipeline._SweepWaves()
    assert waves.every_pass and not pipeline._ResidentWaves(10).every_pass
    a = Buffer(100)
    assert waves.offer((None, 16000), a, 'soff')
    for _ in range(3):   # every later pass borrows the same block
        lent, soff = waves.take((None, 16000))
        assert lent.ptr == a.ptr and soff == 'soff'
        lent.free()
        lent.free(synced=True)
        assert not waves.offer((None, 16000), lent, 'soff')
    assert a.freed == 0 and waves.take((None, 8000)) is None
    waves.clear()
    assert a.freed == 1 and waves.take((None, 16000)) is None
