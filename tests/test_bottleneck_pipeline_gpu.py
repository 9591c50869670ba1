"""Bottleneck features as a pipeline entry, on the device: the one-call extractor (``snf_bottleneck_extract``)
against the staged calls, its status word, and ``extract_features`` / ``extract_features_streamed`` / the by-stage
path / the sharded driver against the composition of the public processors - everything bit for bit (the
corpora and what makes that valid: tests/test_bottleneck_pipeline.py::test_gpu_corpus_conditions).

Synthetic weights of hidden width 96 (``write_weights`` of tests/test_bottleneck.py), utterances of 0.35 to 1.05 s.
Every step on the device runs under its own time limit (the guard of tests/test_crepe_gpu.py)."""

import numpy as np
import pytest

from shennong_amd import Audio, Utterances, pipeline
from shennong_amd.logger import get_logger
from shennong_amd.utils import dict_equal
from test_bottleneck import write_weights
from test_bottleneck_pipeline import HIDDEN, bottleneck_config, corpus, ragged, silent
from test_crepe_gpu import on_device

pytestmark = pytest.mark.gpu
QUIET = get_logger('test', 'error')


def install(directory, monkeypatch, context=5, seed=41, **replace):
    """Synthetic weights in `directory`, found by the processors the pipeline makes"""
    directory.mkdir(exist_ok=True)
    monkeypatch.setenv('SHENNONG_AMD_BOTTLENECK_DIR', str(directory))
    write_weights(directory, 'BabelMulti', seed=seed, hidden=HIDDEN, context=context, **replace)


def processor(dither=0.0):
    from shennong_amd.processor import BottleneckProcessor
    return BottleneckProcessor(weights='BabelMulti', dither=dither)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    assert np.array_equal(bits(got), bits(want)), what


def pitch_entry():
    entry = pipeline.get_default_config('mfcc', with_pitch='kaldi')['pitch']
    entry['postprocessing']['delta_pitch_noise_stddev'] = 0
    return entry


# ---- 1. the entry point ---------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['float32', 'bfloat16'])
@pytest.mark.parametrize('dither', [0.0, 0.1])
@pytest.mark.parametrize('context', [5, 6])
def test_extract_equals_the_staged_calls(gpu, tmp_path, monkeypatch, context, dither, precision):
    """Seven ragged utterances: default scratch and rows end to end; then a bound that cuts the batch into runs
    of two and a last run of one, the rows written through offsets with gaps (and two pairs without) into a
    larger block whose other rows must stay as they were"""
    from shennong_amd import _backend
    from shennong_amd.processor import bottleneck
    install(tmp_path, monkeypatch, context)
    proc = processor(dither)
    waves = ragged()
    batch = bottleneck.BottleneckBatch(waves)
    dnet = proc._device_network(batch.device)
    with on_device():
        voiced = batch.vad()
        batch.fbank(dither)
        want = batch.forward(dnet, precision)
    assert voiced.min() > 0 and np.isfinite(want).all()
    with on_device():
        out, ooff, status = batch.extract(dnet, dither, precision)
        got = out.download(np.empty((int(ooff[-1]), 80), dtype=np.float32))
    assert np.array_equal(ooff, batch.ooff) and np.array_equal(np.diff(ooff), batch.rows(context))
    assert status.dtype == np.int32 and not status.any()
    same_bits(got, want, 'default scratch')

    # two hidden buffers of one tile of 128 rows, 4 kB of rounding, and room for two of these utterances
    # (51 to 61 kB each), not three
    bound = 2 * 128 * HIDDEN * 4 + 4096 + 125000
    assert batch.runs(dnet, bound).tolist() == [0, 2, 4, 6, 7] and batch.runs(dnet).tolist() == [0, 7]
    rows = batch.rows(context)
    gaps = [2, 0, 3, 0, 0, 1, 4]
    offsets = np.zeros(8, dtype=np.int64)
    offsets[0] = 3
    for u in range(7):
        offsets[u + 1] = offsets[u] + rows[u] + gaps[u]
    total = int(offsets[-1]) + 5
    fill = np.full((total, 80), -7.25, dtype=np.float32)
    block = _backend.DeviceBuffer(fill.nbytes)
    block.upload(fill)
    with on_device():
        _, _, status = batch.extract(dnet, dither, precision, out=block, out_offsets=offsets, scratch_bytes=bound)
        host = block.download(np.empty_like(fill))
    assert not status.any()
    untouched = np.ones(total, dtype=bool)
    for u in range(7):
        a = int(offsets[u])
        same_bits(host[a:a + rows[u]], want[ooff[u]:ooff[u + 1]], f'bounded scratch, utterance {u}')
        untouched[a:a + rows[u]] = False
    assert untouched.sum() == 3 + sum(gaps) + 5 and np.array_equal(host[untouched], fill[untouched])


def test_extract_refuses_like_the_staged_calls(gpu, tmp_path, monkeypatch):
    from shennong_amd import _backend
    from shennong_amd.processor import bottleneck
    install(tmp_path, monkeypatch)
    batch = bottleneck.BottleneckBatch(ragged(2) + [np.zeros(150, dtype=np.int16)])
    dnet = processor()._device_network(batch.device)
    with pytest.raises(ValueError, match='utterance 2 has 0 frames, too few for one row at context 5'):
        batch.extract(dnet)
    batch = bottleneck.BottleneckBatch(ragged(2))
    with pytest.raises(ValueError, match='output offsets leave utterance 1 fewer than its'):
        batch.extract(dnet, out_offsets=np.array([0, batch.rows(5)[0], batch.rows(5).sum() - 1]))
    with pytest.raises(ValueError, match='dither must be >= 0'):
        batch.extract(dnet, dither=-1.0)
    L, p = _backend.lib(), 256
    assert L.snf_bottleneck_extract(0, p, None, 1, p, 0.0, 0, 5, p, dnet.widths, dnet.pointers, 0, p, None, None, 0,
                                    None) == -1
    assert b'null sample offsets table' in L.snf_last_error()


# ---- 2. the status word -----------------------------------------------------------------------------------
def test_status_of_a_silent_utterance(gpu, tmp_path, monkeypatch):
    from shennong_amd.processor import bottleneck
    install(tmp_path, monkeypatch)
    proc = processor()
    waves = ragged(2)
    batch = bottleneck.BottleneckBatch([waves[0], silent().data, waves[1]])
    with on_device():
        out, ooff, status = batch.extract(proc._device_network(batch.device))
        got = out.download(np.empty((int(ooff[-1]), 80), dtype=np.float32))
    assert status.tolist() == [0, 1, 0]
    assert np.isfinite(got).all()   # (an utterance without voiced frames has a zero mean: defined rows)
    with pytest.raises(RuntimeError) as err:
        bottleneck.raise_for_status(status, ['a', 'quiet', 'b'])
    assert str(err.value) == 'no voice detected in signal "quiet", failed to extract features'
    utts = Utterances([('a', Audio(waves[0], 8000)), ('quiet', silent()), ('b', Audio(waves[1], 8000))])
    with pytest.raises(RuntimeError) as processors:
        with on_device():
            proc.process_all(utts)
    with pytest.raises(RuntimeError) as piped:
        with on_device():
            pipeline.extract_features(bottleneck_config(), utts, log=QUIET)
    assert str(piped.value) == str(processors.value) == str(err.value)


def test_status_of_values_that_are_not_finite(gpu, tmp_path, monkeypatch):
    """Finite weights whose last layer overflows float32: 96 sigmoid outputs times 3e38"""
    from shennong_amd.processor import bottleneck
    install(tmp_path, monkeypatch, W7=np.full((HIDDEN, 80), 3e38), b7=np.full(80, 3e38))
    proc = processor()
    waves = ragged(2)
    batch = bottleneck.BottleneckBatch(waves)
    with on_device():
        status = batch.extract(proc._device_network(batch.device))[2]
    assert status.tolist() == [2, 2]
    utts = Utterances([('a', Audio(waves[0], 8000)), ('b', Audio(waves[1], 8000))])
    with pytest.raises(ValueError) as processors:
        with on_device():
            proc.process_all(utts)
    with pytest.raises(ValueError) as piped:
        with on_device():
            pipeline.extract_features(bottleneck_config(), utts, log=QUIET)
    assert str(piped.value) == str(processors.value) == 'data contains non-finite numbers (nan of infinity)'


def test_too_short_is_refused_before_any_launch(gpu, tmp_path, monkeypatch):
    """300 samples at 16 kHz are 150 at 8 kHz: no frame.  The processor's message with the name, and no GPU time
    counted - not even the resampler of the group it belongs to"""
    from shennong_amd import _backend
    install(tmp_path, monkeypatch)
    assert _backend.resample_num_out(16000, 8000, 300) == 150
    items = [(name, audio) for name, audio, _ in corpus()]
    items.append(('short', Audio(np.zeros(300, dtype=np.int16), 16000)))
    proc = processor()
    proc.resample = 'kaldi'
    with pytest.raises(ValueError) as processors:
        proc.process_all(Utterances(items))
    assert str(processors.value) == \
        'signal "short" too short: 150 samples at 8 kHz give 0 frames, one row of features needs 1'
    stats = pipeline.RunStats()
    with pytest.raises(ValueError) as piped:
        with on_device():
            pipeline.extract_features_streamed(bottleneck_config(), Utterances(items), lambda feats: None,
                                               stats=stats, log=QUIET)
    assert str(piped.value) == str(processors.value)
    assert stats.gpu_ms == 0 and stats.batches == 0 and stats.bytes_up > 0


# ---- 3. the pipeline is the composition -----------------------------------------------------------------
def by_hand(config, items):
    """audio.astype(int16).resample(8000, backend='kaldi') for the utterances that are not at 8 kHz ->
    BottleneckProcessor (resample = 'kaldi' recorded where due) -> CmvnPostProcessor (weights: EnergyProcessor ->
    VadPostProcessor on the 8 kHz audio) -> DeltaPostProcessor -> concatenation with Kaldi pitch of the 8 kHz audio"""
    from shennong_amd.postprocessor import CmvnPostProcessor, DeltaPostProcessor, VadPostProcessor
    from shennong_amd.processor import EnergyProcessor, KaldiPitchPostProcessor, KaldiPitchProcessor
    feats, audios = {}, {}
    for name, audio, _ in items:
        proc = processor(config['bottleneck']['dither'])
        if audio.sample_rate != 8000:
            audio = audio.astype(np.int16).resample(8000, backend='kaldi')
            proc.resample = 'kaldi'
        assert audio.sample_rate == 8000 and audio.dtype == np.int16
        audios[name], feats[name] = audio, proc.process(audio)
    if 'cmvn' in config:
        group = {name: (speaker if config['cmvn']['by_speaker'] else name) for name, _, speaker in items}
        cmvn = {g: CmvnPostProcessor(80) for g in group.values()}
        for name, _, _ in items:
            weights = None
            if config['cmvn']['with_vad']:
                energy = EnergyProcessor(sample_rate=8000, frame_shift=0.01, frame_length=0.025)
                weights = VadPostProcessor(**config['cmvn']['vad']).process(energy.process(audios[name])).data[:, 0]
            cmvn[group[name]].accumulate(feats[name], weights=weights)
        feats = {name: cmvn[group[name]].process(f) for name, f in feats.items()}
    if 'delta' in config:
        feats = {name: DeltaPostProcessor(**config['delta']).process(f) for name, f in feats.items()}
    if 'pitch' in config:
        params = {k: v for k, v in config['pitch'].items() if k not in ('processor', 'postprocessing')}
        for name in feats:
            raw = KaldiPitchProcessor(sample_rate=8000, frame_shift=0.01, frame_length=0.025, **params).process(
                audios[name])
            post = KaldiPitchPostProcessor(**config['pitch']['postprocessing']).process(raw)
            feats[name] = feats[name].concatenate(post, tolerance=2)
    return feats


ENTRIES = {
    'alone': ({}, [('bottleneck', 80)]),
    'delta': ({'delta': pipeline._processor_params('delta')}, [('bottleneck', 80), ('delta', 240)]),
    'cmvn by utterance': ({'cmvn': {'by_speaker': False, 'with_vad': False}}, [('bottleneck', 80), ('cmvn', 80)]),
    'cmvn by speaker with vad': ({'cmvn': {'by_speaker': True, 'with_vad': True,
                                           'vad': pipeline._processor_params('vad')}},
                                 [('bottleneck', 80), ('cmvn', 80)]),
    'pitch': ({'pitch': pitch_entry()}, [('bottleneck', 80), ('pitch', 83)]),
}


@pytest.mark.parametrize('entries', sorted(ENTRIES))
def test_extract_features_is_the_composition(gpu, tmp_path, monkeypatch, entries):
    install(tmp_path, monkeypatch)
    extra, stages = ENTRIES[entries]
    config = bottleneck_config(**extra)
    items = corpus()
    with on_device():
        got = pipeline.extract_features(config, Utterances(items), log=QUIET)
    with on_device():
        want = by_hand(pipeline._init_config(config, log=QUIET), items)
    assert list(got.keys()) == ['u0', 'u1', 'u2']
    for name, audio, speaker in items:
        g, w = got[name], want[name]
        same_bits(g.data, w.data, f'{entries}: {name}')
        assert g.shape == (w.shape[0], stages[-1][1]) and g.shape[0] in (102, 58, 61)
        assert np.array_equal(g.times, w.times), name
        assert g.properties['audio']['sample_rate'] == 8000 and g.properties['speaker'] == speaker
        expected = {'weights': 'BabelMulti', 'dither': 0.0}
        if audio.sample_rate != 8000:
            expected['resample'] = 'kaldi'
        assert g.properties['bottleneck'] == expected, name
        columns = [(s['name'], s['columns'][1] + 1) for s in g.properties['pipeline']]
        assert columns == stages and g.properties['pipeline'][0]['columns'] == [0, 79]
        assert dict_equal({k: v for k, v in g.properties.items() if k not in ('audio', 'speaker')}, w.properties), name
        if 'pitch' in extra:
            assert g.properties['pitch']['sample_rate'] == 8000


# ---- 4. a context that is not 5 ---------------------------------------------------------------------------
def test_context_six(gpu, tmp_path, monkeypatch):
    """Rows = frames - 2: the pitch join trims within its tolerance of 2, and VAD weights (one per frame) do not fit"""
    install(tmp_path, monkeypatch, context=6)
    items = corpus()
    config = bottleneck_config(pitch=pitch_entry())
    with on_device():
        got = pipeline.extract_features(config, Utterances(items), log=QUIET)
    with on_device():
        want = by_hand(pipeline._init_config(config, log=QUIET), items)
    for name, frames in (('u0', 102), ('u1', 58), ('u2', 61)):
        assert got[name].shape == (frames - 2, 83), name
        same_bits(got[name].data, want[name].data, name)
        assert np.array_equal(got[name].times, want[name].times), name
    config = bottleneck_config(cmvn={'by_speaker': False, 'with_vad': True, 'vad': pipeline._processor_params('vad')})
    with pytest.raises(ValueError) as err:
        with on_device():
            pipeline.extract_features(config, Utterances(items[1:2]), log=QUIET)
    assert str(err.value) == 'there is 58 weights but 56 feature frames, must be equal'
    with pytest.raises(ValueError) as staged:
        with on_device():
            pipeline._extract_features_by_stage(pipeline._init_config(config, log=QUIET), Utterances(items[1:2]),
                                                None, QUIET)
    assert str(staged.value) == str(err.value)


# ---- 5. the other execution paths -------------------------------------------------------------------------
def test_other_paths_give_the_one_shot_bits(gpu, tmp_path, monkeypatch):
    from shennong_amd import distributed
    from shennong_amd.comm import RcclComm
    install(tmp_path, monkeypatch)
    config = bottleneck_config(cmvn={'by_speaker': True, 'with_vad': False}, delta=pipeline._processor_params('delta'))
    utts = Utterances(corpus())
    assert utts.duration() > 1.7 > max(u.duration for u in utts)
    batches, stats = [], pipeline.RunStats()
    with on_device():
        want = pipeline.extract_features(config, utts, log=QUIET)
    with on_device():
        # (two batches, CMVN by speaker: the second pass starts from the 8 kHz blocks the first one left in HBM)
        pipeline.extract_features_streamed(config, utts, batches.append, max_batch_duration=1.7, stats=stats,
                                           log=QUIET)
    assert [len(b) for b in batches] == [2, 1]
    streamed = {name: feats for batch in batches for name, feats in batch.items()}
    # one upload per utterance at its own rate: 16643 + 4815 + 9999 int16 samples, nothing in the second pass
    assert stats.bytes_up == 2 * (16643 + 4815 + 9999)
    with on_device():
        staged = pipeline._extract_features_by_stage(pipeline._init_config(config, log=QUIET), utts, None, QUIET)
    with on_device():
        comm = RcclComm(0, 1)
        try:
            sharded = distributed.extract_features_sharded(config, utts, group=comm, log=QUIET)
        finally:
            comm.close()
    for path, got in (('streamed', streamed), ('by stage', staged), ('sharded', sharded)):
        assert sorted(got.keys()) == sorted(want.keys()), path
        for name in want.keys():
            same_bits(got[name].data, want[name].data, f'{path}: {name}')
            assert np.array_equal(got[name].times, want[name].times), (path, name)
            assert dict_equal(got[name].properties, want[name].properties), (path, name)


# ---- 6. dither ----------------------------------------------------------------------------------------------
def test_dithered_utterance_alone_and_in_the_batch(gpu, tmp_path, monkeypatch):
    install(tmp_path, monkeypatch)
    config = bottleneck_config(0.1)
    items = corpus()
    with on_device():
        together = pipeline.extract_features(config, Utterances(items), log=QUIET)
        clean = pipeline.extract_features(bottleneck_config(0.0), Utterances(items), log=QUIET)
    for item in items:
        with on_device():
            alone = pipeline.extract_features(config, Utterances([item]), log=QUIET)
        same_bits(alone[item[0]].data, together[item[0]].data, item[0])
        assert not np.array_equal(together[item[0]].data, clean[item[0]].data)
        assert together[item[0]].properties['bottleneck']['dither'] == 0.1
