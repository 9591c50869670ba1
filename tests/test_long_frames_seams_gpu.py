"""The long-frame kernels (fbank1024x2_kernel, fbank2048_kernel) on every trip of their grid-stride walk and on
every seam of their window and bank ladders, against the CPU oracle at the tolerance of every long-frame test
(conftest.assert_close, rtol 1e-4), and bit for bit where the project promises batch independence.  The batches
and the host mirror of the walk: tests/long_frame_cases.py; where their features lie is proved without a GPU
by tests/test_long_frame_cases.py."""

import functools

import numpy as np
import pytest

import long_frame_cases as lf
from conftest import FAMILY_ATOL, assert_close, family_of
from oracle import oracle as orc
from shennong_amd import Audio, _backend
from shennong_amd.processor import FilterbankProcessor, MfccProcessor, PlpProcessor, SpectrogramProcessor

pytestmark = pytest.mark.gpu

KINDS = {'fbank40': (FilterbankProcessor, dict(num_bins=40)), 'mfcc': (MfccProcessor, dict()),
         'spectrogram': (SpectrogramProcessor, dict()), 'plp': (PlpProcessor, dict())}
PAIRED, LONG = 'fbank1024x2_kernel', 'fbank2048_kernel'
VALUE_CASES = ([(PAIRED, rate, kind) for rate in (22050, 32000) for kind in ('fbank40', 'mfcc', 'spectrogram')]
               + [(LONG, 44100, kind) for kind in ('mfcc', 'fbank40')])


def _proc(kind, sample_rate, snip_edges, **more):
    cls, opts = KINDS[kind]
    return cls(sample_rate=sample_rate, snip_edges=snip_edges, **dict(dict(dither=0, **opts), **more))


def _run(proc, waves, warps, sample_rate):
    kw = {} if isinstance(proc, SpectrogramProcessor) else dict(vtln_warp=warps)
    return [f.data for f in proc._process_batch([Audio(w, sample_rate) for w in waves], **kw)]


def _kernel(proc):
    return _backend.get_plan(proc._build_options()).kernel_name(1)


def _oracle(proc, wave, warp):
    warp = 1.0 if isinstance(proc, SpectrogramProcessor) else warp
    return orc.compute(proc._build_options(), np.asarray(wave, np.int16), warp)


@functools.lru_cache(maxsize=None)
def _wants(kind, sample_rate, snip_edges):
    """the oracle's features of every utterance of the multi-trip batch: computed once, read by every test"""
    waves, warps = lf.multi_trip_batch(sample_rate, snip_edges)
    proc = _proc(kind, sample_rate, snip_edges)
    wants = [_oracle(proc, w, wf) for w, wf in zip(waves, warps)]
    for want in wants:
        want.setflags(write=False)
    return wants


def _worst_row(got, want, what, rtol=1e-4):
    """the row of an utterance that exceeds assert_close's bound by most"""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = FAMILY_ATOL[family_of(what)] + rtol * np.abs(want.astype(np.float64))
    return int((err / bound).max(axis=1).argmax())


def _assert_every_utterance(gots, wants, what, waves, sample_rate, snip_edges):
    """assert_close of every utterance; a failure names the trip of the worst frame and counts the failing
    utterances by trip"""
    trips = lf.row_trips(waves, sample_rate, snip_edges)
    first = np.concatenate([[0], np.cumsum(lf.frame_counts(waves, sample_rate, snip_edges))])
    labels = lf.batch_labels(sample_rate, snip_edges)
    failures = []
    for u, (got, want) in enumerate(zip(gots, wants)):
        assert got.shape == want.shape, (what, u, got.shape, want.shape)
        try:
            assert_close(got, want, rtol=1e-4, what=what)
        except AssertionError as error:
            row = _worst_row(got, want, what)
            failures.append((u, labels[u], row, int(trips[first[u] + row]), str(error).strip().splitlines()[:4]))
    if failures:
        by_trip = np.bincount([f[3] + 1 for f in failures], minlength=4).tolist()
        u, label, row, trip, text = failures[0]
        raise AssertionError(
            '%s: %d of %d utterances outside the bound; their worst frames by trip (generic kernel, 0, 1, 2): %s; '
            'the first: utterance %d (%s), frame %d, written on trip %d: %s'
            % (what, len(failures), len(gots), by_trip, u, label, row, trip, ' '.join(text)))


# ---- 2. the trips ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('snip_edges', [True, False])
@pytest.mark.parametrize('kernel, sample_rate, kind', VALUE_CASES)
def test_values_on_every_trip(gpu, kernel, sample_rate, kind, snip_edges):
    """one call over 8192 < n < 12288 pairs (frames): every wave hands its pipeline state over once or twice,
    the look-ahead of the last two trips is clamped to the last record, single frames, split pairs and
    reflected replays come up on the later trips with other warps than the trip before"""
    waves, warps = lf.multi_trip_batch(sample_rate, snip_edges)
    proc = _proc(kind, sample_rate, snip_edges)
    gots = _run(proc, waves, warps, sample_rate)
    assert _kernel(proc) == kernel
    _assert_every_utterance(gots, _wants(kind, sample_rate, snip_edges), '%s %d Hz snip_edges %s' % (
        proc.name, sample_rate, snip_edges), waves, sample_rate, snip_edges)


def plp_without_silent_frames(gots, wants):
    """The cepstra of a frame of digital silence are NaN in the reference (all-zero mel energies: the Durbin
    recursion divides 0 by 0; the energy column stays finite), so they must be on the device, in the same rows.
    -> copies of both with those rows zeroed, for assert_close"""
    out = [], []
    for u, (got, want) in enumerate(zip(gots, wants)):
        silent = ~np.isfinite(want).all(axis=1)
        assert got.shape == want.shape
        assert np.array_equal(~np.isfinite(got).all(axis=1), silent), (
            'utterance %d: rows with non-finite numbers %s, the oracle has them in %s'
            % (u, np.nonzero(~np.isfinite(got).all(axis=1))[0].tolist(), np.nonzero(silent)[0].tolist()))
        for side, data in zip(out, (got, want)):
            data = data.copy()
            data[silent] = 0
            side.append(data)
    return out


@pytest.mark.parametrize('snip_edges', [True, False])
def test_plp_rows_and_energies_from_later_trips(gpu, snip_edges):
    """PLP: the kernel writes linear mel rows and `energy_out` for plp_tail_kernel, from every trip.  Two signals
    of the batch hold digital silence, whose PLP cepstra are NaN in the reference: the public call refuses the
    batch as the reference's Features.validate would, the plan's own call returns it"""
    waves, warps = lf.multi_trip_batch(32000, snip_edges)
    proc = _proc('plp', 32000, snip_edges)
    wants = _wants('plp', 32000, snip_edges)
    labels = lf.batch_labels(32000, snip_edges)
    assert {labels[u] for u, want in enumerate(wants) if not np.isfinite(want).all()} == {'unequal0', 'unequal3'}
    with pytest.raises(ValueError, match='non-finite'):
        _run(proc, waves, warps, 32000)
    gots = _backend.get_plan(proc._build_options()).run(waves, warps, check_finite=False)
    assert _kernel(proc) == PAIRED
    gots, wants = plp_without_silent_frames(gots, wants)
    _assert_every_utterance(gots, wants, '%s 32000 Hz snip_edges %s' % (proc.name, snip_edges), waves, 32000,
                            snip_edges)


@pytest.mark.parametrize('snip_edges', [True, False])
@pytest.mark.parametrize('kernel, sample_rate, kind', VALUE_CASES)
def test_bits_alone_and_on_a_later_trip(gpu, kernel, sample_rate, kind, snip_edges):
    """an utterance alone runs on trip 0 of wave 0 ...; inside the batch the same utterance lies on trip 1 or 2
    of some other wave, and after a rotation of the batch by a third on another trip of yet another wave
    (tests/test_long_frame_cases.py): the same bits every time"""
    waves, warps = lf.multi_trip_batch(sample_rate, snip_edges)
    proc = _proc(kind, sample_rate, snip_edges)
    picked = lf.probes(sample_rate, snip_edges)
    alone = {i: _run(proc, [waves[i]], [warps[i]], sample_rate)[0] for i in picked}
    together = _run(proc, waves, warps, sample_rate)
    assert _kernel(proc) == kernel
    order = lf.rotated(list(range(len(waves))), len(waves) // 3)
    turned = _run(proc, [waves[i] for i in order], [warps[i] for i in order], sample_rate)
    labels = lf.batch_labels(sample_rate, snip_edges)
    for i in picked:
        assert alone[i].shape[0] > 0
        assert np.array_equal(alone[i], together[i]), '%s: utterance %d (%s) alone / in the batch' % (
            proc.name, i, labels[i])
        assert np.array_equal(alone[i], turned[order.index(i)]), '%s: utterance %d (%s) alone / rotated' % (
            proc.name, i, labels[i])


@pytest.mark.parametrize('snip_edges', [True, False])
@pytest.mark.parametrize('kernel, sample_rate, kind', [(PAIRED, 22050, 'fbank40'), (PAIRED, 32000, 'mfcc'),
                                                       (LONG, 44100, 'mfcc')])
def test_default_dither_on_a_later_trip(gpu, kernel, sample_rate, kind, snip_edges):
    """dither = 1.0 (the default): the noise of a frame is keyed by its utterance and its index inside it, not
    by the trip or the wave that takes it - alone == in the batch, bit for bit (a fresh plan per call: the same
    call count, as test_default_dither_does_not_depend_on_the_batch)"""
    waves, warps = lf.multi_trip_batch(sample_rate, snip_edges)
    cls, opts = KINDS[kind]
    proc = cls(sample_rate=sample_rate, snip_edges=snip_edges, **opts)
    assert proc.dither == 1.0

    def fresh(ws, wfs):
        _backend.clear_plans()
        return _run(proc, ws, wfs, sample_rate)
    picked = lf.probes(sample_rate, snip_edges)
    alone = {i: fresh([waves[i]], [warps[i]])[0] for i in picked}
    together = fresh(waves, warps)
    assert _kernel(proc) == kernel
    labels = lf.batch_labels(sample_rate, snip_edges)
    for i in picked:
        assert np.array_equal(alone[i], together[i]), '%s: utterance %d (%s)' % (proc.name, i, labels[i])
    # (the noise is there: other bits than without it)
    quiet = _run(_proc(kind, sample_rate, snip_edges), [waves[picked[4]]], [warps[picked[4]]], sample_rate)[0]
    assert not np.array_equal(quiet, alone[picked[4]])
    _backend.clear_plans()


@pytest.mark.parametrize('snip_edges', [True, False])
@pytest.mark.parametrize('kernel, sample_rate', [(PAIRED, 22050), (PAIRED, 32000), (LONG, 44100)])
def test_every_row_of_every_trip_is_written(gpu, kernel, sample_rate, snip_edges):
    """the filterbank of the batch into a block that comes out of the pool full of NaN bit patterns: no word of
    any row keeps the pattern, and the rows are those of the host call"""
    waves, warps = lf.multi_trip_batch(sample_rate, snip_edges)
    proc = _proc('fbank40', sample_rate, snip_edges)
    plan = _backend.get_plan(proc._build_options())
    counts = lf.frame_counts(waves, sample_rate, snip_edges)
    soff = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    foff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total, cols = int(foff[-1]), plan.ndims
    assert cols == 40
    d_wave = gpu.DeviceBuffer(2 * int(soff[-1]))
    d_wave.upload(np.concatenate(waves))
    gpu.DeviceBuffer(4 * total * cols).free()
    d_out = gpu.DeviceBuffer(4 * total * cols)      # (out of the pool: poisoned by the `gpu` fixture's switch)
    before = d_out.download(np.zeros(total * cols, dtype=np.uint32))
    assert (before == 0xFFFFFFFF).all()
    plan.run_device(d_wave.ptr, soff, foff, d_out.ptr, vtln_warps=warps)
    got = d_out.download(np.zeros((total, cols), dtype=np.float32))
    d_wave.free()
    d_out.free()
    assert plan.kernel_name(1) == kernel
    stale = (got.view(np.uint32) == 0xFFFFFFFF).any(axis=1)
    trips = lf.row_trips(waves, sample_rate, snip_edges)
    assert not stale.any(), 'rows never written, by trip (generic kernel, 0, 1, 2): %s' % np.bincount(
        trips[stale] + 1, minlength=4).tolist()
    host = np.concatenate(_run(proc, waves, warps, sample_rate), axis=0)
    assert np.array_equal(got, host)


# ---- 3. window and bank seams --------------------------------------------------------------------------------
def _seam_case(cls, win_len, snip_edges, kernel, **opts):
    """three small utterances (35, 36 and 1 frames) with three warps: the oracle's values, alone == in the
    batch bit for bit; `win_len` is asserted, not assumed"""
    rate = lf.SEAM_RATE
    proc = cls(sample_rate=rate, frame_length=lf.frame_length_for(win_len), dither=0, snip_edges=snip_edges, **opts)
    assert orc.window_size(proc._build_options().frame) == win_len
    waves, warps = lf.seam_batch(win_len, snip_edges)
    what = '%s win_len %d snip_edges %s %s' % (proc.name, win_len, snip_edges, opts)
    try:
        wants = [_oracle(proc, w, wf) for w, wf in zip(waves, warps)]
    except RuntimeError:   # (a warped bank with an empty bin: a Kaldi-class error on both sides)
        with pytest.raises(RuntimeError):
            _run(proc, waves, warps, rate)
        warps = [1.0] * len(waves)
        wants = [_oracle(proc, w, wf) for w, wf in zip(waves, warps)]
    gots = _run(proc, waves, warps, rate)
    assert _kernel(proc) == kernel
    assert [g.shape[0] for g in gots] == [35, 36, 1]
    for got, want in zip(gots, wants):
        assert_close(got, want, rtol=1e-4, what=what)
    for i in range(len(waves)):
        alone = _run(proc, [waves[i]], [warps[i]], rate)[0]
        assert np.array_equal(alone, gots[i]), '%s: utterance %d alone / in the batch' % (what, i)
    # (and an unwarped batch: the kernels' warp 0 tables)
    if cls is not SpectrogramProcessor and warps != [1.0] * len(waves):
        gots = _run(proc, waves, [1.0] * len(waves), rate)
        assert _kernel(proc) == kernel
        for got, wave in zip(gots, waves):
            assert_close(got, _oracle(proc, wave, 1.0), rtol=1e-4, what=what + ' unwarped')


WINDOW_CASES = [(kernel, win_len) for kernel, wins in lf.window_cases().items() for win_len in wins]


@pytest.mark.parametrize('snip_edges', [True, False])
@pytest.mark.parametrize('cls', [MfccProcessor, SpectrogramProcessor])
@pytest.mark.parametrize('kernel, win_len', WINDOW_CASES)
def test_window_seams(gpu, kernel, win_len, cls, snip_edges):
    """every step of the two launch ladders (NJ 9 / 13 / 16 by ceil(win_len / 64); NJ 9 / 10 / 16 by
    ceil(win_len / 128)), one and two 16-byte pieces per lane with and without tail samples, the smallest and
    the largest windows; an odd window above 1024 samples runs on the generic kernel"""
    _seam_case(cls, win_len, snip_edges, kernel)


@pytest.mark.parametrize('snip_edges', [True, False])
@pytest.mark.parametrize('num_bins', lf.BANK_BINS + (129,))
@pytest.mark.parametrize('kernel', [PAIRED, LONG])
def test_bank_seams(gpu, kernel, num_bins, snip_edges):
    """the mel epilogue works in rounds of 8 bins up to 128: a round with idle teams, exactly one round, one
    round and one bin, banks that need 10 and 16 rounds, the limit; 129 bins fall to the generic kernel"""
    _seam_case(FilterbankProcessor, lf.BANK_WINDOWS[kernel], snip_edges,
               kernel if num_bins <= 128 else 'mel_features_generic_kernel', num_bins=num_bins)
