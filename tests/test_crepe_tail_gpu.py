"""The two kernels of the CREPE tail on the device, each alone through ``CrepeBatch.set_rows`` (no network):
``snf_crepe_rows`` against scipy.signal.resample, ``snf_crepe_voicing_convert`` against the host functions
`predict_voicing` and `CrepePitchPostProcessor._convert`.

Tiling of the row resampler (csrc/snf_internal.h): one workgroup per 64 output rows (kCrepeRowsTile), the input
rows staged in LDS 1024 at a time (kCrepeRowsStage); the voicing kernel stages 1024 frames at a time
(kCrepeVoicingChunk).  BIG_PAIR and the long utterance of the conversion cases span several of each.

Every step on the device runs under its own time limit (the guard of tests/test_crepe_gpu.py); nothing is retried.
Measured figures are printed (run with -s); profiles/crepe_tail_errors.txt records them."""

import numpy as np
import pytest
import scipy.signal

import crepe_tail_f64 as tail
from test_crepe_gpu import on_device

pytestmark = pytest.mark.gpu

ROWS_TILE, ROWS_STAGE, VOICING_CHUNK = 64, 1024, 1024
BIG_PAIR = (2500, 2400)   # 38 tiles of output rows, 3 stages of input rows
_CACHE = {}


def offsets(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    return off


def device_rows(inputs, counts):
    """The rows ``snf_crepe_rows`` makes of the utterances `inputs`, one array per utterance"""
    from shennong_amd.processor import pitch_crepe
    with on_device():
        batch = pitch_crepe.CrepeBatch([np.zeros(1, dtype=np.int16)] * len(inputs), 160, True)
        batch.set_rows(np.concatenate(inputs), offsets([len(x) for x in inputs]))
        batch.rows(counts)
        got = batch.host_rows()
        batch.release()
    cuts = offsets(counts)
    return [got[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def rows_cases():
    """(N, M) -> (input rows, scipy's rows), computed once"""
    if 'rows' not in _CACHE:
        cases = {}
        for N, M in tail.PAIRS + [BIG_PAIR]:
            x = tail.decoder_like_rows(N, 1000 * N + M)
            cases[(N, M)] = (x, scipy.signal.resample(x, M))
        _CACHE['rows'] = cases
    return _CACHE['rows']


def test_rows_inputs_stay_clear_of_the_clamp():
    """From scipy alone: no reference confidence within 1e-6 of a threshold of the clamp, so that the rows the
    clamp acts on are the same for anything as close to scipy as the bound below - and the clamp does act"""
    low = high = 0
    for (N, M), (x, want) in rows_cases().items():
        assert np.abs(want[:, 0] - 1e-2).min() > 1e-6 and np.abs(want[:, 0] - 1).min() > 1e-6, (N, M)
        low, high = low + int((want[:, 0] < 1e-2).sum()), high + int((want[:, 0] > 1).sum())
    assert low > 50 and high > 50


def test_rows_against_scipy(gpu):
    """Bound 64 N 2^-52 max|column|: the 16 N 2^-52 of the float64 statement (tests/test_crepe_tail.py) times 4
    for the device's trigonometric functions.  One batch of every case, then every case alone: the same bits."""
    cases = rows_cases()
    pairs = list(cases)
    together = device_rows([cases[p][0] for p in pairs], [p[1] for p in pairs])
    worst = 0.0
    for (N, M), got in zip(pairs, together):
        x, want = cases[(N, M)]
        assert got.shape == (M, 2) and got.dtype == np.float64
        clamped = tail.clamp(want)
        acted = clamped[:, 0] != want[:, 0]
        assert np.array_equal(got[acted, 0], clamped[acted, 0]), (N, M)           # exactly 0 and 1, the same rows
        assert np.array_equal(got[:, 0] == 0, clamped[:, 0] == 0), (N, M)
        assert np.array_equal(got[:, 0] == 1, clamped[:, 0] == 1), (N, M)
        if M == N:
            assert np.array_equal(got, tail.clamp(x))
        for column in range(2):
            rows = ~acted if column == 0 else np.ones(M, dtype=bool)
            bound = 64 * N * 2.0 ** -52 * np.abs(x[:, column]).max()
            err = float(np.abs(got[rows, column] - want[rows, column]).max()) if rows.any() else 0.0
            worst = max(worst, err / bound)
            print('rows (%d, %d) column %d: error %.3g, bound %.3g, ratio %.3g' % (N, M, column, err, bound, err / bound))
            assert err <= bound, (N, M, column, err, bound)
    print('rows: worst error / bound %.3g' % worst)
    for (N, M), batched in zip(pairs, together):
        alone = device_rows([cases[(N, M)][0]], [M])[0]
        assert np.array_equal(alone, batched), (N, M)


def test_rows_refuses_empty_utterances(gpu):
    from shennong_amd.processor import pitch_crepe
    x = tail.decoder_like_rows(5, 1)
    with on_device():
        batch = pitch_crepe.CrepeBatch([np.zeros(1, dtype=np.int16)] * 2, 160, True)
        batch.set_rows(x, [0, 5, 5])
        with pytest.raises(ValueError, match='utterance 1 has no input or no output rows'):
            batch.rows([3, 3])
        batch.set_rows(x, [0, 2, 5])
        with pytest.raises(ValueError, match='utterance 0 has no input or no output rows'):
            batch.rows([0, 3])
        with pytest.raises(ValueError, match='2 utterances, 3 row counts'):
            batch.rows([1, 2, 3])
        batch.release()


def runs(rng, lengths, first_voiced):
    """(confidence, Hertz) rows whose confidence alternates between voiced (around 0.85) and unvoiced (around
    0.06) runs of `lengths` frames, every Hertz value its own"""
    conf, voiced = [], first_voiced
    for n in lengths:
        conf.append((0.85 if voiced else 0.06) + 0.1 * (rng.rand(n) - 0.5))
        voiced = not voiced
    conf = np.concatenate(conf)
    return np.stack([conf, 80 + 300 * rng.rand(len(conf))], axis=1)


def blips(rng, n, voiced, places):
    """A run of `n` frames of one class with short runs of the other class inside, `places` = (first frame,
    frames): what the 0.99 / 0.01 transitions smooth away (a frame of the wrong class costs 1.6 in log
    emission, leaving the class and coming back 9.2)"""
    rows = runs(rng, [n], voiced)
    for first, width in places:
        rows[first:first + width, 0] = (0.1 if voiced else 0.88) + 0.04 * (rng.rand(width) - 0.5)
    return rows


# the cases on which the Viterbi differs from a threshold at 0.5 frame by frame, and by at least how many frames
SMOOTHED = {'dips in a voiced run': 6, 'peaks in an unvoiced run': 4, 'mid confidences': 20,
            'dips across the chunks': 8, 'peaks across the chunks': 7}


def conversion_cases():
    """name -> (rows, expected status).  The bad utterances sit between good ones."""
    if 'conversion' in _CACHE:
        return _CACHE['conversion']
    rng = np.random.RandomState(20260927)
    chunk = VOICING_CHUNK
    mid = runs(rng, [30, 300, 25], True)
    mid[30:330, 0] = 0.3 + 0.4 * rng.rand(300)           # neither class is clear: the transitions decide
    peaks = np.concatenate([runs(rng, [40], True), blips(rng, 150, False, [(60, 1), (120, 3)])])
    # a dip / a peak on every multiple of the chunk: the lattice and the state are handed over inside it
    dips_far = blips(rng, 3 * chunk + 100, True, [(chunk - 1, 3), (2 * chunk - 1, 2), (3 * chunk - 2, 3)])
    peaks_far = np.concatenate([runs(rng, [chunk - 50], True),
                                blips(rng, 2 * chunk + 90, False, [(49, 3), (chunk + 49, 2), (2 * chunk + 49, 2)])])
    cases = [
        ('unvoiced edges', runs(rng, [7, 30, 12, 41, 9], False), 0),
        ('no voiced frame', runs(rng, [50], False), 1),
        ('voiced edges', runs(rng, [25, 11, 33, 6, 18], True), 0),
        ('one voiced frame', np.array([[0.9, 123.0]]), 0),
        ('zero Hertz', runs(rng, [40, 10, 20], True), 2),
        ('all voiced', runs(rng, [130], True), 0),
        ('one unvoiced frame', np.array([[0.03, 150.0]]), 1),
        ('voiced start', runs(rng, [60, 20], True), 0),
        ('out of range POV', runs(rng, [30, 15, 30], True), 3),
        ('several chunks', runs(rng, [700, 300, 900, 500, 210], False), 0),
        ('clamped values', runs(rng, [20, 20, 20], False), 0),
        ('unvoiced end', runs(rng, [21, 13], True), 0),
        ('dips in a voiced run', blips(rng, 200, True, [(20, 1), (90, 2), (150, 3)]), 0),
        ('peaks in an unvoiced run', peaks, 0),
        ('mid confidences', mid, 0),
        ('dips across the chunks', dips_far, 0),
        ('peaks across the chunks', peaks_far, 0)]
    cases = {name: [rows, status] for name, rows, status in cases}
    cases['zero Hertz'][0][5, 1] = 0.0          # a voiced frame
    cases['out of range POV'][0][3, 0] = 0.99995   # above f(1) = 0.99990, below 1
    clamped = cases['clamped values'][0]        # what the clamp leaves: exact zeros and ones
    clamped[:6, 0], clamped[25:30, 0] = 0.0, 1.0
    assert len(cases['several chunks'][0]) > 2 * VOICING_CHUNK
    _CACHE['conversion'] = {name: (rows, status) for name, (rows, status) in cases.items()}
    return _CACHE['conversion']


def test_the_cases_need_the_lattice():
    """On the host alone: on the SMOOTHED cases the most likely states are not the confidences thresholded at 0.5
    - a kernel without the recursion, with other transitions, or one that loses the lattice or the state at a chunk
    boundary does not pass them -, a dip or a peak lies on every multiple of the chunk, and the decisions do not
    hang on the last bits"""
    from shennong_amd.processor.pitch_crepe import predict_voicing
    cases = conversion_cases()
    for name, least in SMOOTHED.items():
        conf = cases[name][0][:, 0]
        states = predict_voicing(conf)
        differ = states != (conf > 0.5)
        print('%-26s %5d frames, the states differ from the threshold on %d' % (name, len(conf), differ.sum()))
        assert differ.sum() >= least, (name, int(differ.sum()))
        for shift in (1e-12, -1e-12):
            assert np.array_equal(predict_voicing(conf + shift), states), name
    for name in ('dips across the chunks', 'peaks across the chunks'):
        conf = cases[name][0][:, 0]
        differ = predict_voicing(conf) != (conf > 0.5)
        for boundary in range(VOICING_CHUNK, len(conf), VOICING_CHUNK):
            assert differ[boundary - 1] and differ[boundary], (name, boundary)
    # the stretch of mid confidences is not one class throughout: both decisions are taken inside it
    states = predict_voicing(cases['mid confidences'][0][:, 0])[30:330]
    print('mid confidences: %d of 300 frames voiced' % states.sum())
    assert 50 < states.sum() < 250


def host_conversion(rows):
    """(states of predict_voicing, the float32 rows of _convert)"""
    from shennong_amd import Features
    from shennong_amd.processor import CrepePitchPostProcessor, CrepePitchProcessor
    from shennong_amd.processor.pitch_crepe import predict_voicing
    states = predict_voicing(rows[:, 0])
    # the comparison of the states is one of decisions: the margins must not hang on the last bits
    for shift in (1e-12, -1e-12):
        assert np.array_equal(predict_voicing(rows[:, 0] + shift), states)
    feats = Features(rows, CrepePitchProcessor().times(len(rows)), validate=False)
    return states, CrepePitchPostProcessor()._convert(feats).data


def device_conversion(named):
    """(status vector, rows per utterance, the exception convert raised or None)"""
    from shennong_amd.processor import pitch_crepe
    inputs = [rows for rows, _ in named.values()]
    cuts = offsets([len(x) for x in inputs])
    with on_device():
        batch = pitch_crepe.CrepeBatch([np.zeros(1, dtype=np.int16)] * len(inputs), 160, True)
        batch.set_rows(np.concatenate(inputs), cuts)
        raised = None
        try:
            batch.convert()
        except ValueError as err:
            raised = str(err)
        got = batch.host_nccf_pitch()
        status = batch.status.copy()
        batch.release()
    return status, [got[a:b] for a, b in zip(cuts[:-1], cuts[1:])], raised


def test_voicing_convert(gpu):
    cases = conversion_cases()
    status, got, raised = device_conversion(cases)
    assert status.tolist() == [want for _, want in cases.values()]
    assert raised == 'No voiced frames'   # the first bad utterance's
    worst = 0.0
    for (name, (rows, want_status)), out in zip(cases.items(), got):
        assert out.shape == (len(rows), 2) and out.dtype == np.float32, name
        assert np.isfinite(out).all(), name
        if want_status in (1, 2):
            assert not out.any(), name
        if want_status:
            continue
        states, want = host_conversion(rows)
        assert 0 < states.sum(), name
        # an unvoiced frame takes a value between (or of) its neighbours', a voiced one keeps its own: every
        # Hertz value is its own, so the pattern is the states
        kept = out[:, 1] == rows[:, 1].astype(np.float32)
        assert np.array_equal(kept, states == 1), name
        ulp = np.spacing(np.abs(want))
        assert (np.abs(out.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), name
        worst = max(worst, float((np.abs(out.astype(np.float64) - want) / ulp).max()))
        same = float((out == want).mean())
        print('convert %-20s %5d frames, %4d voiced, %.4f of the values bit-equal' % (name, len(rows), states.sum(), same))
    print('convert: worst difference %.3g float32 ulp' % worst)
    assert set(SMOOTHED) <= set(cases)
    # the good utterances alone: no exception, and the bits they had between the bad ones
    good = {name: case for name, case in cases.items() if case[1] == 0}
    status, alone, raised = device_conversion(good)
    assert raised is None and not status.any()
    for name, out in zip(good, alone):
        assert np.array_equal(out, got[list(cases).index(name)]), name
    # every bad utterance alone raises its own message
    from shennong_amd.processor.pitch_crepe import _STATUS_MESSAGES
    for name, case in cases.items():
        if case[1]:
            status, _, raised = device_conversion({name: case})
            assert status.tolist() == [case[1]] and raised == _STATUS_MESSAGES[case[1]], name


def test_voicing_convert_empty(gpu):
    """No utterance, and an utterance without rows (status 0, nothing written)"""
    cases = conversion_cases()
    named = {'a': cases['all voiced'], 'empty': (np.zeros((0, 2)), 0), 'b': cases['voiced edges']}
    status, got, raised = device_conversion(named)
    assert raised is None and status.tolist() == [0, 0, 0] and got[1].shape == (0, 2)
    assert np.array_equal(got[0], device_conversion({'a': cases['all voiced']})[1][0])
