"""The five kernels of the post-processing path that the route tests left out - vad_threshold_kernel / vad_kernel,
sliding_cmvn_kernel (kernels_cmvn.hip), concat_columns_kernel, count_nonfinite_kernel (kernels_post.hip) and
mfcc_dct_kernel (kernels_dct.hip) - on the batches of post_layouts.py, against the statements and derived bounds of post_f64.py.
test_post_remaining.py shows on the CPU that the layouts reach their seams, that no VAD frame lies in the band a
float64 statement cannot decide, and that the float32 C oracle meets the same bounds on the same inputs.  Every test
asserts its route through Plan.kernel_name where a plan exists and prints its worst error over bound (run with -s;
the committed lines are profiles/post_remaining_errors.txt).  The `gpu` fixture fills LDS and pooled buffers with NaN
bit patterns: output a kernel never wrote is not finite, and no statement below allows that."""

import ctypes as C
import functools

import numpy as np
import pytest

import post_f64
import post_layouts as lay
from conftest import assert_close
from oracle import oracle as orc
from shennong_amd import Audio, Features, _backend
from shennong_amd.postprocessor import SlidingWindowCmvnPostProcessor, VadPostProcessor
from shennong_amd.processor import FilterbankProcessor, MfccProcessor

pytestmark = pytest.mark.gpu


def _features(mats):
    return [Features(m, np.arange(m.shape[0], dtype=np.float64) * 0.01, validate=False) for m in mats]


# ---- VAD ------------------------------------------------------------------------------------------------------------
def _vad(ctx, scale, p, et):
    return VadPostProcessor(energy_threshold=et, energy_mean_scale=scale, frames_context=ctx, proportion_threshold=p)


def _run_vad(proc, mats):
    outs = proc._process_batch(_features(mats))
    if any(m.shape[0] for m in mats):
        assert _backend.get_plan(proc._build_options()).kernel_name(1) == 'vad_kernel'
    assert [(o.shape, o.dtype) for o in outs] == [((m.shape[0], 1), np.uint8) for m in mats]
    return [o.data[:, 0] for o in outs]


@pytest.mark.parametrize('cols', lay.VAD_COLS)
@pytest.mark.parametrize('options', lay.VAD_OPTIONS, ids=str)
def test_vad(gpu, options, cols):
    """every flag of every frame equals the statement's: no frame is excluded (test_post_remaining.py shows that no
    energy of these batches lies within the four float32 roundings of its threshold)"""
    ctx, scale, p, et = options
    mats = post_f64.vad_batch(cols, lay.vad_layout())
    got = _run_vad(_vad(ctx, scale, p, et), mats)
    wrong = excluded = 0
    for u, (g, m) in enumerate(zip(got, mats)):
        want, inside, _ = post_f64.vad_want(m[:, 0], ctx, scale, p, et)
        excluded += inside
        wrong += int(np.count_nonzero(g != want))
        assert np.array_equal(g, want.astype(np.uint8)), (u, m.shape[0], np.flatnonzero(g != want)[:8])
    print(f'vad {options} d{cols}: {wrong} wrong flags of {sum(m.shape[0] for m in mats)}, {excluded} frames excluded')
    assert excluded == 0


@pytest.mark.parametrize('ctx', [2, 300])
def test_vad_alone_and_in_the_batch(gpu, ctx):
    """an utterance's flags do not depend on its neighbours: the window stops at the utterance's own ends"""
    mats = post_f64.vad_batch(13, lay.vad_layout())
    proc = _vad(ctx, 0.5, 0.5, 5.0)
    batch = _run_vad(proc, mats)
    for u, m in enumerate(mats):
        if m.shape[0]:
            assert np.array_equal(_run_vad(proc, [m])[0], batch[u]), (u, m.shape[0])
    # all-empty batches and a batch of one empty utterance come back empty
    assert [o.shape for o in _run_vad(proc, [mats[0], mats[7]])] == [(0,), (0,)]


@pytest.mark.parametrize('ctx, p', lay.VAD_TIES)
def test_vad_ties(gpu, ctx, p):
    """energies that are multiples of 1/4 with mean 10: the threshold 5 + 0.5 x 10 is exact in every step, ten frames
    lie exactly on it and do not count (`>` is strict); where num == den x proportion_threshold holds exactly in
    float32 - 3 of 5 at 0.6, 1 of 4 at 0.25 at the utterance's edges - the frame is voiced (`>=`)"""
    mats = post_f64.vad_tie_batch(13)
    got = _run_vad(_vad(ctx, 0.5, p, 5.0), mats)
    want = [post_f64.vad_want(m[:, 0], ctx, 0.5, p, 5.0, threshold=10.0 if u == 1 else None)[0]
            for u, m in enumerate(mats)]
    for u, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w.astype(np.uint8)), (u, np.flatnonzero(g != w)[:8])
    e = mats[1][:, 0]
    if ctx == 0:
        assert not np.any(got[1][e == 10.0]) and np.array_equal(got[1], (e > 10.0).astype(np.uint8))
    if (ctx, p) == (2, 0.25):
        assert got[1][1] == 1 and got[1][254] == 1
    assert np.array_equal(_run_vad(_vad(ctx, 0.5, p, 5.0), [mats[1]])[0], got[1])
    print(f'vad ties context {ctx} proportion {p}: {int(got[1].sum())} of 256 voiced, every flag as stated')


# ---- sliding-window CMVN --------------------------------------------------------------------------------------------
def _sliding(center, cmn, minw, nv):
    return SlidingWindowCmvnPostProcessor(center=center, cmn_window=cmn, min_window=minw, normalize_variance=nv)


def _run_sliding(proc, mats):
    outs = proc._process_batch(_features(mats))
    if any(m.size for m in mats):
        assert _backend.get_plan(proc._build_options()).kernel_name(1) == 'sliding_cmvn_kernel'
    assert [(o.shape, o.dtype) for o in outs] == [(m.shape, np.float32) for m in mats]
    return [o.data for o in outs]


@functools.lru_cache(maxsize=None)
def _sliding_reference(cmn, minw, center, nv, which):
    """(inputs of 257 columns, (want, bound) per utterance): computed once per window and shared by the column counts
    (read only) - a narrower batch is the first columns of this one"""
    lengths = lay.sliding_lengths(cmn, minw) if which == 'all' else lay.sliding_five(cmn, minw)
    mats = post_f64.sliding_batch(lengths, post_f64.SLIDING_MAX_COLS)
    return mats, [post_f64.sliding_want(m, center, cmn, minw, nv) for m in mats]


@pytest.mark.parametrize('cols', lay.SLIDING_COLS)
@pytest.mark.parametrize('case', lay.SLIDING_CASES, ids=lay.sliding_id)
def test_sliding_cmvn(gpu, case, cols):
    """|got - want| <= 2^-24 |want| + K 2^-53 A s against the statement that forms every window directly
    (post_f64.sliding_want); with 13 columns also the batch of five utterances: 65 threads, the last alone in a
    second workgroup"""
    (cmn, minw), center, nv = case
    proc = _sliding(center, cmn, minw, nv)
    for which in ('all', 'five') if cols == 13 else ('all',):
        mats, wants = _sliding_reference(cmn, minw, center, nv, which)
        got = _run_sliding(proc, [np.ascontiguousarray(m[:, :cols]) for m in mats])
        ratio, u, row, col = post_f64.sliding_ratio(got, [(w[:, :cols], b[:, :cols]) for w, b in wants])
        print(f'sliding_cmvn {lay.sliding_id(case)} d{cols} {which}: worst error / bound {ratio:.3f} '
              f'(utterance {u}, row {row}, column {col})')
        assert ratio <= 1.0, (ratio, u, row, col)


@pytest.mark.parametrize('case', lay.SLIDING_CASES, ids=lay.sliding_id)
def test_sliding_cmvn_alone_and_in_the_batch(gpu, case):
    """the rows of an utterance alone equal its rows in the batch bit for bit; a window of one frame (a one-frame
    utterance) gives the literal 0 with variance normalisation"""
    (cmn, minw), center, nv = case
    proc = _sliding(center, cmn, minw, nv)
    mats, _ = _sliding_reference(cmn, minw, center, nv, 'all')
    mats = [np.ascontiguousarray(m[:, :13]) for m in mats]
    batch = _run_sliding(proc, mats)
    for u, m in enumerate(mats):
        if m.shape[0]:
            alone = _run_sliding(proc, [m])[0]
            assert np.array_equal(alone.view(np.uint32), batch[u].view(np.uint32)), (u, m.shape[0])
        if m.shape[0] == 1 and nv:
            assert not np.any(batch[u].view(np.uint32))
    assert [o.shape for o in _run_sliding(proc, [mats[0], mats[6]])] == [(0, 13), (0, 13)]


@pytest.mark.parametrize('center', [True, False])
def test_sliding_cmvn_window_of_one_frame(gpu, center):
    """cmn_window = 1, centred: every window is the frame itself, wf == 1 everywhere - the literal 0 with variance
    normalisation, x - x = 0 without"""
    mats = post_f64.sliding_batch([0, 1, 5, 70, 0], 13)
    for nv in (True, False):
        got = _run_sliding(_sliding(center, 1, 1, nv), mats)
        wants = [post_f64.sliding_want(m, center, 1, 1, nv) for m in mats]
        assert post_f64.sliding_ratio(got, wants)[0] <= 1.0
        if center:
            assert all(not np.any(g.view(np.uint32)) for g in got)


@pytest.mark.parametrize('nv', [False, True], ids=['mean', 'var'])
def test_sliding_cmvn_constant_columns(gpu, nv):
    """A column that is constant over an utterance gives exactly 0.0 with and without variance normalisation, at
    every window length: its sums are exact (S = wf x), the kernel's mean S / wf is one correctly rounded quotient
    and returns x itself, and 0 stays 0 whatever the variance floor multiplies it by.  The derived bound is asserted
    first.

    This test found the kernel forming x + fl(-1 / wf) S as Kaldi's SlidingWindowCmnInternal does (AddVec with
    alpha = -1.0 / window_frames), compiled to one fused multiply-add: x times the rounding error of -1 / wf was
    left wherever wf is no power of two - 15 420 of the 15 536 results of these batches were not 0.0, the largest
    5.82e-16 without and 5.82e-11 with variance normalisation (the floor 1e-10 scales the residue by 1e5).  The C
    oracle, which keeps Kaldi's form and fuses nothing, still leaves up to 8.9e-16 and 8.9e-11 wherever
    fl(1 / wf) wf != 1 (test_post_remaining.py::test_sliding_constant_columns_on_the_oracle)."""
    worst, where, nonzero, total = 0.0, None, 0, 0
    for cmn, minw in lay.SLIDING_WINDOWS:
        mats = post_f64.sliding_constant_batch(lay.sliding_lengths(cmn, minw))
        for center in (True, False):
            got = _run_sliding(_sliding(center, cmn, minw, nv), mats)
            wants = [post_f64.sliding_want(m, center, cmn, minw, nv) for m in mats]
            assert post_f64.sliding_ratio(got, wants)[0] <= 1.0
            for u, g in enumerate(got):
                if g.size:
                    size = float(np.abs(g[:, [0, 2]]).max())
                    nonzero += int(np.count_nonzero(g[:, [0, 2]]))
                    total += 2 * g.shape[0]
                    if size > worst:
                        worst, where = size, (cmn, minw, center, u, g.shape[0])
    print(f'sliding_cmvn constant columns {"var" if nv else "mean"}: largest |result| {worst:.3g} at '
          f'(cmn_window, min_window, center, utterance, frames) {where}, {nonzero} of {total} results not 0.0')
    assert worst == 0.0, (worst, where, nonzero, total)


# ---- column concatenation -------------------------------------------------------------------------------------------
SENTINELS = 64


def _upload(array, extra=0):
    array = np.ascontiguousarray(array)
    buf = _backend.DeviceBuffer(array.nbytes + extra)
    if array.nbytes:
        buf.upload(array)
    return buf


def _concat(a, b, rows_out, ca, cb):
    """(output rows as uint32, the sentinel floats behind them before and after) of one concat_columns_device call"""
    rows_a, rows_b = [m.shape[0] for m in a], [m.shape[0] for m in b]
    total, co = int(sum(rows_out)), ca + cb
    flat_a = np.concatenate(a) if a else np.zeros((0, ca), np.float32)
    flat_b = np.concatenate(b) if b else np.zeros((0, cb), np.float32)
    before = np.arange(total * co + SENTINELS, dtype=np.uint32) + np.uint32(0x4B000000)   # 2^23 + i: finite, distinct
    d_a, d_b, d_out = _upload(flat_a), _upload(flat_b), _upload(before)
    try:
        _backend.concat_columns_device(d_a.ptr, ca, lay.offsets_of(rows_a), d_b.ptr, cb, lay.offsets_of(rows_b),
                                       d_out.ptr, lay.offsets_of(rows_out))
        after = d_out.download(np.empty_like(before))
    finally:
        for d in (d_a, d_b, d_out):
            d.free()
    return after[:total * co].reshape(total, co), before, after


@pytest.mark.parametrize('ca, cb', lay.CONCAT_COLS)
def test_concat_columns(gpu, ca, cb):
    """np.concatenate([a[u][:r], b[u][:r]], axis=1), bit for bit, with an utterance boundary on every seam of the
    32-row tiles, a and b longer than the output by turns, -0 and denormals among the values, and 64 sentinel floats
    behind the output that stay as they were"""
    rows_out, rows_a, rows_b = lay.check_concat(*lay.concat_layout())
    a, b = post_f64.concat_inputs(rows_a, rows_b, ca, cb)
    want = np.concatenate(post_f64.concat_want(a, b, rows_out)).view(np.uint32)
    got, before, after = _concat(a, b, rows_out, ca, cb)
    wrong = np.argwhere(got != want)
    print(f'concat_columns ({ca}, {cb}): {len(wrong)} of {want.size} elements differ'
          + (f', the first at row {wrong[0][0]}, column {wrong[0][1]}' if len(wrong) else ''))
    assert not len(wrong)
    assert np.array_equal(after[-SENTINELS:], before[-SENTINELS:])


def test_concat_columns_refusals(gpu):
    """an output longer than an input is refused before any launch; no utterance, or none with rows, touches
    nothing"""
    rows_out, rows_a, rows_b = lay.concat_layout()
    a, b = post_f64.concat_inputs(rows_a, rows_b, 13, 3)
    for u in (12, 11):     # utterance 12: one row more than a holds (b has three to spare); utterance 11: than b holds
        longer = list(rows_out)
        longer[u] += 1
        assert (longer[u] > rows_a[u], longer[u] > rows_b[u]) == ((True, False) if u == 12 else (False, True))
        with pytest.raises(ValueError, match=f'concatenation rows exceed an input for utterance {u}'):
            _concat(a, b, longer, 13, 3)
    got, before, after = _concat([], [], [], 13, 3)
    assert np.array_equal(after, before)
    empty_out = [0] * len(rows_out)
    got, before, after = _concat(a, b, empty_out, 13, 3)
    assert got.shape == (0, 16) and np.array_equal(after, before)
    # ... and the refused calls wrote nothing either: the same inputs still concatenate
    got, _, _ = _concat(a, b, rows_out, 13, 3)
    assert np.array_equal(got, np.concatenate(post_f64.concat_want(a, b, rows_out)).view(np.uint32))


# ---- non-finite count -----------------------------------------------------------------------------------------------
def _count(ptr, n):
    bad = C.c_uint64(12345)
    _backend.check(_backend.lib().snf_count_nonfinite_device(_backend._DEVICE, C.c_void_p(ptr), int(n), C.byref(bad)))
    return int(bad.value)


def _poke(ptr, index, bits):
    word = np.array([bits], dtype=np.uint32)
    _backend.check(_backend.lib().snf_memcpy_h2d(C.c_void_p(ptr + 4 * int(index)), word.ctypes.data_as(C.c_void_p), 4))


@pytest.mark.parametrize('n', lay.NONFINITE_SIZES + [lay.NONFINITE_SECOND_PASS])
def test_count_nonfinite(gpu, n):
    """np.count_nonzero(~np.isfinite(x)): none among finite values that include +-FLT_MAX, denormals and +-0; one at
    element 0, at the end of the vector body, at each tail element and at the first elements of a thread's second
    pass; several at once; every element"""
    x = post_f64.finite_fill(n)
    places = lay.nonfinite_places(n)
    kinds = list(post_f64.NONFINITE_BITS.values())
    buf = _upload(x, extra=16)
    try:
        assert buf.ptr % 16 == 0
        assert _count(buf.ptr, n) == 0
        with pytest.raises(ValueError, match='not 16-byte aligned'):
            _count(buf.ptr + 4, max(n - 1, 1))
        _backend.check_finite_device(buf.ptr, n)
        for k, index in enumerate(places):
            _poke(buf.ptr, index, kinds[k % len(kinds)])
            assert _count(buf.ptr, n) == 1, (n, index)
            with pytest.raises(ValueError, match='non-finite'):
                _backend.check_finite_device(buf.ptr, n)
            _poke(buf.ptr, index, x[index:index + 1].view(np.uint32)[0])
        assert _count(buf.ptr, n) == 0
        y = x.copy()
        y.view(np.uint32)[places] = [kinds[k % len(kinds)] for k in range(len(places))]
        buf.upload(y)
        assert _count(buf.ptr, n) == post_f64.nonfinite_count(y) == len(places)
        # a pointer 16 bytes in: the first four floats are not read, the body and the tail move with it
        if n > 4:
            assert _count(buf.ptr + 16, n - 4) == post_f64.nonfinite_count(y[4:])
        buf.upload(np.full(n, kinds[n % len(kinds)], np.uint32))
        assert _count(buf.ptr, n) == n
    finally:
        buf.free()
    print(f'count_nonfinite n = {n}: {lay.nonfinite_launch(n)} (workgroups, vectors, passes, tail), '
          f'{len(places)} places, every count as stated')


def test_count_nonfinite_kinds(gpu):
    """each kind that counts - +-Inf, quiet, signalling and negative NaN patterns - and each that does not - +-FLT_MAX,
    the smallest and the largest denormal, +-0 - in the vector body and in the tail"""
    n = 7
    buf = _upload(np.ones(n, np.float32))
    try:
        for index in (0, 3, 6):
            for name, bits in post_f64.NONFINITE_BITS.items():
                _poke(buf.ptr, index, bits)
                assert _count(buf.ptr, n) == 1, (name, index)
            for name, bits in post_f64.FINITE_BITS.items():
                _poke(buf.ptr, index, bits)
                assert _count(buf.ptr, n) == 0, (name, index)
        assert _count(buf.ptr, 0) == 0 and _count(0, 0) == 0
    finally:
        buf.free()


# ---- MFCC DCT tail --------------------------------------------------------------------------------------------------
def _oracle(proc, wave):
    return orc.compute(proc._build_options(), np.asarray(wave, np.int16), 1.0)


def _mfcc_batch(proc, wave, copies):
    feats = proc._process_batch([Audio(wave, 16000)] * copies)
    plan = _backend.get_plan(proc._build_options())
    names = {plan.kernel_name(k) for k in range(1, 6)} - {None}
    assert 'mfcc_dct_kernel' in names and names & {'fbank512b_kernel', 'fbank512_kernel'}, names
    return [f.data for f in feats]


@pytest.mark.parametrize('case', lay.MFCC_FIRST + [lay.MFCC_BIG], ids=lay.mfcc_id)
def test_mfcc_dct_position_independence(gpu, case):
    """the kernel works row by row: copies of one utterance (77 or 821 frames: no multiple of 64) in a batch just past
    one workgroup's frames - or past 256 workgroups' frames, where every wave takes a second tile - give the same
    cepstra bit for bit wherever their rows fall, and alone the utterance matches the oracle"""
    opts, copies = case
    big = 'frame_shift' in opts
    wave = post_f64.mfcc_wave(big)
    proc = MfccProcessor(dither=0, **opts)
    frames = lay.MFCC_BIG_FRAMES if big else lay.MFCC_UTT_FRAMES
    waves, per_group, blocks, per_wave = lay.mfcc_dct_launch(opts['num_bins'], opts['num_ceps'], lay.mfcc_energy(opts),
                                                             copies * frames)
    assert (blocks, per_wave) == ((256, 2) if big else (2, 1)) and copies * frames > per_group
    alone = _mfcc_batch(proc, wave, 1)[0]
    assert alone.shape == (frames, opts['num_ceps'])
    assert_close(alone, _oracle(proc, wave), rtol=1e-4, what=f'mfcc {opts}')
    batch = _mfcc_batch(proc, wave, copies)
    differ = [u for u, rows in enumerate(batch) if not np.array_equal(rows.view(np.uint32), alone.view(np.uint32))]
    print(f'mfcc_dct {lay.mfcc_id(case)}: {waves} waves, {blocks} workgroups, {per_wave} tile(s) per wave, '
          f'{len(differ)} of {copies} copies differ from the utterance alone')
    assert not differ, differ[:8]


@pytest.mark.parametrize('case', lay.MFCC_FIRST + [lay.MFCC_BIG], ids=lay.mfcc_id)
def test_mfcc_dct_bound(gpu, case):
    """|got - want| <= K 2^-24 sum |dct| |lifter| |x| against the float64 DCT (lifter, c0 and htk rules of
    oracle/spec_f64.py) of the float32 rows FilterbankProcessor returns for the same options.  Those are the bits
    the MFCC plan's scratch holds: the plan builds its filterbank stage with the function a filterbank plan uses
    (capi_plan.hip build_fbank_fast / fast512_build, from the same window, mel banks and options: log, power, the
    energy in column 0, no warp), and capi_mel.hip runs both through the same run_front_end -> launch_fbank512 on
    the same batch tables.  With use_energy, c0 is the filterbank's energy column bit for bit."""
    opts, copies = case
    copies = min(copies, 9)
    wave = post_f64.mfcc_wave('frame_shift' in opts)
    fbank = FilterbankProcessor(dither=0, **lay.fbank_options(opts))
    rows = [f.data for f in fbank._process_batch([Audio(wave, 16000)] * copies)]
    assert _backend.get_plan(fbank._build_options()).kernel_name(1) in ('fbank512b_kernel', 'fbank512_kernel')
    got = _mfcc_batch(MfccProcessor(dither=0, **opts), wave, copies)
    energy, htk = lay.mfcc_energy(opts), opts.get('htk_compat', False)
    want, bound = post_f64.mfcc_dct_want(rows[0], opts['num_bins'], opts['num_ceps'], opts.get('cepstral_lifter', 22.0),
                                         energy, htk)
    worst = 0.0
    for r, g in zip(rows, got):
        assert np.array_equal(r, rows[0]) and g.shape == want.shape
        assert np.isfinite(g).all()
        err = np.abs(g.astype(np.float64) - want)
        worst = max(worst, float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))))
        if energy:
            assert np.array_equal(g[:, opts['num_ceps'] - 1 if htk else 0], r[:, 0])
    print(f'mfcc_dct {lay.mfcc_id(case)}: worst error / bound {worst:.3f} (K = {post_f64.mfcc_dct_k(opts["num_bins"])})')
    assert worst <= 1.0
