"""CPU half of the tests of the VAD, sliding-window CMVN, column concatenation, non-finite count and MFCC DCT
kernels: the layouts of post_layouts.py reach the seams they claim, no frame of any VAD case lies in the band a
float64 statement cannot decide, and the float32 C oracle meets the bounds of post_f64.py on the very inputs
test_post_remaining_gpu.py gives the HIP kernels.  The last section restates each kernel's indexing in numpy, with
the mutations the device tests are meant to catch: the statements and bounds tell the restated kernel from each
mutant on the inputs of the device tests."""

import functools

import numpy as np
import pytest

import post_f64
import post_layouts as lay
from oracle import oracle as orc
from oracle import spec_f64
from shennong_amd.processor import FilterbankProcessor, MfccProcessor


# ---- VAD ------------------------------------------------------------------------------------------------------------
def test_vad_layout():
    lengths = lay.vad_layout()
    assert lengths[:-5] == lay.seam_layout(256)[:-1] and lengths[-5:] == [255, 256, 257, 513, 0]
    assert max(lengths) == 764 and 2600 < sum(lengths) < 2800
    # passes of `for (t = threadIdx.x; t < T; t += 256)` that thread 0 makes, and the lanes of the last pass
    assert {(n + 255) // 256 for n in (255, 256, 257, 513, 764)} == {1, 2, 3}
    assert 257 % 256 == 1 and 513 % 256 == 1 and 764 % 64 != 0
    with pytest.raises(ValueError, match='257'):
        lay.check_vad_passes([n for n in lengths if n != 257])
    with pytest.raises(ValueError, match='empty'):
        lay.check_vad_passes(lengths[1:])


def _spec_flags(e, ctx, scale, p, et):
    return spec_f64.vad_energy(np.asarray(e, np.float64)[:, None], float(np.float32(et)), float(np.float32(scale)),
                               ctx, float(np.float32(p)))[0]


@pytest.mark.parametrize('options', lay.VAD_OPTIONS, ids=str)
def test_vad_no_frame_in_the_band(options):
    """the cap on excluded frames is zero: for every case no energy lies within the rounding of its threshold, so
    every flag is decided; the float32 oracle decides them as the statement does, whatever the other columns hold;
    and the statement is spec_f64.vad_energy but for the float32 product den x proportion_threshold"""
    ctx, scale, p, et = options
    lengths = lay.vad_layout()
    closest, voiced = np.inf, 0
    for cols in lay.VAD_COLS:
        mats = post_f64.vad_batch(cols, lengths)
        for u, m in enumerate(mats):
            assert m.shape == (lengths[u], cols)
            assert np.array_equal(m[:, 0], post_f64.vad_batch(1, lengths)[u][:, 0]) or cols == 1
            want, inside, gap = post_f64.vad_want(m[:, 0], ctx, scale, p, et)
            assert inside == 0, (u, inside)
            _, band = post_f64.vad_band(m[:, 0], et, scale)
            assert gap > band
            closest = min(closest, gap / band if band else np.inf)
            voiced += int(want.sum())
            assert np.array_equal(orc.vad_energy(m, et, scale, ctx, p), want.astype(np.float32)), (cols, u)
            if cols == 1 and m.shape[0]:
                spec = _spec_flags(m[:, 0], ctx, scale, p, et)
                differ = np.flatnonzero(spec != want)
                if p in (0.5, 0.25):     # the product is exact in float32 and in double
                    assert differ.size == 0
                assert np.all(want[differ] == 1.0)     # (a float32 product that rounds DOWN to num)
            if cols > 1 and ctx == 0 and m.shape[0] > 100:
                # column 1 in place of column 0 would turn most decisions round
                wrong, _, _ = post_f64.vad_want(m[:, 1], ctx, scale, p, et)
                assert np.mean(wrong != want) > 0.8
    total = 3 * sum(lengths)
    assert 0.1 * total < voiced < 0.9 * total      # neither all voiced nor all silent
    print(f'vad oracle {options}: closest energy to its threshold {closest:.3g} bands away, {voiced} of {total} voiced')


def test_vad_statement_tells_a_single_pass_of_the_sum():
    """a threshold kernel whose stride loop ran once would take the mean of the first 256 energies only (still
    dividing by T): the flags of the utterances of 513 and 764 frames tell, at every context"""
    lengths = lay.vad_layout()
    mats = post_f64.vad_batch(1, lengths)
    for ctx, scale, p, et in lay.VAD_OPTIONS:
        if scale == 0:
            continue
        told = []
        for u, m in enumerate(mats):
            e = m[:, 0].astype(np.float64)
            if e.shape[0] <= lay.VAD_THREADS:
                continue
            want, _, _ = post_f64.vad_want(e, ctx, scale, p, et)
            short = float(np.float32(et)) + float(np.float32(scale)) * e[:lay.VAD_THREADS].sum() / e.shape[0]
            wrong, _, _ = post_f64.vad_want(e, ctx, scale, p, et, threshold=short)
            if not np.array_equal(want, wrong):
                told.append(e.shape[0])
        assert {513, 764} <= set(told), (ctx, told)


def test_vad_band():
    """four float32 roundings of |energy_threshold| + |scale mean|, plus the double sum"""
    e = post_f64.vad_batch(1, [764])[0][:, 0]
    thr, band = post_f64.vad_band(e, 5.0, 0.5)
    mean = float(np.mean(e.astype(np.float64)))
    assert abs(thr - (5.0 + 0.5 * mean)) < 1e-12
    assert 4 * post_f64.U24 * (5.0 + 0.5 * mean) <= band <= 4.001 * post_f64.U24 * (5.0 + 0.5 * mean)
    # the float32 chain of the kernel is inside it, in either summation order
    for total in (np.sum(e.astype(np.float64)), np.sum(e[::-1].astype(np.float64))):
        v = np.float32(5.0) + np.float32(0.5) * np.float32(total) / np.float32(e.shape[0])
        assert v.dtype == np.float32 and abs(float(v) - thr) <= band
    assert post_f64.vad_band(e, 5.0, 0.0) == (5.0, 0.0) and post_f64.vad_band(e[:0], 5.0, 0.5) == (5.0, 0.0)


def test_vad_tie_energies_are_exact():
    """every step of the threshold is exact, so an energy of 10 IS a tie"""
    e = post_f64.vad_tie_energies()
    assert e.dtype == np.float32 and e.shape == (256,)
    total = np.sum(e.astype(np.float64))
    assert total == 2560.0 and np.float32(total) == 2560.0
    thr = np.float32(5.0) + np.float32(0.5) * np.float32(total) / np.float32(256)
    assert thr.dtype == np.float32 and thr == 10.0
    assert np.count_nonzero(e == 10.0) == 10 and e[2] == 10.0 and e[253] != 10.0 and e[252] == 10.0
    # every partial sum, in any order, is a multiple of 1/4 below 2^24: exact in double
    assert np.all(np.cumsum(e[::-1].astype(np.float64)) * 4 % 1 == 0)


@pytest.mark.parametrize('ctx, p', lay.VAD_TIES)
def test_vad_ties(ctx, p):
    """`>` is strict: a frame exactly on the threshold does not count; `>=` is not: num == den x p is voiced"""
    mats = post_f64.vad_tie_batch(13)
    e = mats[1][:, 0]
    want, inside, gap = post_f64.vad_want(e, ctx, 0.5, p, 5.0, threshold=10.0)
    assert inside == 0 and gap == 0.0
    assert np.array_equal(orc.vad_energy(mats[1], 5.0, 0.5, ctx, p), want.astype(np.float32))
    on = np.flatnonzero(e == 10.0)
    above = np.concatenate([[0], np.cumsum(e.astype(np.float64) > 10.0)])
    t = np.arange(256)
    lo, hi = np.maximum(t - ctx, 0), np.minimum(t + ctx + 1, 256)
    num, den = above[hi] - above[lo], hi - lo
    if ctx == 0:
        assert np.all(want[on] == 0.0) and np.array_equal(want, (e > 10.0).astype(np.float64))
    if (ctx, p) == (2, 0.6):
        ties = np.flatnonzero((den == 5) & (num == 3))
        assert ties.size >= 10 and np.all(want[ties] == 1.0)
        # ... which a float64 product 5 x 0.6f = 3.00000012 refuses
        assert np.all(_spec_flags(e, ctx, 0.5, p, 5.0)[ties] == 0.0)
        # and with `>=` in place of `>` some tie frame would have changed a decision
        loose = np.concatenate([[0], np.cumsum(e.astype(np.float64) >= 10.0)])
        assert np.any(((loose[hi] - loose[lo]) >= 3) != (num >= 3))
    if (ctx, p) == (2, 0.25):
        assert den[1] == 4 and num[1] == 1 and want[1] == 1.0
        assert den[254] == 4 and num[254] == 1 and want[254] == 1.0
        assert np.array_equal(want, _spec_flags(e, ctx, 0.5, p, 5.0))     # 0.25 den is exact either way
    # the other utterances of the batch are decided too
    for u in (0, 3):
        assert post_f64.vad_want(mats[u][:, 0], ctx, 0.5, p, 5.0)[1] == 0


# ---- sliding-window CMVN --------------------------------------------------------------------------------------------
SLIDING_CASES, sliding_id = lay.SLIDING_CASES, lay.sliding_id


def test_sliding_layouts():
    for cmn, minw in lay.SLIDING_WINDOWS:
        lengths = lay.check_sliding(lay.sliding_lengths(cmn, minw), cmn, minw)
        with pytest.raises(ValueError):
            lay.check_sliding(lengths[1:], cmn, minw)
        with pytest.raises(ValueError):
            lay.check_sliding([n for n in lengths if n != cmn + 1], cmn, minw)
        shapes = {cols: lay.sliding_threads(lengths, cols) for cols in lay.SLIDING_COLS}
        assert shapes[1][1] == 1 and shapes[13][3] and shapes[257][3]        # a boundary inside a wave
        assert shapes[64][1] == len(lengths) and not shapes[64][3]           # one workgroup per utterance
        assert shapes[257][1] > 64 // 2
        five = lay.sliding_five(cmn, minw)
        assert len(five) == 5 and min(five) > 0
        assert lay.sliding_threads(five, 13)[:3] == (65, 2, 1)               # the last thread alone in workgroup 1
    assert {w for w in lay.SLIDING_WINDOWS if w[0] % 2} == {(41, 10), (7, 50)}
    assert max(lay.sliding_lengths(600, 100)) < 2 * 600 + 6 and (7, 50) in lay.SLIDING_WINDOWS


@pytest.mark.parametrize('cmn, minw', lay.SLIDING_WINDOWS + [(1, 1), (2, 1)])
@pytest.mark.parametrize('center', [True, False])
def test_sliding_windows_restated(cmn, minw, center):
    """`sliding_windows` gives the windows of spec_f64.sliding_cmvn (the same results bit for bit when formed from
    them), every window holds its frame, and from one frame to the next both ends stay or move on by ONE frame:
    what Kaldi asserts, and what the incremental sums of the kernel and of the C oracle silently rely on"""
    lengths = sorted(set(lay.sliding_lengths(max(cmn, 3), max(minw, 2)) + lay.sliding_five(cmn, minw)))
    rng = np.random.default_rng(3)
    for n in lengths:
        if n == 0 or n > 200:
            continue
        ws, we = post_f64.sliding_windows(n, center, cmn, minw)
        assert np.all(np.diff(ws) >= 0) and np.all(np.diff(ws) <= 1), (n, ws)
        assert np.all(np.diff(we) >= 0) and np.all(np.diff(we) <= 1), (n, we)
        assert ws[0] == 0 and we[-1] == n and np.all(ws <= np.arange(n)) and np.all(we > np.arange(n))
        assert np.all(we - ws <= (cmn if center else max(cmn + 1, minw)))
        x = rng.standard_normal((n, 2))
        direct = np.stack([x[t] - x[ws[t]:we[t]].mean(axis=0) for t in range(n)])
        assert np.array_equal(direct, spec_f64.sliding_cmvn(x, center, cmn, minw, False))


@functools.lru_cache(maxsize=None)
def _sliding_reference(cmn, minw, center, nv, which):
    lengths = lay.sliding_lengths(cmn, minw) if which == 'all' else lay.sliding_five(cmn, minw)
    mats = post_f64.sliding_batch(lengths, post_f64.SLIDING_MAX_COLS)
    return mats, [post_f64.sliding_want(m, center, cmn, minw, nv) for m in mats]


@pytest.mark.parametrize('case', SLIDING_CASES, ids=sliding_id)
def test_sliding_bound_is_met_by_the_oracle(case):
    (cmn, minw), center, nv = case
    for which in ('all', 'five'):
        mats, wants = _sliding_reference(cmn, minw, center, nv, which)
        got = [orc.sliding_cmn(m, center, cmn, minw, nv) for m in mats]
        ratio, u, row, col = post_f64.sliding_ratio(got, wants)
        print(f'sliding oracle {sliding_id(case)} {which}: worst error / bound {ratio:.3f} '
              f'(utterance {u}, row {row}, column {col})')
        assert ratio <= 1.0
        # the bound is tight enough to see one float32 ulp: 2^-24 |want| is all of it but a few 1e-9
        big = np.concatenate([np.abs(w).ravel() for w, _ in wants if w.size])
        bnd = np.concatenate([b.ravel() for _, b in wants if b.size])
        keep = big > 1e-3
        assert np.median(bnd[keep] / big[keep]) < 1.01 * post_f64.U24
        # a narrower batch is the first columns of this one: the same statement serves it
        lengths = [m.shape[0] for m in mats]
        for cols in (1, 13, 64):
            for m, n in zip(post_f64.sliding_batch(lengths, cols), mats):
                assert np.array_equal(m, n[:, :cols])


def _sliding_incremental(x, center, cmn, minw, nv, skip_drop=False):
    """the kernel's walk over one column block in numpy doubles; `skip_drop`: the mutant that never takes the frame
    that left the window out of the sums"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    ws, we = post_f64.sliding_windows(n, center, cmn, minw)
    out = np.zeros_like(x)
    s = q = None
    for t in range(n):
        if t == 0:
            s, q = x[ws[0]:we[0]].sum(axis=0), (x[ws[0]:we[0]] ** 2).sum(axis=0)
        else:
            if ws[t] > ws[t - 1] and not skip_drop:
                s, q = s - x[ws[t - 1]], q - x[ws[t - 1]] ** 2
            if we[t] > we[t - 1]:
                s, q = s + x[we[t - 1]], q + x[we[t - 1]] ** 2
        wf = float(we[t] - ws[t])
        r = x[t] - s / wf
        if nv:
            r = np.zeros_like(r) if wf == 1 else r * np.maximum(q / wf - (s / wf) ** 2, 1e-10) ** -0.5
        out[t] = r
    return out.astype(np.float32)


@pytest.mark.parametrize('nv', [False, True])
def test_sliding_bound_tells_the_mutant(nv):
    """the restated walk meets the bound; without the `ws > last_start` update it misses it as soon as the window
    has moved - in every utterance longer than the window, and in none that the window covers whole"""
    (cmn, minw), center = (40, 40), True
    mats, wants = _sliding_reference(cmn, minw, center, nv, 'all')
    good = [_sliding_incremental(m, center, cmn, minw, nv) for m in mats]
    assert post_f64.sliding_ratio(good, wants)[0] <= 1.0
    for u, (m, want) in enumerate(zip(mats, wants)):
        bad = _sliding_incremental(m, center, cmn, minw, nv, skip_drop=True)
        ratio = post_f64.sliding_ratio([bad], [want])[0]
        assert (ratio > 1e3) == (m.shape[0] > cmn), (u, m.shape[0], ratio)


def test_sliding_constant_columns_on_the_oracle():
    """A constant column's sums are exact, and the float64 statement gives exactly 0.  Kaldi's arithmetic, which the
    C oracle follows, does not for every window length: x + fl(-1 / wf) (wf x) leaves one rounding of -1 / wf behind
    whenever wf x fl(1 / wf) is not 1 to the last bit (49 is the first such length; with a fused multiply-add every
    length that is not a power of two), and the variance floor 1e-10 scales that residue by 1e5.  The residue is
    within the derived bound, which is what is asserted of the oracle here.  The kernel forms x - S / wf, one
    correctly rounded quotient of the exact sum, and the GPU module asserts the exact zero of it."""
    assert 3.25 + (-1.0 / 49.0) * (49.0 * 3.25) != 0.0 and 3.25 + (-1.0 / 40.0) * (40.0 * 3.25) == 0.0
    worst = {}
    for cmn, minw in lay.SLIDING_WINDOWS:
        mats = post_f64.sliding_constant_batch(lay.sliding_lengths(cmn, minw))
        for center in (True, False):
            for nv in (False, True):
                wants = [post_f64.sliding_want(m, center, cmn, minw, nv) for m in mats]
                for m, (want, _) in zip(mats, wants):
                    assert not np.any(want[:, [0, 2]])         # the statement: exactly 0
                got = [orc.sliding_cmn(m, center, cmn, minw, nv) for m in mats]
                assert post_f64.sliding_ratio(got, wants)[0] <= 1.0
                size = max(float(np.abs(g[:, [0, 2]]).max()) for g in got if g.size)
                worst[nv] = max(worst.get(nv, 0.0), size)
                for g, m in zip(got, mats):
                    if m.shape[0] == 1 and nv:
                        assert not np.any(g)                   # wf == 1: the literal 0
    print(f'sliding oracle, constant columns: largest |result| {worst[False]:.3g} (mean), {worst[True]:.3g} (variance)')
    assert worst[False] < 1e-14 and worst[True] < 1e-9


# ---- column concatenation -------------------------------------------------------------------------------------------
def test_concat_layout():
    out, a, b = lay.check_concat(*lay.concat_layout())
    found = lay.seams(out, lay.CONCAT_ROWS)
    assert all(found.values()) and len(found) == 17, found
    assert lay.CONCAT_ROWS == 32 and 5 * 32 < sum(out) < 6 * 32
    with pytest.raises(ValueError, match='drifting'):
        lay.check_concat(out, out, out)
    with pytest.raises(ValueError, match='shorter'):
        lay.check_concat(out, [max(n - 1, 0) for n in out], b)
    kinds = {(32 * (ca + cb)) % 256 == 0 for ca, cb in lay.CONCAT_COLS}
    assert kinds == {True, False}
    assert (13, 3) in lay.CONCAT_COLS and max(max(c) for c in lay.CONCAT_COLS) > 256


def _concat_restated(a_flat, ca, off_a, b_flat, cb, off_b, off_o, row_shift=0):
    """concat_columns_kernel's indexing in numpy: per output row its utterance, the row's start in a and in b (the
    latter less ca: indexed with the output column), then element i of the 32-row tile; `row_shift`: the mutant
    that reads the LDS record of a neighbouring row"""
    total, co = int(off_o[-1]), ca + cb
    out = np.zeros(total * co, np.float32)
    af, bf = a_flat.ravel(), b_flat.ravel()
    for row0 in range(0, total, lay.CONCAT_ROWS):
        rows = min(lay.CONCAT_ROWS, total - row0)
        g = row0 + np.arange(rows)
        u = np.searchsorted(off_o, g, side='right') - 1
        t = g - off_o[u]
        row_a, row_b = (off_a[u] + t) * ca, (off_b[u] + t) * cb - ca
        for i in range(rows * co):
            r, c = divmod(i, co)
            r = min(max(r + row_shift, 0), rows - 1)
            out[row0 * co + i] = af[row_a[r] + c] if c < ca else bf[row_b[r] + c]
    return out.reshape(total, co)


@pytest.mark.parametrize('ca, cb', [(1, 1), (13, 3), (3, 13)])
def test_concat_statement_tells_the_mutant(ca, cb):
    rows_out, rows_a, rows_b = lay.concat_layout()
    a, b = post_f64.concat_inputs(rows_a, rows_b, ca, cb)
    want = np.concatenate(post_f64.concat_want(a, b, rows_out))
    offs = [lay.offsets_of(r) for r in (rows_a, rows_b, rows_out)]
    a_flat, b_flat = np.concatenate(a), np.concatenate(b)
    got = _concat_restated(a_flat, ca, offs[0], b_flat, cb, offs[1], offs[2])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    bad = _concat_restated(a_flat, ca, offs[0], b_flat, cb, offs[1], offs[2], row_shift=1)
    assert not np.array_equal(bad.view(np.uint32), want.view(np.uint32))
    # every element is distinct, the special values are there and survive as bits
    bits = want.view(np.uint32).ravel()
    assert np.unique(bits).size >= bits.size - 2 * len(post_f64.SPECIAL_BITS)
    both = np.concatenate([a_flat.view(np.uint32).ravel(), b_flat.view(np.uint32).ravel()])
    assert set(post_f64.SPECIAL_BITS) <= set(both.tolist())


# ---- non-finite count -----------------------------------------------------------------------------------------------
def test_nonfinite_sizes():
    """launch_count_nonfinite restated.  4 x 256 x 4096 + 3 floats fill the capped grid exactly once - every thread
    reads one vector - so the second pass of the stride loop needs a larger size: NONFINITE_SECOND_PASS"""
    assert lay.NONFINITE_GRID + 3 == 4194307 and lay.NONFINITE_GRID + 3 in lay.NONFINITE_SIZES
    assert lay.nonfinite_launch(4194307) == (4096, 1048576, 1, 3)
    blocks, n4, passes, tail = lay.nonfinite_launch(lay.NONFINITE_SECOND_PASS)
    assert (blocks, passes, tail) == (4096, 2, 3) and n4 - blocks * 256 == 257      # workgroup 0 whole, 1 lane of 1
    assert [lay.nonfinite_launch(n)[1:] for n in (1, 2, 3)] == [(0, 0, 1), (0, 0, 2), (0, 0, 3)]
    assert [lay.nonfinite_launch(n)[3] for n in (4, 5, 7, 1024, 1025, 1027)] == [0, 1, 3, 0, 1, 3]
    places = lay.nonfinite_places(lay.NONFINITE_SECOND_PASS)
    assert 4 * 4096 * 256 in places and 4 * (4096 * 256 + 256) in places and places[-3:] == [4195332, 4195333, 4195334]
    assert lay.nonfinite_places(7) == [0, 3, 4, 5, 6] and lay.nonfinite_places(3) == [0, 1, 2]


def _exponent_test(x, tail=True):
    """count_nonfinite_kernel's test in numpy: an exponent field of all ones; `tail=False`: the mutant without the
    0 - 3 floats behind the vector body"""
    bits = np.asarray(x, np.float32).view(np.uint32)
    if not tail:
        bits = bits[:bits.shape[0] & ~3]
    return int(np.count_nonzero((bits & 0x7F800000) == 0x7F800000))


def test_nonfinite_kinds():
    bad = np.array(list(post_f64.NONFINITE_BITS.values()), np.uint32).view(np.float32)
    fine = np.array(list(post_f64.FINITE_BITS.values()), np.uint32).view(np.float32)
    assert post_f64.nonfinite_count(bad) == bad.size == 7 and post_f64.nonfinite_count(fine) == 0
    assert _exponent_test(bad) == 7 and _exponent_test(fine) == 0
    assert np.isnan(bad[2:]).all() and np.isinf(bad[:2]).all() and np.signbit(bad[4])
    assert fine[0] == np.finfo(np.float32).max and fine[1] == -fine[0] and fine[3] < np.finfo(np.float32).tiny
    for n in (1, 3, 7, 1027):
        x = post_f64.finite_fill(n)
        assert _exponent_test(x) == 0
        for k in lay.nonfinite_places(n):
            y = x.copy()
            y[k] = np.inf
            assert _exponent_test(y) == 1 == post_f64.nonfinite_count(y)
            assert _exponent_test(y, tail=False) == (1 if k < (n & ~3) else 0)


# ---- MFCC DCT tail --------------------------------------------------------------------------------------------------
def test_mfcc_dct_launch_restated():
    """launch_mfcc_dct: as many waves as 64-row tiles (rows of odd pitch + 17 floats of outgoing cepstra) fit beside
    the matrix in 159 KiB - 10 for 40 bins (14 before the outgoing tile shared the LDS), 5 for 80 bins - and at most
    256 workgroups"""
    assert lay.mfcc_dct_launch(40, 40, True, 1)[:2] == (10, 640)
    assert lay.mfcc_dct_launch(40, 40, False, 1)[:2] == (10, 640)
    assert lay.mfcc_dct_launch(80, 40, True, 1)[:2] == (5, 320)
    for opts, copies in lay.MFCC_FIRST:
        frames = copies * lay.MFCC_UTT_FRAMES
        waves, per_group, blocks, per_wave = lay.mfcc_dct_launch(opts['num_bins'], opts['num_ceps'],
                                                                 lay.mfcc_energy(opts), frames)
        assert waves == (10 if opts['num_bins'] == 40 else 5)
        assert per_group < frames < per_group + 2 * lay.MFCC_UTT_FRAMES and blocks == 2 and per_wave == 1
    opts, copies = lay.MFCC_BIG
    frames = copies * lay.MFCC_BIG_FRAMES
    waves, per_group, blocks, per_wave = lay.mfcc_dct_launch(80, 40, True, frames)
    assert (waves, blocks, per_wave) == (5, 256, 2) and 256 * per_group == 81920 < frames - lay.MFCC_BIG_FRAMES
    # the last copy lies wholly in tiles of the second pass, and no utterance is a whole number of tiles
    assert (copies - 1) * lay.MFCC_BIG_FRAMES >= 81920 and lay.MFCC_BIG_FRAMES % 64 and lay.MFCC_UTT_FRAMES % 64
    assert lay.MFCC_UTT_SAMPLES == 12560 and lay.MFCC_BIG_SAMPLES == 26640
    # htk: column 0 goes last; with 17, 24 and 33 cepstra the last column is in another 16-cepstrum chunk than column 0
    assert {o['num_ceps'] for o, _ in lay.MFCC_FIRST if o.get('htk_compat')} >= {17, 24, 33}


@pytest.mark.parametrize('case', lay.MFCC_FIRST + [lay.MFCC_BIG], ids=lay.mfcc_id)
def test_mfcc_dct_bound_is_met_by_the_oracle(case):
    """the oracle's cepstra against the float64 DCT of the oracle's own float32 filterbank rows"""
    opts, _ = case
    wave = post_f64.mfcc_wave(big='frame_shift' in opts)
    proc = MfccProcessor(dither=0, **opts)
    rows = orc.compute(FilterbankProcessor(dither=0, **lay.fbank_options(opts))._build_options(), wave)
    got = orc.compute(proc._build_options(), wave)
    frames = lay.MFCC_BIG_FRAMES if 'frame_shift' in opts else lay.MFCC_UTT_FRAMES
    assert got.shape == (frames, opts['num_ceps']) and rows.shape == (frames, opts['num_bins'] + lay.mfcc_energy(opts))
    want, bound = post_f64.mfcc_dct_want(rows, opts['num_bins'], opts['num_ceps'], opts.get('cepstral_lifter', 22.0),
                                         lay.mfcc_energy(opts), opts.get('htk_compat', False))
    err = np.abs(got.astype(np.float64) - want)
    ratio = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)))
    print(f'mfcc_dct oracle {lay.mfcc_id(case)}: worst error / bound {ratio:.3f}')
    assert ratio <= 1.0
    if lay.mfcc_energy(opts):
        col = opts['num_ceps'] - 1 if opts.get('htk_compat') else 0
        assert np.array_equal(got[:, col], rows[:, 0])
    # the statement is spec_f64's: the same rules on the same rows
    assert post_f64.mfcc_dct_k(40) == 46 and post_f64.mfcc_dct_k(80) == 86


def test_mfcc_dct_want_follows_spec_f64():
    """DCT, lifter, c0 and htk rules of spec_f64.features, applied to ITS log-mel energies"""
    wave = post_f64.mfcc_wave().astype(np.float64)
    for opts, _ in lay.MFCC_FIRST:
        args = dict(num_bins=opts['num_bins'], num_ceps=opts['num_ceps'], use_energy=lay.mfcc_energy(opts),
                    cepstral_lifter=opts.get('cepstral_lifter', 22.0), htk_compat=opts.get('htk_compat', False))
        rows = spec_f64.features(wave, kind='fbank', num_bins=opts['num_bins'], use_energy=lay.mfcc_energy(opts))
        want, _ = post_f64.mfcc_dct_want(rows, args['num_bins'], args['num_ceps'], args['cepstral_lifter'],
                                         args['use_energy'], args['htk_compat'])
        np.testing.assert_allclose(want, spec_f64.features(wave, kind='mfcc', **args), rtol=1e-12, atol=1e-12)


def test_mfcc_utterances_suit_the_oracle():
    """the device's cepstra of an utterance alone are compared with the float32 oracle at the family tolerance of
    conftest.py; that asks for an utterance on which the oracle itself is within that tolerance of the float64
    statement.  The 77-frame utterance is, for every case; of the twenty 821-frame candidates the big batch uses the
    one on which the oracle is closest to the statement"""
    from conftest import FAMILY_ATOL
    small = post_f64.mfcc_wave()
    for opts, _ in lay.MFCC_FIRST:
        excess = post_f64.mfcc_oracle_excess(orc.compute, MfccProcessor(dither=0, **opts)._build_options(), small, opts)
        assert excess <= FAMILY_ATOL['mfcc'], (opts, excess)
    opts, _ = lay.MFCC_BIG
    options = MfccProcessor(dither=0, **opts)._build_options()
    excess = {i: post_f64.mfcc_oracle_excess(orc.compute, options, post_f64.mfcc_wave(True, i), opts)
              for i in lay.MFCC_BIG_CANDIDATES}
    print('mfcc oracle, 821 frames of 80 bins: absolute term the oracle itself needs, per candidate',
          ' '.join(f'{i}:{e:.2g}' for i, e in excess.items()))
    assert min(excess, key=excess.get) == lay.MFCC_BIG_ID and excess[lay.MFCC_BIG_ID] <= FAMILY_ATOL['mfcc']
    assert sum(e > FAMILY_ATOL['mfcc'] for e in excess.values()) > len(excess) // 2
