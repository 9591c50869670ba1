"""Float64 statements and derived error bounds of the delta, pitch-post and CMVN kernels, shared by
test_post_routes.py (the float32 C oracle must meet them on the CPU) and test_post_routes_gpu.py (every launch
route of the HIP kernels must).  Nothing here is tuned on what the kernels give:

delta       |got - want| <= K 2^-24 A, per element, where want is oracle/spec_f64.py `delta` (float64 scales), A the
            sum of |scale| |input| over the clamped taps and K = taps + roundings + 1 (`delta_k`).
CMVN sums   want is the exactly rounded sum (math.fsum) of the float32 products x w and (x x) w;
            |got - want| <= n 2^-53 sum |terms| for n terms: n - 1 additions in any order, one rounding of want.
CMVN apply  the statement's scale and offset (spec_f64.cmvn_apply at 0 and 1) rounded to float32, the product and
            the sum rounded once each as cmvn_apply_kernel states; 2 ulp of the result + 1 ulp of the offset.
pitch post  no derived bound for logf / exp / pow on the device: per output column 4 times the largest error of
            the float32 C oracle against oracle/spec_f64.py `process_pitch`, the rule of test_bottleneck_gpu.py and
            test_crepe_gpu.py (and the family tolerance of conftest.py against the oracle).

The second half of the file holds the same for the kernels those tests left out - VAD, sliding-window CMVN, column
concatenation, the non-finite count and the MFCC DCT tail (test_post_remaining.py, test_post_remaining_gpu.py): see
the comment in front of it."""

import math

import numpy as np

from oracle import spec_f64

U24 = 2.0 ** -24
U53 = 2.0 ** -53


def inputs(rng, lengths, cols, scale=3.0, offset=10.0):
    """float32 [n, cols] per utterance, like tests/tools/fuzz_post.py `feats_of`"""
    return [(rng.standard_normal((int(n), cols)) * scale + offset).astype(np.float32) for n in lengths]


def pitch_inputs(rng, lengths):
    """raw pitch rows per utterance: NCCF uniform in [-1, 1], pitch uniform in [50, 400] Hz"""
    return [np.stack([rng.uniform(-1, 1, int(n)), rng.uniform(50, 400, int(n))], axis=1).astype(np.float32)
            for n in lengths]


# ---- delta ----------------------------------------------------------------------------------------------------
def delta_scale_roundings(i, window):
    """float32 roundings behind one scale of order i in make_delta_scales (host_tables.cpp), counted from its
    loops and at most: every order convolves the previous one with [-window .. window] - 2 window + 1 products
    `float(j) * prev[k]` and as many additions `cur[..] +=` per entry -, rounds `s = float(1 / normalizer)` once
    (the normaliser itself is a sum of small integers: exact) and multiplies every entry by it once.  That is
    2 (2 window + 1) + 2 = 4 window + 4 per order, on top of the roundings of the order below; order 0 is the
    literal 1."""
    return i * (4 * window + 4)


def delta_k(i, window):
    """K of the bound for block i: the 2 i window + 1 taps of the dot product (one product and one addition
    less than taps, with or without contraction to FMA), the roundings of its scales, and 1 for the higher-order
    terms of (1 + 2^-24)^K"""
    return (2 * i * window + 1) + delta_scale_roundings(i, window) + 1


def delta_want(x, order, window):
    """(want, bound) for one utterance x float32 [n, d]: float64 [n, d (order + 1)] each"""
    x64 = np.asarray(x, dtype=np.float64)
    n = x64.shape[0]
    want = spec_f64.delta(x64, order, window)
    bounds = []
    for i, s in enumerate(spec_f64.delta_scales(order, window)):
        half = (len(s) - 1) // 2
        a = np.zeros_like(x64)
        for k, c in enumerate(s):
            a += abs(c) * np.abs(x64[np.clip(np.arange(n) + k - half, 0, max(n - 1, 0))])
        bounds.append(delta_k(i, window) * U24 * a)
    return want, np.concatenate(bounds, axis=1)


def delta_ratio(got, mats, order, window):
    """largest |got - want| / bound over a batch (0 where both vanish), and where: (ratio, utterance, row, column)"""
    worst = (0.0, -1, -1, -1)
    for u, (g, x) in enumerate(zip(got, mats)):
        want, bound = delta_want(x, order, window)
        assert g.shape == want.shape, (u, g.shape, want.shape)
        if not g.size:
            continue
        err = np.abs(np.asarray(g, dtype=np.float64) - want)
        ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
        k = int(np.argmax(ratio))
        if ratio.flat[k] > worst[0]:
            worst = (float(ratio.flat[k]), u, k // g.shape[1], k % g.shape[1])
    return worst


# ---- CMVN -----------------------------------------------------------------------------------------------------
def cmvn_weights(rng, n):
    """weights in [0, 2) that are multiples of 1/64, about one in five exactly zero: their sum is exact in double"""
    w = rng.integers(0, 128, int(n)).astype(np.float32) / np.float32(64)
    w[rng.random(int(n)) < 0.2] = 0.0
    return w


def cmvn_terms(x, w=None):
    """the float32 products the kernels sum: (x w, (x x) w), rows of weight zero left out, and the count"""
    x = np.asarray(x, dtype=np.float32)
    if w is None:
        w = np.ones(x.shape[0], dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    keep = w != 0
    x, w = x[keep], w[keep][:, None]
    return x * w, (x * x) * w, float(np.sum(w, dtype=np.float64))


def cmvn_want(x, w=None):
    """(want, bound) [2, d + 1] of one utterance: exactly rounded sums, n 2^-53 sum |terms| (count: exact, bound 0)"""
    s, q, count = cmvn_terms(x, w)
    d, n = s.shape[1], s.shape[0]
    want, bound = np.zeros((2, d + 1)), np.zeros((2, d + 1))
    for row, terms in enumerate((s, q)):
        t64 = terms.astype(np.float64)
        want[row, :d] = [math.fsum(col) for col in t64.T.tolist()] if n else 0.0
        bound[row, :d] = n * U53 * np.abs(t64).sum(axis=0)
    want[0, d] = count
    return want, bound


def cmvn_apply_want(x, stats, norm_vars, reverse):
    """(want, tolerance) float32 / float64 [n, d]: the statement's affine map through the kernel's two roundings.
    Without variance normalisation the host forms the offset as float(-1 / count) * sum (Kaldi's AddVec takes a
    BaseFloat alpha), one ulp of the offset away from the statement's -mean: where the result is near zero that ulp
    is the whole tolerance, and the measured ratio is 1."""
    x = np.asarray(x, dtype=np.float32)
    d = x.shape[1]
    offset = spec_f64.cmvn_apply(np.zeros((1, d)), stats, norm_vars=norm_vars, reverse=reverse)[0]
    scale = spec_f64.cmvn_apply(np.ones((1, d)), stats, norm_vars=norm_vars, reverse=reverse)[0] - offset
    fo, fs = offset.astype(np.float32), scale.astype(np.float32)
    scaled = x * fs if norm_vars else x
    want = scaled + fo
    tol = 2.0 * np.spacing(np.abs(want)).astype(np.float64) + np.spacing(np.abs(fo)).astype(np.float64)
    return want, tol


# ---- pitch post -----------------------------------------------------------------------------------------------
def pitch_statement(proc, raw):
    """oracle/spec_f64.py `process_pitch` with the options of a KaldiPitchPostProcessor"""
    return spec_f64.process_pitch(
        raw, pitch_scale=proc.pitch_scale, pov_scale=proc.pov_scale, pov_offset=proc.pov_offset,
        delta_pitch_scale=proc.delta_pitch_scale, left_context=proc.normalization_left_context,
        right_context=proc.normalization_right_context, delta_window=proc.delta_window,
        add_pov_feature=proc.add_pov_feature, add_normalized_log_pitch=proc.add_normalized_log_pitch,
        add_delta_pitch=proc.add_delta_pitch, add_raw_log_pitch=proc.add_raw_log_pitch)


def column_errors(rows, wants):
    """largest |rows - wants| per column over a batch of utterances"""
    errs = [np.abs(np.asarray(r, dtype=np.float64) - w).max(axis=0) for r, w in zip(rows, wants) if r.shape[0]]
    return np.max(errs, axis=0)


# ---- the inputs of a case, the same in both test modules --------------------------------------------------------
def delta_batch(cols, layout, seed=11):
    return inputs(np.random.default_rng([seed, cols, len(layout), int(sum(layout))]), layout, cols)


def pitch_batch(layout, seed=12):
    return pitch_inputs(np.random.default_rng([seed, len(layout), int(sum(layout))]), layout)


def cmvn_batch(cols, lengths, setting, seed=13):
    """(mats, weights): weights None, or per utterance; 'one_utterance_all_zero' zeroes those of utterance 4"""
    rng = np.random.default_rng([seed, cols])
    mats = inputs(rng, lengths, cols)
    if setting == 'none':
        return mats, None
    weights = [cmvn_weights(rng, n) for n in lengths]
    if setting == 'one_utterance_all_zero':
        weights[4][:] = 0.0
    return mats, weights


# =====================================================================================================================
# The remaining kernels of the path: VAD, sliding-window CMVN, column concatenation, the non-finite count and the
# MFCC DCT tail (test_post_remaining.py on the CPU, test_post_remaining_gpu.py on the device)
#
# VAD         flags are compared for equality.  The statement is oracle/spec_f64.py `vad_energy` with Kaldi's
#             BaseFloat arithmetic where a decision depends on it (`vad_want`); a frame whose energy lies within
#             the rounding of the threshold cannot be decided by a float64 statement: the band is derived in
#             `vad_band`, and the seeds are such that no frame lies in it.
# sliding     |got - want| <= 2^-24 |want| + K 2^-53 A s against spec_f64.sliding_cmvn, which forms every window
#             directly: `sliding_want`.
# concat      np.concatenate([a[u][:r], b[u][:r]], axis=1), bit for bit.
# non-finite  np.count_nonzero(~np.isfinite(x)), exactly.
# MFCC DCT    |got - want| <= K 2^-24 sum |dct| |lifter| |x| against the float64 DCT of the float32 log-mel rows:
#             `mfcc_dct_want`.
# =====================================================================================================================

# ---- VAD ------------------------------------------------------------------------------------------------------------
def vad_band(energy, energy_threshold, energy_mean_scale):
    """(threshold in float64, half-width of the band around it in which a float32 implementation may decide either
    way).  vad_threshold_kernel (and Kaldi's ComputeVadEnergy, in BaseFloat) forms

        threshold = energy_threshold + energy_mean_scale * float(sum) / float(T)

    with `sum` accumulated in double: four float32 roundings - float(sum), the product, the quotient and the sum -,
    each of a quantity of magnitude at most |energy_threshold| + |energy_mean_scale mean|, so at most
    4 x 2^-24 of that.  The double sum of T float32 energies adds T 2^-53 sum |e| / T x scale: the order of the
    additions (a tree on the device, a loop in the oracle) is inside it."""
    e = np.asarray(energy, dtype=np.float64)
    n = e.shape[0]
    et, scale = float(np.float32(energy_threshold)), float(np.float32(energy_mean_scale))
    if n == 0 or scale == 0.0:
        return et, 0.0     # (the threshold is the float32 option itself: no rounding, no band)
    mean = math.fsum(e.tolist()) / n
    band = 4 * U24 * (abs(et) + abs(scale * mean)) + n * U53 * float(np.abs(e).sum()) / n * abs(scale)
    return et + scale * mean, band


def vad_want(energy, frames_context, energy_mean_scale, proportion_threshold, energy_threshold, threshold=None):
    """(flags float64 [n], number of frames inside the band, smallest |energy - threshold|).

    oracle/spec_f64.py `vad_energy`, with Kaldi's BaseFloat arithmetic in the one place where it decides: a frame
    is voiced when float(num) >= float(den) * proportion_threshold, where proportion_threshold is the float32
    value of the option and the product is ROUNDED TO FLOAT32 (`BaseFloat` in ComputeVadEnergy, `float` in
    vad_kernel).  spec_f64.vad_energy forms the product in float64: with the option 0.6 and den = 5 the float32
    product is 3 exactly (0.6f = 0.6 + 2.4e-8, 5 x 0.6f = 3 + 1.19e-7 lies half way between two float32 values
    and rounds to the even one), so 3 frames of 5 are enough for Kaldi and not for a float64 product.
    `threshold`: given by the caller when it is known exactly (the tie cases)."""
    e = np.asarray(energy, dtype=np.float64)
    n = e.shape[0]
    if n == 0:
        return np.zeros(0), 0, np.inf
    if threshold is None:
        threshold, band = vad_band(e, energy_threshold, energy_mean_scale)
    else:
        band = 0.0
    gap = np.abs(e - threshold)
    inside = int(np.count_nonzero(gap <= band)) if band > 0 else 0
    above = np.concatenate([[0], np.cumsum(e > threshold)])
    t = np.arange(n)
    lo, hi = np.maximum(t - frames_context, 0), np.minimum(t + frames_context + 1, n)
    num, den = above[hi] - above[lo], hi - lo
    limit = den.astype(np.float32) * np.float32(proportion_threshold)     # float32 x float32 -> float32
    assert limit.dtype == np.float32
    return (num.astype(np.float32) >= limit).astype(np.float64), inside, float(gap.min())


def vad_batch(cols, lengths, seed=21):
    """float32 [n, cols] per utterance.  Column 0 is the energy, normal around 10 with deviation 3 (the default
    threshold 5 + 0.5 mean is 10: about half of the frames lie above it); every other column is the energy
    mirrored at 10 plus noise - read in place of column 0 it turns nearly every decision round.  The energies do
    not depend on `cols`."""
    rng = np.random.default_rng([seed, len(lengths), int(sum(lengths))])
    energies = [(rng.standard_normal(int(n)) * 3.0 + 10.0).astype(np.float32) for n in lengths]
    other = np.random.default_rng([seed, cols])
    mats = []
    for e in energies:
        m = np.empty((e.shape[0], cols), np.float32)
        m[:, 0] = e
        m[:, 1:] = (20.0 - e)[:, None] + other.standard_normal((e.shape[0], cols - 1)).astype(np.float32) * 0.01
        mats.append(m)
    return mats


def vad_tie_energies(seed=22):
    """256 energies, all multiples of 1/4, whose mean is exactly 10: with energy_mean_scale 0.5 and
    energy_threshold 5 every step of the threshold - the sum 2560, float(sum), 0.5 x 2560 = 1280, 1280 / 256 = 5,
    5 + 5 = 10 - is exact in float32 and in double, so the threshold IS 10 and an energy of 10 is a tie.

    frames 0-3     9, 11, 10, 9.5: with a context of 2, frame 1 sees frames 0-3 (den 4 at the utterance's edge)
                   and exactly one of them above (the 10 is not: `>` is strict); 4 x 0.25 = 1
    frames 4-251   eight more energies of exactly 10 and 120 pairs 10 - d, 10 + d, shuffled
    frames 252-255 10, 9.25, 9.25, 12: the same at the other edge (frame 254 sees 252-255, one of them above)"""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 17, 120).astype(np.float64) / 4.0
    middle = np.concatenate([np.full(8, 10.0), 10.0 - d, 10.0 + d])
    rng.shuffle(middle)
    e = np.concatenate([[9.0, 11.0, 10.0, 9.5], middle, [10.0, 9.25, 9.25, 12.0]])
    assert e.shape == (256,) and math.fsum(e.tolist()) == 2560.0 and np.all(e * 4 == np.round(e * 4))
    return e.astype(np.float32)


def vad_tie_batch(cols, seed=22):
    """the tie utterance between two ordinary ones and an empty one, `cols` columns as in `vad_batch`"""
    mats = vad_batch(cols, [37, 256, 0, 300], seed=seed)
    e = vad_tie_energies(seed)
    mats[1][:, 0] = e
    mats[1][:, 1:] = (20.5 - e)[:, None]      # (mirrored off the threshold: a tie in column 0 is none here)
    return mats


# ---- sliding-window CMVN --------------------------------------------------------------------------------------------
def sliding_windows(n, center, cmn_window, min_window):
    """[ws, we) of every frame of an utterance of n frames: Kaldi's SlidingWindowCmnInternal, restated"""
    t = np.arange(n, dtype=np.int64)
    if center:
        ws = t - cmn_window // 2
        we = ws + cmn_window
    else:
        ws, we = t - cmn_window, t + 1
    we = np.where(ws < 0, we - ws, we)
    ws = np.maximum(ws, 0)
    if not center:
        we = np.where(we > t, np.maximum(t + 1, min_window), we)
    over = np.maximum(we - n, 0)
    ws, we = np.maximum(ws - over, 0), we - over
    return ws, we


def sliding_want(x, center, cmn_window, min_window, normalize_variance):
    """(want, bound) float64 [n, d] for one utterance x float32 [n, d]; want is oracle/spec_f64.py `sliding_cmvn`.

    The kernel (and Kaldi) keeps S = sum x and Q = sum x^2 over the window in double and updates them as the window
    moves; for frame t, with window [ws, we) of wf frames,

        r = x_t - S / wf                                             without variance normalisation: the result
        v = max(Q (1 / wf) + (-1 / wf^2) S S, 1e-10),  y = r v^(-1/2)     with it (y = 0 when wf = 1)

    and rounds r (or y) to float32 once: 2^-24 |want|.  In double, with u = 2^-53:

    S     has seen the wf_0 additions of the first window and at most two per later frame: K_S = wf_0 + 2 t
          additions, each with an error of at most u times the sum of |x| over the frames touched so far (frames 0
          to we - 1: the first window starts at frame 0), which we call a: |dS| <= K_S u a.
    r     at most three more roundings - Kaldi and the C oracle form x_t + (-1 / wf) S: the quotient -1 / wf, its
          product with S and the sum; the kernel forms x_t - S / wf: the quotient and the difference -, each of a
          quantity of at most |x_t| + a / wf: |dr| <= K u A with K = K_S + 3 and A = |x_t| + a / wf.
    Q     the squares of float32 values are exact in double; the same count of additions, each with an error of at
          most u q, q the sum of x^2 over the frames touched: |dQ| <= K_S u q.
    v     |dv| <= |dQ| / wf + 2 (a / wf) |dS| / wf + 6 u (q / wf + (a / wf)^2): the two sums' errors, and six
          roundings (1 / wf, its product with Q; -1 / wf^2, its two products with S, the sum; wf wf is exact), each
          of a quantity of at most B = q / wf + (a / wf)^2.  Together |dv| <= K_v u B with K_v = 2 K_S + 6; the
          float64 statement's own v carries a few u B of its own, so K_v = 2 K_S + 10.  The floor is 1-Lipschitz:
          flooring both sides does not increase |dv|.
    y     the sensitivity of r v^(-1/2) to dr is v^(-1/2) and to dv it is |r| v^(-3/2) / 2, both decreasing in v:
          taken at v_low = max(v - |dv|, 1e-10), and |r| at |r| + |dr|, they bound the change rigorously (mean value
          theorem).  pow and the product round y a few times: 8 u |y|.

    bound = 2^-24 |want| + (1 + 2^-24) (K u A s + |r| v_low^(-3/2) / 2 K_v u B + 8 u |y|), s = v_low^(-1/2), or
    s = 1 and the last two terms absent without variance normalisation.  For a column that is constant over the
    window v is 0, the floor makes s = 1e5, and the bound stays K u A 1e5 ~ 1e-8 |x|: round-off of r is allowed
    through, scaled by the floor, and nothing more."""
    x32 = np.asarray(x, dtype=np.float32)
    x64 = x32.astype(np.float64)
    n, d = x64.shape
    want = spec_f64.sliding_cmvn(x64, center=center, cmn_window=cmn_window, min_window=min_window,
                                 normalize_variance=normalize_variance) if n else np.zeros((0, d))
    bound = np.zeros((n, d))
    if n == 0:
        return want, bound
    ws, we = sliding_windows(n, center, cmn_window, min_window)
    wf = (we - ws).astype(np.float64)[:, None]
    assert ws[0] == 0 and np.all(we > ws) and np.all(ws <= np.arange(n)) and np.all(np.arange(n) < we)
    k_s = (we[0] - ws[0]) + 2.0 * np.arange(n)[:, None]
    zero = np.zeros((1, d))
    a = np.concatenate([zero, np.cumsum(np.abs(x64), axis=0)])[we]
    big_a = np.abs(x64) + a / wf
    dr = (k_s + 3.0) * U53 * big_a
    if not normalize_variance:
        return want, U24 * np.abs(want) + (1.0 + U24) * dr
    q = np.concatenate([zero, np.cumsum(x64 * x64, axis=0)])[we]
    big_b = q / wf + (a / wf) ** 2
    dv = (2.0 * k_s + 10.0) * U53 * big_b
    mean, var = np.empty((n, d)), np.empty((n, d))
    for t in range(n):     # every window formed directly, as the statement does
        seg = x64[ws[t]:we[t]]
        mean[t] = seg.mean(axis=0)
        var[t] = np.maximum((seg * seg).mean(axis=0) - mean[t] * mean[t], 1.0e-10)
    r = np.abs(x64 - mean) + dr
    v_low = np.maximum(var - dv, 1.0e-10)
    dy = dr / np.sqrt(v_low) + 0.5 * r * v_low ** -1.5 * dv + 8.0 * U53 * np.abs(want)
    bound = U24 * np.abs(want) + (1.0 + U24) * dy
    bound[(we - ws) == 1] = 0.0       # wf = 1: the result is the literal 0
    return want, bound


def sliding_ratio(got, wants):
    """largest |got - want| / bound over a batch (0 where the error vanishes): (ratio, utterance, row, column)"""
    worst = (0.0, -1, -1, -1)
    for u, (g, (want, bound)) in enumerate(zip(got, wants)):
        assert g.shape == want.shape and g.dtype == np.float32, (u, g.shape, want.shape, g.dtype)
        if not g.size:
            continue
        err = np.abs(g.astype(np.float64) - want)
        ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
        ratio[~np.isfinite(g)] = np.inf
        k = int(np.argmax(ratio))
        if ratio.flat[k] > worst[0]:
            worst = (float(ratio.flat[k]), u, k // g.shape[1], k % g.shape[1])
    return worst


SLIDING_MAX_COLS = 257


def sliding_batch(lengths, cols, seed=23):
    """the first `cols` columns of ONE batch of 257 columns: a column's arithmetic does not depend on its neighbours,
    so one float64 statement of the 257 columns serves every column count"""
    rng = np.random.default_rng([seed, len(lengths), int(sum(lengths))])
    return [np.ascontiguousarray(m[:, :cols]) for m in inputs(rng, lengths, SLIDING_MAX_COLS)]


def sliding_constant_batch(lengths, seed=24):
    """[n, 3] per utterance: column 0 is 3.25 everywhere, column 1 is random, column 2 is constant over each utterance
    ((u + 1) / 2).  Every sum of a constant column is exact in double."""
    rng = np.random.default_rng([seed, len(lengths)])
    mats = []
    for u, n in enumerate(lengths):
        m = np.empty((int(n), 3), np.float32)
        m[:, 0] = 3.25
        m[:, 1] = rng.standard_normal(int(n)) * 3.0 + 10.0
        m[:, 2] = 0.5 * (u + 1)
        mats.append(m)
    return mats


# ---- column concatenation -------------------------------------------------------------------------------------------
SPECIAL_BITS = (0x80000000, 0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x00000000)   # -0, denormals, +0


def concat_inputs(rows_a, rows_b, cols_a, cols_b):
    """(a, b) float32 [rows, cols] per utterance, every element distinct across BOTH: a counts up from the bits of
    1.0, b from the bits of -2.0 (no NaN, no infinity: the rows are far from the exponent's end), and a few elements
    of each are replaced by -0, +0 and denormals, which must survive as bits"""
    def fill(rows, cols, first):
        total = int(sum(rows)) * cols
        bits = (np.arange(total, dtype=np.uint64) + first).astype(np.uint32)
        for k, special in enumerate(SPECIAL_BITS):
            if total:
                bits[(k * 7919 + 3) % total] = special
        flat = bits.view(np.float32).reshape(-1, cols)
        off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        return [flat[s:e] for s, e in zip(off[:-1], off[1:])]
    a, b = fill(rows_a, cols_a, 0x3F800000), fill(rows_b, cols_b, 0xC0000000)
    assert all(np.isfinite(m).all() for m in a + b)
    return a, b


def concat_want(a, b, rows_out):
    """np.concatenate([a[u][:r], b[u][:r]], axis=1) per utterance"""
    return [np.concatenate([x[:r], y[:r]], axis=1) for x, y, r in zip(a, b, rows_out)]


# ---- non-finite count -----------------------------------------------------------------------------------------------
# float32 bit patterns whose exponent field is all ones: they count
NONFINITE_BITS = {'+inf': 0x7F800000, '-inf': 0xFF800000, 'quiet nan': 0x7FC00000, 'signalling nan': 0x7F800001,
                  'negative nan': 0xFFC00000, 'nan, all ones': 0xFFFFFFFF, 'signalling nan, high payload': 0x7FBFFFFF}
# ... and the values next to them, which do not: +-FLT_MAX, the smallest and the largest denormal, +-0,
# the smallest normal value
FINITE_BITS = {'+flt_max': 0x7F7FFFFF, '-flt_max': 0xFF7FFFFF, 'smallest denormal': 0x00000001,
               'largest denormal': 0x007FFFFF, 'negative denormal': 0x807FFFFF, '+0': 0x00000000, '-0': 0x80000000,
               'smallest normal': 0x00800000}


def nonfinite_count(x):
    return int(np.count_nonzero(~np.isfinite(np.asarray(x, dtype=np.float32))))


def finite_fill(n, seed=25):
    """n finite float32 values that walk through the values next to the exponent test"""
    x = np.random.default_rng([seed, n]).standard_normal(n).astype(np.float32)
    fine = np.array(list(FINITE_BITS.values()), dtype=np.uint32).view(np.float32)
    x[::5] = np.resize(fine, x[::5].shape[0])
    assert nonfinite_count(x) == 0
    return x


# ---- MFCC DCT tail --------------------------------------------------------------------------------------------------
def mfcc_wave(big=False, first_id=None):
    """the utterance of the MFCC cases: int16, 77 frames at the default shift, or 821 frames at a shift of 32 samples"""
    import post_layouts as lay
    from shennong_amd import synth
    if first_id is None:
        first_id = lay.MFCC_BIG_ID if big else lay.MFCC_UTT_ID
    return synth.utterances(first_id, 1, lay.MFCC_BIG_SAMPLES if big else lay.MFCC_UTT_SAMPLES)[0]


def mfcc_oracle_excess(compute, proc_options, wave, opts, rtol=1e-4):
    """how far the float32 oracle (`compute(options, wave)`) is from oracle/spec_f64.py `features` beyond
    rtol |want|: the absolute term it would need as its own judge"""
    args = dict(opts)
    args.setdefault('use_energy', True)
    want = spec_f64.features(np.asarray(wave, np.float64), kind='mfcc', **args)
    got = np.asarray(compute(proc_options, wave), np.float64)
    return float((np.abs(got - want) - rtol * np.abs(want)).max())


def mfcc_dct_k(num_bins):
    """K of the bound: mfcc_dct_kernel's chain `acc += dct x` is num_bins fused multiply-adds (one rounding each;
    the first adds to 0); a coefficient of make_dct_matrix (host_tables.cpp) is float(float(sqrt(2 / N)) cos(.)):
    two float32 roundings; a lifter coefficient of make_lifter is rounded once and its product with the sum once;
    the sqrt(2) of an htk c0 is applied in double and rounded once; 1 for the higher-order terms."""
    return num_bins + 2 + 2 + 1 + 1


def mfcc_dct_want(rows, num_bins, num_ceps, cepstral_lifter, use_energy, htk_compat):
    """(want, bound) float64 [n, num_ceps] from the float32 rows [log energy (use_energy) | num_bins log-mel
    energies]: the DCT, lifter, c0 and htk rules of oracle/spec_f64.py `features`, in float64.
    bound = K 2^-24 sum_m |dct[c, m]| |lifter[c]| |x[m]| (x sqrt 2 for an htk c0 that is not the energy); the
    energy column is copied: bound 0."""
    rows = np.asarray(rows, dtype=np.float64)
    logmel = rows[:, 1:] if use_energy else rows
    assert logmel.shape[1] == num_bins
    m = np.arange(num_bins)
    dct = np.sqrt(2.0 / num_bins) * np.cos(np.pi / num_bins * (m[None, :] + 0.5) * np.arange(num_ceps)[:, None])
    dct[0] = np.sqrt(1.0 / num_bins)
    lifter = np.ones(num_ceps)
    if cepstral_lifter:
        lifter = 1 + 0.5 * cepstral_lifter * np.sin(np.pi * np.arange(num_ceps) / cepstral_lifter)
    want = (logmel @ dct.T) * lifter[None, :]
    bound = mfcc_dct_k(num_bins) * U24 * (np.abs(logmel) @ np.abs(dct).T) * np.abs(lifter)[None, :]
    if use_energy:
        want[:, 0] = rows[:, 0]
        bound[:, 0] = 0.0
    if htk_compat:
        scale = 1.0 if use_energy else np.sqrt(2.0)
        want = np.hstack((want[:, 1:], want[:, :1] * scale))
        bound = np.hstack((bound[:, 1:], bound[:, :1] * scale))
    return want, bound
