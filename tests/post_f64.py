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
            test_crepe_gpu.py (and the family tolerance of conftest.py against the oracle)."""

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
