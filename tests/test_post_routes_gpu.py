"""Every launch route of launch_deltas, launch_pitch_post and launch_cmvn_stats (kernels_delta.hip,
kernels_pitch_post.hip, kernels_cmvn.hip; the ladders: post_route.h, on the CPU in test_post_route.py), on batches whose
utterance boundaries sit on every kind of tile seam (post_layouts.py), against the float64 statements with the
derived bounds of post_f64.py.  test_post_routes.py shows on the CPU that the float32 C oracle meets the same bounds
on the same inputs.  Every test asserts the route through Plan.kernel_name and prints its worst error over bound
(run with -s; the committed lines are profiles/post_routes_errors.txt).

Delta: |got - want| <= K 2^-24 sum |scale| |input| with K = taps + roundings of the scales + 1, where
make_delta_scales (host_tables.cpp) spends at most 4 window + 4 float32 roundings per order on a scale: 2 window + 1
products and as many additions of its convolution, the rounding of 1 / normaliser and the multiplication by it
(post_f64.delta_scale_roundings).  Order 2, window 2: K = 2, 18 and 34 for the three blocks."""

import ctypes as C
import functools

import numpy as np
import pytest

import post_f64
import post_layouts as lay
from conftest import assert_close
from oracle import oracle as orc
from shennong_amd import Features, _abi, _backend
from shennong_amd.postprocessor import CmvnPostProcessor, DeltaPostProcessor
from shennong_amd.processor import KaldiPitchPostProcessor

pytestmark = pytest.mark.gpu


def _features(mats):
    return [Features(m, np.arange(m.shape[0], dtype=np.float64) * 0.01, validate=False) for m in mats]


def _pitch_features(raws):
    return [Features(r, np.arange(r.shape[0], dtype=np.float64) * 0.01,
                     properties={'pitch': {}, 'pipeline': [{'name': 'pitch', 'columns': [0, 1]}]}, validate=False)
            for r in raws]


def _split(flat, lengths):
    off = lay.offsets_of(lengths)
    return [flat[a:b] for a, b in zip(off[:-1], off[1:])]


# ---- delta ------------------------------------------------------------------------------------------------------
def _check_delta(tag, got, mats, order, window):
    cols = mats[0].shape[1]
    ratio, u, row, col = post_f64.delta_ratio(got, mats, order, window)
    print(f'delta {tag}: worst error / bound {ratio:.3f} (utterance {u}, row {row}, column {col})')
    assert ratio <= 1.0, (tag, ratio, u, row, col)
    for g, m in zip(got, mats):
        assert np.array_equal(g[:, :cols], m), tag     # block 0 is the input, bit for bit


@pytest.mark.parametrize('case', lay.DELTA_CASES, ids=lay.delta_id)
def test_delta_routes(gpu, case):
    route, order, window, cols, name = case
    mats = post_f64.delta_batch(cols, lay.layout_of(name))
    proc = DeltaPostProcessor(order=order, window=window)
    outs = proc._process_batch(_features(mats))
    assert _backend.get_plan(proc._build_options()).kernel_name(1) == route
    assert [o.shape for o in outs] == [(m.shape[0], cols * (order + 1)) for m in mats]
    _check_delta(lay.delta_id(case), [o.data for o in outs], mats, order, window)


def test_delta_tile_records_follow_the_table(gpu):
    """the flat kernel's tile records are cached on the plan: kept while the offsets table and the column count stay,
    rebuilt when either changes - every call gives the bits of a plan that never saw another table"""
    lengths_a = lay.seam_layout(lay.flat_rows(13))
    lengths_b = lengths_a[::-1]                      # the same frames, other boundaries
    x13 = np.concatenate(post_f64.delta_batch(13, lengths_a))
    x23 = np.concatenate(post_f64.delta_batch(23, lengths_a))
    opts = DeltaPostProcessor()._build_options()
    plan = _backend.get_plan(opts)
    for step, (flat, lengths) in enumerate([(x13, lengths_a), (x13, lengths_b), (x13, lengths_a), (x23, lengths_a),
                                            (x13, lengths_a)]):
        mats = _split(flat, lengths)
        got = plan.run_post(mats)
        assert plan.kernel_name(1) == 'delta_flat_o2w2_kernel'
        fresh = _backend.Plan(opts)
        want = fresh.run_post(mats)
        assert fresh.kernel_name(1) == 'delta_flat_o2w2_kernel'
        for u, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (step, u)
        _check_delta(f'tile records step {step}', got, mats, 2, 2)


def _run_device(plan, flat, foff, cols, in_skew, out_skew):
    """snf_post_run_batch_device on buffers that start `in_skew` / `out_skew` bytes behind a 16-byte boundary"""
    L = _backend.lib()
    ocols = plan.post_ndims(cols)
    d_in = _backend.DeviceBuffer(flat.nbytes + 16)
    d_out = _backend.DeviceBuffer(flat.shape[0] * ocols * 4 + 16)
    try:
        assert d_in.ptr % 16 == 0 and d_out.ptr % 16 == 0
        _backend.check(L.snf_memcpy_h2d(C.c_void_p(d_in.ptr + in_skew), flat.ctypes.data_as(C.c_void_p), flat.nbytes))
        plan.run_post_device(d_in.ptr + in_skew, cols, foff, d_out.ptr + out_skew)   # (the plan's stream: waited for)
        out = np.empty((flat.shape[0], ocols), np.float32)
        _backend.check(L.snf_memcpy_d2h(out.ctypes.data_as(C.c_void_p), C.c_void_p(d_out.ptr + out_skew), out.nbytes))
        return out, plan.kernel_name(1)
    finally:
        d_in.free()
        d_out.free()


@pytest.fixture(scope='module')
def cross_route_input():
    lengths = lay.seam_layout(lay.flat_rows(13))
    return lengths, post_f64.delta_batch(13, lengths)


@pytest.mark.parametrize('which', ['input', 'output'])
def test_delta_pointers_off_the_16_byte_grid(gpu, cross_route_input, which):
    """the flat kernel loads and stores 16 bytes at a time: a pointer off that grid takes delta_tiled_fixed_kernel,
    and the tile records built on the first call serve the third"""
    lengths, mats = cross_route_input
    flat, foff = np.ascontiguousarray(np.concatenate(mats)), lay.offsets_of(lengths)
    plan = _backend.Plan(DeltaPostProcessor()._build_options())
    outs = []
    for skew, route in ((0, 'delta_flat_o2w2_kernel'), (4, 'delta_tiled_fixed_kernel'), (0, 'delta_flat_o2w2_kernel')):
        out, name = _run_device(plan, flat, foff, 13, skew if which == 'input' else 0, skew if which == 'output' else 0)
        assert name == route
        _check_delta(f'{which} pointer + {skew} bytes, {route}', _split(out, lengths), mats, 2, 2)
        outs.append(out)
    assert np.array_equal(outs[0], outs[2])
    # "the same products in the same order" (kernels_delta.hip): the two routes agree bit for bit
    assert np.array_equal(outs[0], outs[1])


def test_delta_routes_agree_bit_for_bit(gpu, cross_route_input):
    """order 2, window 2 on the same 13 columns: delta_flat_o2w2_kernel, delta_tiled_fixed_kernel<2,2> (the first 7
    of them as a batch of their own) and delta_kernel (the 13 inside rows of 257 columns) promise the same products
    in the same order; a column's arithmetic does not depend on its neighbours"""
    lengths, mats = cross_route_input
    proc = DeltaPostProcessor()
    plan = _backend.get_plan(proc._build_options())
    flat = [o.data for o in proc._process_batch(_features(mats))]
    assert plan.kernel_name(1) == 'delta_flat_o2w2_kernel'
    narrow = [o.data for o in proc._process_batch(_features([np.ascontiguousarray(m[:, :7]) for m in mats]))]
    assert plan.kernel_name(1) == 'delta_tiled_fixed_kernel'
    rng = np.random.default_rng(5)
    wide_in = [np.concatenate([m, rng.standard_normal((m.shape[0], 244)).astype(np.float32)], axis=1) for m in mats]
    wide = [o.data for o in proc._process_batch(_features(wide_in))]
    assert plan.kernel_name(1) == 'delta_kernel'
    for u, (f, n, w) in enumerate(zip(flat, narrow, wide)):
        for block in range(3):
            want = f[:, 13 * block:13 * block + 13]
            assert np.array_equal(n[:, 7 * block:7 * block + 7], want[:, :7]), ('delta_tiled_fixed_kernel', u, block)
            assert np.array_equal(w[:, 257 * block:257 * block + 13], want), ('delta_kernel', u, block)


# ---- pitch post -------------------------------------------------------------------------------------------------
def _pitch_proc(left, right, window, flags):
    return KaldiPitchPostProcessor(
        delta_pitch_noise_stddev=0, normalization_left_context=left, normalization_right_context=right,
        delta_window=window, add_pov_feature=flags[0], add_normalized_log_pitch=flags[1],
        add_delta_pitch=flags[2], add_raw_log_pitch=flags[3])


@functools.lru_cache(maxsize=None)
def _pitch_reference(left, right, window):
    """(raw rows, float64 statement, float32 oracle) per utterance, all four columns: computed once per window and
    shared by the flag sets (read only)"""
    raws = post_f64.pitch_batch(lay.seam_layout(lay.PITCH_POST_ROWS))
    proc = _pitch_proc(left, right, window, (1, 1, 1, 1))
    return (raws, [post_f64.pitch_statement(proc, r) for r in raws],
            [orc.process_pitch(proc._options, r) for r in raws])


@pytest.mark.parametrize('flags', lay.PITCH_FLAGS, ids=lambda f: ''.join(map(str, f)))
@pytest.mark.parametrize('context', lay.PITCH_CONTEXTS, ids=lambda c: f'{c[0]}-{c[1]}-{c[2]}-{c[3]}')
def test_pitch_post_routes(gpu, context, flags):
    """per output column the device may err 4 times as far from the float64 statement as the float32 C oracle does
    on the same input (the rule of test_bottleneck_gpu.py / test_crepe_gpu.py: logf, exp and pow have no derived
    bound), and stays inside the family tolerance of the oracle.  The oracle's logf is correctly rounded at these
    pitches, so the raw log-pitch column allows 2 ulp: a log pitch that is off by more than a last-place rounding
    or two does not pass."""
    route, left, right, window = context
    raws, statement, oracle = _pitch_reference(left, right, window)
    keep = [k for k in range(4) if flags[k]]
    proc = _pitch_proc(left, right, window, flags)
    outs = [o.data for o in proc._process_batch(_pitch_features(raws))]
    assert _backend.get_plan(proc._build_options()).kernel_name(1) == route
    assert [o.shape for o in outs] == [(r.shape[0], len(keep)) for r in raws]
    want = [s[:, keep] for s in statement]
    bound = 4.0 * post_f64.column_errors([o[:, keep] for o in oracle], want)
    err = post_f64.column_errors(outs, want)
    print(f'pitch_post {route} ({left}, {right}, {window}) flags {flags}: worst error / bound per column',
          ' '.join(f'{e / b:.3f}' for e, b in zip(err, bound)), '(bounds', ' '.join(f'{b:.3g}' for b in bound) + ')')
    assert np.all(err <= bound), (err, bound)
    for o, w in zip(outs, oracle):
        assert_close(o, np.ascontiguousarray(w[:, keep]), rtol=1e-4, family='pitch_post')


def test_pitch_post_kernels_agree_bit_for_bit(gpu, monkeypatch):
    """pitch_post_tiled_kernel is "the same arithmetic" as pitch_post_kernel with the POV weight and the log pitch of
    a frame evaluated once: the same options (75, 75, 2) on the same input give the same bits"""
    raws, _, _ = _pitch_reference(75, 75, 2)
    proc = _pitch_proc(75, 75, 2, (1, 1, 1, 1))
    plan = _backend.get_plan(proc._build_options())
    tiled = [o.data for o in proc._process_batch(_pitch_features(raws))]
    assert plan.kernel_name(1) == 'pitch_post_tiled_kernel'
    monkeypatch.setenv('SNF_PITCH_POST_PER_FRAME', '1')
    per_frame = [o.data for o in proc._process_batch(_pitch_features(raws))]
    assert plan.kernel_name(1) == 'pitch_post_kernel'
    for u, (a, b) in enumerate(zip(tiled, per_frame)):
        assert np.array_equal(a, b), u


# ---- CMVN -------------------------------------------------------------------------------------------------------
def _cmvn_plan():
    return _backend.get_plan(_abi.default_options(_abi.KIND_CMVN))


def _ratio(err, bound):
    return float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)))


@pytest.mark.parametrize('setting', lay.CMVN_WEIGHTS)
@pytest.mark.parametrize('cols, route', lay.CMVN_COLS)
def test_cmvn_stats_routes(gpu, cols, route, setting):
    """per utterance through CmvnPostProcessor.accumulate, and per group (two groups, interleaved) through
    snf_cmvn_accumulate: |got - want| <= n 2^-53 sum |terms| against the exactly rounded sum of the n float32
    products, the count exact"""
    lengths = lay.cmvn_lengths(cols)
    mats, weights = post_f64.cmvn_batch(cols, lengths, setting)
    plan = _cmvn_plan()
    worst = 0.0
    for u, m in enumerate(mats):
        w = None if weights is None else weights[u]
        proc = CmvnPostProcessor(cols)
        proc.accumulate(_features([m])[0], weights=w)
        if m.shape[0]:
            assert plan.kernel_name(1) == route
        want, bound = post_f64.cmvn_want(m, w)
        assert proc.count == want[0, cols]
        err = np.abs(proc.stats - want)
        assert np.all(err <= bound), (u, float((err - bound).max()))
        worst = max(worst, _ratio(err, bound))
    groups = np.arange(len(mats), dtype=np.int32) % 2
    stats = np.zeros((2, 2, cols + 1))
    plan.cmvn_accumulate(mats, stats, weights=weights, groups=groups)
    assert plan.kernel_name(1) == route
    for g in (0, 1):
        mine = [u for u in range(len(mats)) if groups[u] == g]
        want, bound = post_f64.cmvn_want(np.concatenate([mats[u] for u in mine]),
                                         None if weights is None else np.concatenate([weights[u] for u in mine]))
        assert stats[g, 0, cols] == want[0, cols]
        err = np.abs(stats[g] - want)
        assert np.all(err <= bound), (g, float((err - bound).max()))
        worst = max(worst, _ratio(err, bound))
    print(f'cmvn {route} d{cols} weights {setting}: worst error / bound {worst:.3g}')


@pytest.mark.parametrize('norm_vars', [True, False])
@pytest.mark.parametrize('reverse', [True, False])
@pytest.mark.parametrize('cols, lengths', [(1, [255, 256, 257])] + [(d, lay.cmvn_lengths(d)) for d, _ in lay.CMVN_COLS],
                         ids=lambda v: str(v) if isinstance(v, int) else '-'.join(map(str, v)))
def test_cmvn_apply(gpu, cols, lengths, norm_vars, reverse):
    """cmvn_apply_kernel with the device's own statistics of two interleaved groups: the float64 statement's scale
    and offset through the two float32 roundings the kernel states, 2 ulp of the result + 1 ulp of the offset"""
    mats, _ = post_f64.cmvn_batch(cols, lengths, 'none')
    plan = _cmvn_plan()
    groups = np.arange(len(mats), dtype=np.int32) % 2
    stats = np.zeros((2, 2, cols + 1))
    plan.cmvn_accumulate(mats, stats, groups=groups)
    outs = plan.cmvn_apply(mats, stats, groups=groups, norm_vars=norm_vars, reverse=reverse)
    assert plan.kernel_name(1) == 'cmvn_apply_kernel'
    worst = 0.0
    for u, (m, o) in enumerate(zip(mats, outs)):
        want, tol = post_f64.cmvn_apply_want(m, stats[groups[u]], norm_vars, reverse)
        assert o.shape == want.shape
        err = np.abs(o.astype(np.float64) - want)
        assert np.all(err <= tol), (u, float((err - tol).max()))
        if m.shape[0]:
            worst = max(worst, _ratio(err, tol))
            # the processor with the group's statistics gives the same rows
            single = CmvnPostProcessor(cols, stats=stats[groups[u]]).process(
                _features([m])[0], norm_vars=norm_vars, reverse=reverse)
            assert np.array_equal(single.data, o)
    print(f'cmvn_apply d{cols} norm_vars {norm_vars} reverse {reverse}: worst error / tolerance {worst:.3g}')
