"""CPU half of the route tests of the delta, pitch-post and CMVN kernels: the layouts of post_layouts.py reach every
tile seam they claim, and the bounds of post_f64.py are bounds that a correct float32 implementation meets - the C
oracle does, on the very inputs test_post_routes_gpu.py gives the HIP kernels."""

import numpy as np
import pytest

import post_f64
import post_layouts as lay
from oracle import oracle as orc
from oracle import spec_f64
from shennong_amd.processor import KaldiPitchPostProcessor


def test_tile_heights():
    """the heights restated in post_layouts.py are those of shennong_amd/csrc/post_route.h (kFlatTileBytes and
    flat_rows, kDeltaRows, kPostRows; test_post_route.py reads them from the header itself)"""
    assert [lay.flat_rows(d) for d in (13, 23, 40, 43)] == [132, 72, 40, 36]
    assert lay.DELTA_TILED_ROWS == 256 and lay.PITCH_POST_ROWS == 256


@pytest.mark.parametrize('rows', [36, 40, 72, 132, 256])
def test_seam_layout_has_every_seam(rows):
    lengths = lay.seam_layout(rows)
    found = lay.seams(lengths, rows)
    assert all(found.values()), found
    assert len(found) == 17
    off = lay.offsets_of(lengths)
    assert 5 * rows < off[-1] < 6 * rows
    # the properties once more, without the helper: the long utterance and the tile inside it
    long_u = int(np.argmax(lengths))
    a, b = int(off[long_u]), int(off[long_u + 1])
    assert b - a >= 2 * rows + 8 and a % rows != 0 and b % rows == 0
    assert a + 4 <= 2 * rows and 3 * rows <= b - 4
    assert lengths[0] == 0 and lengths[-1] == 0 and (off[-1] % rows) % 2 == 1
    ends = {int(e) for e, n in zip(off[1:], lengths) if n}
    for k in (1, 2, 3, 4):
        assert any(e % rows == rows - k for e in ends) and any(e > rows and e % rows == k for e in ends)


def test_check_seams_names_what_is_missing():
    lengths = lay.seam_layout(36)
    with pytest.raises(ValueError, match='trailing_empty'):
        lay.check_seams(lengths[:-1], 36)
    with pytest.raises(ValueError, match='leading_empty'):
        lay.check_seams(lengths[1:], 36)
    with pytest.raises(ValueError, match='many_boundaries'):
        lay.check_seams([n for i, n in enumerate(lengths) if i != 7], 36)
    with pytest.raises(ValueError, match='interior'):
        lay.check_seams(lengths, 40)    # (a layout is written for ONE tile height)
    with pytest.raises(ValueError):
        lay.seam_layout(32)


def test_seam_layout_small():
    small = lay.seam_layout_small()
    assert [tuple(s) for s in small] == [(1,), (0, 3, 0, 2)]
    assert all(sum(s) < min(lay.flat_rows(d) for d in lay.FLAT_COLS) for s in small)


def test_delta_cases_cover_every_route():
    routes = {case[0] for case in lay.DELTA_CASES}
    assert routes == {'delta_flat_o2w2_kernel', 'delta_tiled_fixed_kernel', 'delta_tiled_kernel', 'delta_kernel'}
    assert {c[3] for c in lay.DELTA_CASES if c[0] == 'delta_flat_o2w2_kernel'} == set(lay.FLAT_COLS)
    for route, order, window, cols, name in lay.DELTA_CASES:
        # launch_deltas' choice as post_layouts.py restates it (a record buffer, aligned pointers)
        assert route == lay.delta_route_of(order, window, cols), (route, order, window, cols)


def test_delta_k():
    """K = taps + roundings of the scales + 1, the roundings counted in post_f64.delta_scale_roundings"""
    assert [post_f64.delta_k(i, 2) for i in range(3)] == [2, 5 + 12 + 1, 9 + 24 + 1]
    assert post_f64.delta_k(5, 5) == 51 + 5 * 24 + 1
    # the float32 scales of the oracle are inside their share of it, relative to the products that make them up
    # (the convolution of the magnitudes: some entries are sums of both signs)
    for order, window in ((2, 2), (3, 3), (5, 5), (1, 1)):
        base = np.abs(spec_f64.delta_scales(1, window)[1])
        size = [np.ones(1)]
        for _ in range(order):
            size.append(np.convolve(size[-1], base))
        for i, (s32, s64) in enumerate(zip(orc.delta_scales(order, window), spec_f64.delta_scales(order, window))):
            err = np.abs(s32.astype(np.float64) - s64)
            assert np.all(err <= post_f64.delta_scale_roundings(i, window) * post_f64.U24 * size[i]), (order, window, i)


@pytest.mark.parametrize('case', lay.DELTA_CASES, ids=lay.delta_id)
def test_delta_bound_is_met_by_the_oracle(case):
    route, order, window, cols, name = case
    mats = post_f64.delta_batch(cols, lay.layout_of(name))
    got = [orc.deltas(m, order, window) for m in mats]
    ratio, u, row, col = post_f64.delta_ratio(got, mats, order, window)
    print(f'delta oracle {lay.delta_id(case)}: worst error / bound {ratio:.3f} (utterance {u}, row {row}, column {col})')
    assert ratio <= 1.0
    for g, m in zip(got, mats):
        assert np.array_equal(g[:, :cols], m)


def test_delta_bound_catches_a_neighbour_from_the_wrong_row():
    """a clamp that is off by one row misses the bound by orders of magnitude"""
    cols, layout = 13, lay.seam_layout(132)
    mats = post_f64.delta_batch(cols, layout)
    u = int(np.argmax(layout))
    wrong = orc.deltas(np.concatenate([mats[u], mats[u + 1][:1]]), 2, 2)[:-1]   # the end clamps one row late
    ratio, _, row, _ = post_f64.delta_ratio([wrong], [mats[u]], 2, 2)
    assert ratio > 1000.0 and row >= mats[u].shape[0] - 4


def _pitch_proc(left, right, window, flags=(1, 1, 1, 1)):
    return KaldiPitchPostProcessor(
        delta_pitch_noise_stddev=0, normalization_left_context=left, normalization_right_context=right,
        delta_window=window, add_pov_feature=flags[0], add_normalized_log_pitch=flags[1],
        add_delta_pitch=flags[2], add_raw_log_pitch=flags[3])


@pytest.mark.parametrize('context', lay.PITCH_CONTEXTS, ids=lambda c: f'{c[0]}-{c[1]}-{c[2]}-{c[3]}')
def test_pitch_post_bound_is_met_by_the_oracle(context):
    """the oracle is within the family tolerance of the float64 statement (so 4 times its error is a bound the
    tolerance does not cut short), and the sum of POV weights that the normalised column divides by stays away from
    zero: every weight is at least nccf_to_pov(0) = 7.4e-4 and they only add"""
    route, left, right, window = context
    raws = post_f64.pitch_batch(lay.seam_layout(lay.PITCH_POST_ROWS))
    proc = _pitch_proc(left, right, window)
    for raw in raws:
        if not raw.shape[0]:
            continue
        want = post_f64.pitch_statement(proc, raw)
        got = orc.process_pitch(proc._options, raw)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=7e-6)
        pov = spec_f64.nccf_to_pov(raw[:, 0].astype(np.float64))
        n = raw.shape[0]
        sums = [pov[max(0, t - left):min(n, t + right + 1)].sum() for t in range(n)]
        assert min(sums) >= 7.4e-4 and pov.min() >= 7.4e-4
    for flags in lay.PITCH_FLAGS:
        assert _pitch_proc(left, right, window, flags).ndims == sum(flags)


@pytest.mark.parametrize('setting', lay.CMVN_WEIGHTS)
@pytest.mark.parametrize('cols, route', lay.CMVN_COLS)
def test_cmvn_bounds_are_met_by_the_oracle(cols, route, setting):
    lengths = lay.cmvn_lengths(cols)
    mats, weights = post_f64.cmvn_batch(cols, lengths, setting)
    worst = 0.0
    for u, m in enumerate(mats):
        w = None if weights is None else weights[u]
        want, bound = post_f64.cmvn_want(m, w)
        got = orc.cmvn_accumulate(m, weights=w)
        assert got[0, cols] == want[0, cols]     # the count is exact
        err = np.abs(got - want)
        assert np.all(err <= bound), (u, float((err - bound).max()))
        worst = max(worst, float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))))
        # the float64 statement on the same float32 products is inside the bound too
        s, q, _ = post_f64.cmvn_terms(m, w)
        assert np.all(np.abs(spec_f64.cmvn_stats(s)[0, :cols] - want[0, :cols]) <= bound[0, :cols])
        assert np.all(np.abs(spec_f64.cmvn_stats(q)[0, :cols] - want[1, :cols]) <= bound[1, :cols])
    print(f'cmvn oracle d{cols} {setting}: worst error / bound {worst:.3g}')
    if setting == 'one_utterance_all_zero':
        assert not np.any(orc.cmvn_accumulate(mats[4], weights=weights[4]))


@pytest.mark.parametrize('norm_vars', [True, False])
@pytest.mark.parametrize('reverse', [True, False])
def test_cmvn_apply_tolerance_is_met_by_the_oracle(norm_vars, reverse):
    for cols, lengths in [(1, [255, 256, 257])] + [(d, lay.cmvn_lengths(d)) for d, _ in lay.CMVN_COLS]:
        mats, _ = post_f64.cmvn_batch(cols, lengths, 'none')
        for group in (0, 1):
            mine = [m for u, m in enumerate(mats) if u % 2 == group]
            stats = np.zeros((2, cols + 1))
            for m in mine:
                orc.cmvn_accumulate(m, stats=stats)
            for m in mine:
                want, tol = post_f64.cmvn_apply_want(m, stats, norm_vars, reverse)
                got = orc.cmvn_apply(m, stats, norm_vars=norm_vars, reverse=reverse)
                assert np.all(np.abs(got.astype(np.float64) - want) <= tol)
