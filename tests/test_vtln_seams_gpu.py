"""GPU checks of the linear-VTLN kernels (csrc/kernels_vtln.hip) and their host scheduling (csrc/capi_models.hip,
shennong_amd/lvtln.py, VtlnProcessor._estimate_device) at every column group, item, pass and segment seam, against
the float64 statement of tests/lvtln_f64.py: the shapes and the derived scales are those of tests/model_cases.py,
whose CPU half (tests/test_model_cases.py) shows that they reach the seams.  Every test prints its worst measured
ratio to its bound (profiles/gmm_vtln_seams_errors.txt)."""

import functools

import numpy as np
import pytest

import lvtln_f64 as R
import model_cases as M
from shennong_amd import _backend
from shennong_amd import gmm as G
from shennong_amd import lvtln as LV
from test_vtln_gpu import check_stats, device_stats

pytestmark = pytest.mark.gpu

STATS_RTOL = 1e-11    # check_stats: against the same sums over absolute values
GRAM_RTOL = 1e-12
OBJ_RTOL = 1e-10      # class objectives: against the sum of the absolute values of their terms


def stats_ratio(got, x, sel, post, gmm, offsets):
    """Worst error of the statistics over check_stats' own scales, as a fraction of its 1e-11"""
    worst = 0.0
    for s in range(len(offsets) - 1):
        a, b = offsets[s], offsets[s + 1]
        if a == b:
            continue
        beta, K, Gm = R.fmllr_stats(x[a:b], sel[a:b], post[a:b], gmm.means_invvars_, gmm.inv_vars_)
        _, Ks, Gs = R.fmllr_stats(np.abs(x[a:b]), sel[a:b], post[a:b], np.abs(gmm.means_invvars_), gmm.inv_vars_)
        st = LV.FmllrStats.from_device_layout(got[s])
        worst = max(worst, abs(st.beta - beta) / max(1.0, beta), float(np.max(np.abs(st.K - K) / (Ks + 1e-300))),
                    float(np.max(np.abs(st.G - Gm) / (Gs + 1e-300))))
    return worst / STATS_RTOL


def fmllr_at(D, n, C, lens):
    x, gmm, sel, post, offsets = M.fmllr_case(D, n, C, lens)
    got = device_stats(x, sel, post, gmm, offsets)
    assert not np.isnan(got).any()
    check_stats(got, x, sel, post, gmm, offsets)
    again = device_stats(x, sel, post, gmm, offsets)
    assert np.array_equal(M.bits(got), M.bits(again))
    for s in np.nonzero(np.diff(offsets) == 0)[0]:
        assert (M.bits(got[s]) == 0).all()
    return stats_ratio(got, x, sel, post, gmm, offsets)


# ---- F. fMLLR statistics -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', M.VTLN_DIMS + (13,))
def test_fmllr_statistics_at_every_seam(gpu, D, monkeypatch):
    if D * max(M.LONG_LENS) > 100000:
        # the float64 statement as one matrix product (tests/test_model_cases.py: the same sums to 1e-12)
        monkeypatch.setattr(R, 'fmllr_stats', functools.partial(R.fmllr_stats, fast=True))
    worst = {'short': fmllr_at(D, 15, 64, M.SHORT_LENS)}
    if D in M.LONG_DIMS:
        worst['long'] = fmllr_at(D, 15, 64, M.LONG_LENS)
    if D == 13:
        worst['n = 1'] = fmllr_at(D, 1, 64, M.SHORT_LENS)
        worst['n = 64'] = fmllr_at(D, 64, 64, M.SHORT_LENS + (2049,))
    print('D', D, 'worst ratio to the bound (1e-11 of the absolute-value sums):',
          ', '.join('%s %.3g' % kv for kv in worst.items()))


def test_fmllr_statistics_of_no_frames_and_refusals(gpu):
    D, n, C = 13, 15, 64
    x, gmm, sel, post, offsets = M.fmllr_case(D, n, C, (0, 0, 0))
    got = device_stats(x, sel, post, gmm, offsets)
    assert got.shape == (3, LV.stats_rows(D), D + 1) and (M.bits(got) == 0).all()
    x, gmm, sel, post, offsets = M.fmllr_case(D, 65, 80, (5,))
    with pytest.raises(ValueError, match=r'num_gselect must be in \[1, 64\]'):
        device_stats(x, sel, post, gmm, offsets)
    # D = 65 is refused everywhere
    x, gmm, sel, post, offsets = M.fmllr_case(65, 2, 4, (5,))
    refused = r'feature dimension must be in \[1, 64\]'
    with pytest.raises(ValueError, match=refused):
        device_stats(x, sel, post, gmm, offsets)
    dx = _backend.upload_rows([x], np.float32)
    with pytest.raises(ValueError, match=refused):
        LV.vtln_gram(dx, dx, 5, 65)
    lvtln = LV.LinearVtln(65, 2, 0)
    with pytest.raises(ValueError, match=refused):
        LV.DeviceLvtln(lvtln).select(_backend.DeviceBuffer(8 * LV.stats_rows(65) * 66), 1, 'none', 0.0)
    W = _backend.DeviceBuffer(4 * 65 * 66)
    with pytest.raises(ValueError, match=refused):
        LV.affine_apply_segments(G.FrameBlock([x]), offsets, W)
    print('no frames: statistics exactly 0; n = 65 and D = 65 refused')


# ---- E (of the GMM list). an index out of range in the fMLLR selection ---------------------------------------------
@pytest.mark.parametrize('bad_index', ['C', -1])
def test_fmllr_selection_index_out_of_range(gpu, bad_index):
    D, n, C = 13, 5, 32
    x, gmm, sel, post, offsets = M.fmllr_case(D, n, C, (7, 0, 40))
    before = device_stats(x, sel, post, gmm, offsets)
    bad = sel.copy()
    bad[30, 3] = C if bad_index == 'C' else -1
    with pytest.raises(ValueError, match='index out of range'):
        device_stats(x, bad, post, gmm, offsets)
    after = device_stats(x, sel, post, gmm, offsets)
    assert np.array_equal(M.bits(before), M.bits(after))


# ---- G. calls that start inside the block --------------------------------------------------------------------------
def test_fmllr_accumulate_from_inside_the_block(gpu):
    D, n, C = 13, 5, 32
    x, gmm, sel, post, offsets = M.fmllr_case(D, n, C, M.MIXED_LENS)
    block = G.FrameBlock([x])
    dg = G.DeviceGmm(gmm)
    dsel = block.upload_selection(sel)
    dpost = _backend.upload_rows([post], np.float32)
    whole = LV.download_stats(LV.fmllr_accumulate(block, dg, dsel, dpost, n, offsets), 12, D)
    check_stats(whole, x, sel, post, gmm, offsets)
    for first, last in ((0, 12), (0, 5), (5, 12), (3, 4), (11, 12)):
        part = LV.download_stats(LV.fmllr_accumulate(block, dg, dsel, dpost, n, offsets, first, last), last - first, D)
        assert np.array_equal(M.bits(part), M.bits(whole[first:last])), (first, last)
    print('calls from inside the block: bit-equal to the rows of the whole call; worst ratio to the bound %.3g'
          % stats_ratio(whole, x, sel, post, gmm, offsets))


def test_estimate_in_batches_of_five_segments(gpu, monkeypatch):
    from shennong_amd.features import Features, FeaturesCollection
    from shennong_amd.processor.ubm import DiagUbmProcessor
    from shennong_amd.processor.vtln import VtlnProcessor
    D, n, C = 13, 5, 32
    x, gmm, sel, post, offsets = M.fmllr_case(D, n, C, M.MIXED_LENS)
    lvtln = M.tied_lvtln(D, 9, 4, (), 21)
    for c in range(9):
        lvtln.set_warp(c, 0.9 + 0.025 * c)
    utts = ['u%02d' % i for i in range(12)]
    coll = FeaturesCollection({u: Features(x[offsets[i]:offsets[i + 1]], np.arange(M.MIXED_LENS[i]) * 0.01,
                                           validate=False) for i, u in enumerate(utts)})
    arrays = {u: (sel[offsets[i]:offsets[i + 1]], post[offsets[i]:offsets[i + 1]]) for i, u in enumerate(utts)}
    ubm = DiagUbmProcessor(C)
    ubm.gmm = gmm
    vt = VtlnProcessor()
    vt.lvtln = lvtln
    assert LV.segments_per_call(D) > 12
    t1, w1 = vt.estimate(ubm, coll, arrays)
    calls = []
    monkeypatch.setattr(LV, 'segments_per_call', lambda dim: calls.append(dim) or 5)
    t2, w2 = vt.estimate(ubm, coll, arrays)
    assert calls == [D]
    assert list(t1) == list(t2) == utts and w1 == w2
    for u in utts:
        assert np.array_equal(M.bits(t1[u]), M.bits(t2[u])), u
    assert all(w1[utts[i]] == lvtln.get_warp(4) for i in (0, 5, 11))
    print('estimate in batches of 5 segments: transforms and warps identical to the single batch')


# ---- H. the Gram ---------------------------------------------------------------------------------------------------
def gram_case(F, D, weighted):
    rng = np.random.RandomState(1000 * D + F)
    x = (rng.randn(F, D) * 2 + 0.5).astype(np.float32)
    y = (rng.randn(F, D) - 0.25).astype(np.float32)
    w = rng.rand(F).astype(np.float32) if weighted else None
    return x, y, w


@pytest.mark.parametrize('D', M.VTLN_DIMS + (13,))
def test_gram_at_every_seam(gpu, D):
    worst = 0.0
    for F in M.GRAM_FRAMES + (M.GRAM_LONG_FRAMES if D in M.LONG_DIMS else ()):
        for weighted in (False, True):
            x, y, w = gram_case(F, D, weighted)
            dx, dy = _backend.upload_rows([x], np.float32), _backend.upload_rows([y], np.float32)
            dw = _backend.upload_rows([w], np.float32) if weighted else None
            gram = LV.vtln_gram(dx, dy, F, D, dw)
            assert not np.isnan(gram).any(), (F, D, weighted)
            z = np.concatenate([x, np.ones((F, 1)), y], axis=1).astype(np.float64)
            w64 = w.astype(np.float64) if weighted else np.ones(F)
            want = (z * w64[:, None]).T @ z
            scale = (np.abs(z) * w64[:, None]).T @ np.abs(z)
            err = np.abs(gram - want)
            assert (err[scale == 0] == 0).all()
            worst = max(worst, float(np.max(err[scale > 0] / scale[scale > 0])) / GRAM_RTOL)
            assert np.all(err <= GRAM_RTOL * scale), (F, D, weighted)
            assert np.array_equal(M.bits(gram), M.bits(LV.vtln_gram(dx, dy, F, D, dw))), (F, D, weighted)
    print('D', D, 'worst ratio to the bound (1e-12 of the absolute-value Gram): %.3g' % worst)


def test_gram_rows_over_two_blocks(gpu):
    D, F = 64, 2049
    x, y, w = gram_case(F, D, True)
    dx, dy = _backend.upload_rows([x], np.float32), _backend.upload_rows([y], np.float32)
    dw = _backend.upload_rows([w], np.float32)
    cut = 1000
    xb = [_backend.upload_rows([x[:cut]], np.float32), _backend.upload_rows([x[cut:]], np.float32)]
    yb = [_backend.upload_rows([y[:cut]], np.float32), _backend.upload_rows([y[cut:]], np.float32)]
    blk = np.concatenate([np.zeros(cut, np.int32), np.ones(F - cut, np.int32)])
    row = np.concatenate([np.arange(cut), np.arange(F - cut)]).astype(np.int64)
    dblock, drow = LV.upload_row_list(blk, row)
    for weights in (None, dw):
        gram = LV.vtln_gram(dx, dy, F, D, weights)
        rows = LV.vtln_gram_rows(xb, yb, dblock, drow, F, D, weights)
        assert not np.isnan(rows).any()
        assert np.array_equal(M.bits(rows), M.bits(gram))
    print('gram over gathered rows of two blocks: bit-equal to the compact Gram at D = 64, F = 2049')


# ---- I. the class search -------------------------------------------------------------------------------------------
def accumulate_for(lvtln, gmm, x, sel, post, offsets):
    """(statistics on the device, on the host) of a class_setup-style case"""
    block = G.FrameBlock([x])
    dsel = block.upload_selection(sel)
    dpost = _backend.upload_rows([post], np.float32)
    n = sel.shape[1]
    stats = LV.fmllr_accumulate(block, G.DeviceGmm(gmm), dsel, dpost, n, offsets)
    return stats, LV.download_stats(stats, len(offsets) - 1, lvtln.dim())


def check_search(lvtln, stats, host, norm_type, logdet_scale, skip=()):
    """One select against lvtln_f64 per segment; -> (worst objective error over its bound, the outputs)"""
    D, S = lvtln.dim(), host.shape[0]
    dl = LV.DeviceLvtln(lvtln)
    objf, cls, impr, count, dtrans = dl.select(stats, S, norm_type, logdet_scale)
    trans = dtrans.download(np.empty((S, D, D + 1), np.float32))
    worst = 0.0
    what = (D, lvtln.num_classes(), norm_type, logdet_scale)
    for s in range(S):
        if s in skip:
            continue
        st = LV.FmllrStats.from_device_layout(host[s])
        ref = (st.beta, st.K, st.G)
        if st.beta == 0:
            assert cls[s] == lvtln.default_class and impr[s] == 0 and count[s] == 0, what
            assert (objf[s] == 0).all(), what
            np.testing.assert_array_equal(trans[s][:, :D], lvtln.A[lvtln.default_class])
            assert np.all(trans[s][:, D] == 0)
            continue
        objs, scales = M.class_reference(lvtln.A, lvtln.logdets, ref, norm_type, logdet_scale)
        ratio = float(np.max(np.abs(objf[s] - objs) / scales)) / OBJ_RTOL
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, s, ratio)
        assert cls[s] == int(np.argmax(objf[s])), (what, s)     # the FIRST maximum
        assert count[s] == pytest.approx(st.beta, rel=1e-12)
        W = R.compute_transform([lvtln.A[cls[s]]], [lvtln.logdets[cls[s]]], ref, norm_type, logdet_scale, 0,
                                fast=D > 13)[4]
        np.testing.assert_allclose(trans[s], W, atol=1e-6, rtol=1e-6, err_msg=str(what))
        np.testing.assert_allclose(impr[s], objf[s][cls[s]] - R.aux(np.eye(D, D + 1), ref),
                                   rtol=1e-9, atol=1e-9 * abs(objf[s][cls[s]]))
    return worst, (objf, cls, impr, count, trans)


@pytest.mark.parametrize('D,C', M.SELECT_CASES)
def test_class_search_over_several_passes(gpu, D, C):
    S = M.select_segments(D)
    lvtln, gmm, x, sel, post, offsets = M.class_setup(D, C, S, 7 + D + C)
    assert offsets[1] == 0 and len(offsets) == S + 1
    stats, host = accumulate_for(lvtln, gmm, x, sel, post, offsets)
    worst = {}
    for norm_type in ('none', 'offset', 'diag'):
        for logdet_scale in (0.0, 1.0):
            worst[norm_type, logdet_scale], _ = check_search(lvtln, stats, host, norm_type, logdet_scale)
    print('D', D, 'C', C, 'worst ratio of the objectives to the bound (1e-10 of the sum of |terms|): %.3g'
          % max(worst.values()), ' '.join('%s/%g %.3g' % (k[0], k[1], v) for k, v in worst.items()))


def test_class_search_ties_across_passes(gpu):
    D, C, S = 13, 41, 4
    _, gmm, x, sel, post, offsets = M.class_setup(D, C, S, 3)
    # 41 classes that are all one matrix: the first maximum is class 0, not the default class
    lvtln = M.tied_lvtln(D, C, 15, 'all', 5)
    stats, host = accumulate_for(lvtln, gmm, x, sel, post, offsets)
    for norm_type in ('none', 'offset', 'diag'):
        objf, cls, _, _, _ = LV.DeviceLvtln(lvtln).select(stats, S, norm_type, 1.0)
        assert (cls[1:] == 0).all() and cls[0] == 15, (norm_type, cls)
        assert (M.bits(objf[1:]) == M.bits(objf[1:, :1])).all(), norm_type
    # classes 5 and 37 hold one matrix, one in each pass
    lvtln = M.tied_lvtln(D, C, 15, (5, 37), 6)
    base = {}
    for norm_type in ('none', 'offset', 'diag'):
        worst, (objf, cls, _, _, _) = check_search(lvtln, stats, host, norm_type, 0.0)
        assert np.array_equal(M.bits(objf[:, 5]), M.bits(objf[:, 37])), norm_type
        assert (cls != 37).all()
        base[norm_type] = objf
    # an objective depends on the class's matrix alone, not on its slot or its pass
    perm = np.random.RandomState(8).permutation(C)
    assert (perm // 32 != np.arange(C) // 32).any()
    moved = LV.LinearVtln(D, C, 15)
    for c in range(C):
        moved.set_transform(c, lvtln.A[perm[c]])
    for norm_type in ('none', 'offset', 'diag'):
        objf, cls, _, _, _ = LV.DeviceLvtln(moved).select(stats, S, norm_type, 0.0)
        assert np.array_equal(M.bits(objf), M.bits(base[norm_type][:, perm])), norm_type
        assert (cls[1:] == [int(np.argmax(o)) for o in objf[1:]]).all()
    print('ties: 41 equal classes give class 0; classes 5 and 37 bit-equal; objectives follow a permutation of '
          'the classes bit for bit')


def test_class_search_of_the_default_configuration(gpu):
    from shennong_amd.processor.ubm import DiagUbmProcessor
    from shennong_amd.processor.vtln import VtlnProcessor
    vt = VtlnProcessor()
    num_classes = int(1.5 + (vt.max_warp - vt.min_warp) / vt.warp_step)
    default_class = int(0.5 + (1 - vt.min_warp) / vt.warp_step)
    assert (num_classes, default_class) == (M.DEFAULT_CLASSES, M.DEFAULT_CLASS)
    case = M.default_config_case()
    lvtln, x, offsets = case['lvtln'], case['x'], case['offsets']
    for c in range(num_classes):
        lvtln.set_warp(c, vt.min_warp + c * vt.warp_step)
    vt.lvtln = lvtln
    ubm = DiagUbmProcessor(32)
    ubm.gmm = case['gmm']
    block = G.FrameBlock([x])
    dsel = block.upload_selection(case['sel'])
    dpost = _backend.upload_rows([case['post']], np.float32)
    keys = ['a', 'b', 'c']
    transforms, warps, trans = vt._estimate_device(ubm, block, dsel, dpost, 5, offsets, keys)
    worst = 0.0
    for s, (objs, best, W) in enumerate(M.default_config_reference(case)):
        assert M.top_two_margin(objs) > 1e-6
        assert warps[keys[s]] == lvtln.get_warp(best), (s, best)
        np.testing.assert_allclose(trans[s], W, atol=1e-6, rtol=1e-6)
        np.testing.assert_array_equal(transforms[keys[s]], trans[s])
        worst = max(worst, float(np.max(np.abs(trans[s] - W) / (1e-6 + 1e-6 * np.abs(W)))))
    print('default configuration (41 classes, D = 39): classes equal to the reference\'s, worst transform error '
          'over 1e-6 + 1e-6 |W|: %.3g' % worst)


def test_class_search_of_a_one_frame_segment(gpu):
    D, C = 13, 9
    lvtln, gmm, _, _, _, _ = M.class_setup(D, C, 2, 31)
    x, _, sel, post, offsets = M.fmllr_case(D, 5, 32, (120, 1, 200))
    stats, host = accumulate_for(lvtln, gmm, x, sel, post, offsets)
    worst = 0.0
    for norm_type in ('none', 'offset'):
        for logdet_scale in (0.0, 1.0):
            worst = max(worst, check_search(lvtln, stats, host, norm_type, logdet_scale)[0])
    # 'diag': one frame makes the quadratic degenerate (aq = bq = 0 up to rounding), in the reference too
    _, with_it = check_search(lvtln, stats, host, 'diag', 0.0, skip=(1,))
    assert 0 <= with_it[1][1] < C
    keep = np.r_[0:120, 121:321]
    stats2, host2 = accumulate_for(lvtln, gmm, x[keep], sel[keep], post[keep], M.offsets_of((120, 200)))
    assert np.array_equal(M.bits(host2), M.bits(host[[0, 2]]))
    _, without = check_search(lvtln, stats2, host2, 'diag', 0.0)
    for a, b in zip(with_it, without):
        assert np.array_equal(M.bits(a[[0, 2]]), M.bits(b))
    print('one-frame segment: worst ratio of the objectives to the bound under none / offset %.3g; under diag the '
          'call returns, class %d, neighbours bit-equal' % (worst, with_it[1][1]))


# ---- J. affine apply -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 13, 64])
def test_affine_apply_with_empty_segments(gpu, D):
    worst = 0.0
    for offsets in (np.asarray(M.APPLY_OFFSETS, np.int64), np.asarray([0, 300], np.int64)):
        x, W = M.apply_case(D, offsets)
        F = x.shape[0]
        want, tol = M.apply_reference(x, W, offsets)
        block = G.FrameBlock([x])
        dW = _backend.DeviceBuffer(W.nbytes)
        dW.upload(W)
        # an output block out of the poisoned pool, of exactly F D floats
        _backend.DeviceBuffer(4 * F * D).free()
        out = _backend.DeviceBuffer(4 * F * D)
        assert (out.download(np.zeros(F * D, np.uint32)) == M.POISON).all()
        assert LV.affine_apply_segments(block, offsets, dW, out=out) is out
        y = out.download(np.empty((F, D), np.float32))
        assert not (M.bits(y) == M.POISON).any() and np.isfinite(y).all()
        err = np.abs(y - want)
        worst = max(worst, float(np.max(err / tol)))
        assert np.all(err <= tol), (D, len(offsets) - 1)
        assert abs(y[-1, -1] - want[-1, -1]) <= tol[-1, -1]     # the last element of the buffer is the last written
    print('D', D, 'worst ratio to the bound 2^-23 (D + 1) (sum |W x| + |b|): %.3g' % worst)
