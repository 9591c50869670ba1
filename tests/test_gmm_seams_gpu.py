"""GPU checks of the diagonal-GMM kernels (csrc/kernels_gmm.hip) and their host scheduling (csrc/capi_models.hip)
at every tile, block, chunk and scratch seam, against the float64 statement of tests/gmm_f64.py: the shapes and the
derived scales are those of tests/model_cases.py, whose CPU half (tests/test_model_cases.py) shows that they reach
the seams.  Every test prints its worst measured ratio to its bound (profiles/gmm_vtln_seams_errors.txt)."""

import numpy as np
import pytest

import gmm_f64 as R
import model_cases as M
from shennong_amd import gmm as G

pytestmark = pytest.mark.gpu

POST_ATOL = 2e-6     # the project's figure for selection posteriors (test_ubm_gpu.py)
LSE_TOL = 1e-6       # ... for every log-sum-exp, relative and absolute
LOGLIKE_RATIO = 1e-5


def warm(gpu, *sizes):
    """Parks one block per size in the device pool, so that the buffers the next call allocates come out of the
    pool, full of the poison pattern (the `gpu` fixture)"""
    held = [gpu.DeviceBuffer(max(16, int(n))) for n in sizes]
    for buf in held:
        buf.free()


def written(*arrays):
    """No 32-bit word of an output still holds the poison pattern"""
    return all(not (M.bits(a).view(np.uint32) == M.POISON).any() for a in arrays)


def lse_ratio(got, want):
    return float(np.max(np.abs(got - want) / (LSE_TOL + LSE_TOL * np.abs(want))))


# ---- A. L, gselect, the gathered path, selection posteriors --------------------------------------------------------
@pytest.mark.parametrize('D', M.GMM_DIMS)
def test_loglikes_selection_and_posteriors_at_every_seam(gpu, D):
    worst = {'L': 0.0, 'post': 0.0, 'lse': 0.0}
    soft_entropy = []
    for F, C, soft in M.seam_shapes(M.SEAM_FRAMES):
        what = (F, C, D, soft)
        x, gmm = M.seam_mixture(F, C, D, soft)
        block = G.FrameBlock([x])
        dg = G.DeviceGmm(gmm)
        n = min(C, 15)
        warm(gpu, 4 * F * C, 4 * F * n, 4 * F, 4 * F * C, 4 * F, 8 * C * (2 * D + 1) + 8)
        L = block.loglikes(dg)
        assert written(L) and np.isfinite(L).all(), what
        m64 = M.model64(gmm)
        ratio = float(np.max(np.abs(L - R.loglikes(x, *m64)) / R.loglike_bound(x, *m64)))
        worst['L'] = max(worst['L'], ratio / LOGLIKE_RATIO)
        assert ratio <= LOGLIKE_RATIO, (what, ratio)
        # the selection is exactly the order of the downloaded L under the tie rule
        idx, gl = block.gselect(dg, n)
        assert written(gl), what
        np.testing.assert_array_equal(idx, R.gselect(L, n), err_msg=str(what))
        # the gathered kernel sees the same bits of L
        pre = np.tile(np.arange(C)[::-1], (F, 1)).astype(np.int32)
        idx2, gl2 = block.gselect(dg, n, preselect=pre)
        np.testing.assert_array_equal(idx2, idx, err_msg=str(what))
        assert np.array_equal(M.bits(gl2), M.bits(gl)), what
        Lsel = np.take_along_axis(L, idx.astype(np.int64), axis=1)
        for min_post in (None, 0.01):
            post, like = block.selection_posteriors(dg, idx, min_post)
            assert written(post, like), what
            want, wlike = R.selection_posteriors(Lsel, min_post)
            err = float(np.abs(post - want).max())
            worst['post'] = max(worst['post'], err / POST_ATOL)
            assert err <= POST_ATOL, (what, min_post, err)
            worst['lse'] = max(worst['lse'], lse_ratio(like, wlike))
            np.testing.assert_allclose(like, wlike, rtol=LSE_TOL, atol=LSE_TOL, err_msg=str(what))
        np.testing.assert_allclose(gl, R.logsumexp(Lsel, axis=1), rtol=LSE_TOL, atol=LSE_TOL, err_msg=str(what))
        # every log-sum-exp over all of C against that of the downloaded L
        lse = R.logsumexp(L, axis=1)
        if soft:
            soft_entropy.append(float(np.median(lse - L.max(axis=1))))
        idx_all, gl_all = block.gselect(dg, C)
        np.testing.assert_array_equal(idx_all, R.gselect(L, C), err_msg=str(what))
        _, _, acc_lse = block.accumulate(dg, with_lse=True)
        _, like_all = block.selection_posteriors(dg, idx_all)
        for name, got in (('gselect', gl_all), ('accumulate', acc_lse), ('selection', like_all)):
            assert written(got), (what, name)
            worst['lse'] = max(worst['lse'], lse_ratio(got, lse))
            np.testing.assert_allclose(got, lse, rtol=LSE_TOL, atol=LSE_TOL, err_msg=str((what, name)))
    print('D', D, 'worst ratio to the bound: loglikes %.3g (of 1e-5 of the dot-product scale), posteriors %.3g '
          '(of 2e-6), log-sum-exps %.3g (of 1e-6 + 1e-6 |lse|); median lse - max L of the soft mixtures %.3g'
          % (worst['L'], worst['post'], worst['lse'], min(soft_entropy)))
    assert min(soft_entropy) > 0.01     # the soft mixtures are soft: the log-sum-exps are not the maximum


# ---- B. the E-step, element by element -----------------------------------------------------------------------------
def check_estep(block, dg, x, w, what):
    """(ratio to the derived bound, the same without its floor wherever T > 0, ratio to the row-max bound, ratio of
    tot_like to its bound) of one accumulate against gmm_f64.accumulate fed with the device's L"""
    L = block.loglikes(dg)
    stats, tot, _ = block.accumulate(dg)
    assert not np.isnan(stats).any(), what
    occ, m1, m2, tl = R.accumulate(x, L, w)
    want = np.concatenate([occ[:, None], m1, m2], axis=1)
    err = np.abs(stats - want)
    T, floor = M.estep_scale(x, L, w)
    bound = T + floor
    assert (err[bound == 0] == 0).all(), what
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    live = T > 0
    plain = float(np.max(err[live] / T[live])) if live.any() else 0.0
    assert ratio <= 1.0, (what, ratio, plain)
    # the existing check, against the largest entry of the row
    scale = np.max(np.abs(want), axis=1, keepdims=True) + 1e-30
    rowmax = float(np.max(err / scale))
    assert rowmax <= 1e-5, (what, rowmax)
    tot_bound = 1e-5 * np.sum(np.abs(R.logsumexp(L, axis=1)) * (1 if w is None else w))
    assert abs(tot - tl) <= tot_bound, (what, tot, tl)
    # deterministic
    stats2, tot2, _ = block.accumulate(dg)
    assert np.array_equal(M.bits(stats), M.bits(stats2)) and tot == tot2, what
    return ratio, plain, rowmax / 1e-5, abs(tot - tl) / tot_bound if tot_bound else 0.0


@pytest.mark.parametrize('D', M.GMM_DIMS)
def test_estep_statistics_element_by_element(gpu, D):
    worst = np.zeros(4)
    for F, C, soft in M.seam_shapes(M.ESTEP_FRAMES):
        x, gmm = M.seam_mixture(F, C, D, soft)
        dg = G.DeviceGmm(gmm)
        for w in (None, M.estep_weights(F)):
            block = G.FrameBlock([x], None if w is None else [w])
            warm(gpu, 8 * C * (2 * D + 1) + 8, 4 * F * C)
            worst = np.maximum(worst, check_estep(block, dg, x, w, (F, C, D, soft, w is not None)))
    print('D', D, 'worst ratio to the bound: statistics %.3g (derived, element by element; %.3g without the floor '
          'wherever T > 0), %.3g (1e-5 of the row maximum), tot_like %.3g' % tuple(worst))


def test_estep_in_22_chunks(gpu):
    F, C, D = M.CHUNKED
    x, gmm = M.mixture(F + C + D, F, D, C)
    block = G.FrameBlock([x])
    worst = check_estep(block, G.DeviceGmm(gmm), x, None, M.CHUNKED)
    print('chunked', M.CHUNKED, 'worst ratio to the bound: statistics %.3g (derived; %.3g without the floor '
          'wherever T > 0), %.3g (row maximum), tot_like %.3g' % worst)


def test_estep_of_no_frames(gpu):
    x, gmm = M.seam_mixture(65, 17, 33)
    dg = G.DeviceGmm(gmm)
    real = G.FrameBlock([x])
    empty = G.FrameBlock([x[:0]])
    before, tot_before, lse_before = real.accumulate(dg, with_lse=True)
    warm(gpu, 8 * 17 * 67 + 8)
    stats, tot, _ = empty.accumulate(dg)
    assert stats.shape == (17, 67) and (M.bits(stats) == 0).all() and tot == 0.0
    after, tot_after, lse_after = real.accumulate(dg, with_lse=True)
    assert np.array_equal(M.bits(before), M.bits(after)) and tot_before == tot_after
    assert np.array_equal(M.bits(lse_before), M.bits(lse_after))
    print('no frames: statistics and tot_like exactly 0, the next call bit-equal to the one before')


# ---- C. the gselect scratch seam -----------------------------------------------------------------------------------
def test_gselect_across_the_scratch_seam(gpu):
    F, C, D = M.SCRATCH
    n = 5
    x, gmm = M.mixture(F + C + D, F, D, C)
    dg = G.DeviceGmm(gmm)
    warm(gpu, 4 * F * n, 4 * F)
    idx, lse = G.FrameBlock([x]).gselect(dg, n)
    assert written(lse) and np.isfinite(lse).all()
    assert idx.min() >= 0 and idx.max() < C
    tail = M.SCRATCH_TAIL
    small = G.FrameBlock([x[tail:]])
    idx_s, lse_s = small.gselect(dg, n)
    wrong = int((idx[tail:] != idx_s).any(axis=1).sum()) + int((M.bits(lse[tail:]) != M.bits(lse_s)).sum())
    print('scratch seam: %d of %d frames differ from the block that does not cross it' % (wrong, F - tail))
    np.testing.assert_array_equal(idx[tail:], idx_s)
    assert np.array_equal(M.bits(lse[tail:]), M.bits(lse_s))
    np.testing.assert_array_equal(idx_s, R.gselect(small.loglikes(dg), n))
    # the first block too: its head against a block of its own
    head = G.FrameBlock([x[:67]])
    idx_h, lse_h = head.gselect(dg, n)
    np.testing.assert_array_equal(idx[:67], idx_h)
    assert np.array_equal(M.bits(lse[:67]), M.bits(lse_h))


# ---- D. Gaussians of weight zero -----------------------------------------------------------------------------------
def test_zero_weight_gaussians(gpu):
    x, gmm = M.zero_weight_case()
    F, C = x.shape[0], gmm.num_gauss()
    zero = list(M.ZERO_WEIGHT)
    others = [c for c in range(C) if c not in zero]
    block = G.FrameBlock([x])
    dg = G.DeviceGmm(gmm)
    L = block.loglikes(dg)
    assert np.isneginf(L[:, zero]).all() and np.isfinite(L[:, others]).all()
    lse = R.logsumexp(L[:, others], axis=1)
    worst = 0.0
    # dense posteriors
    post, plse = block.posteriors(dg, with_lse=True)
    assert not np.isnan(post).any() and (post[:, zero] == 0).all()
    assert np.abs(post[:, others] - M.posteriors64(L[:, others])[0]).max() <= POST_ATOL
    # gselect: the two last, the higher index first among equals
    idx, glse = block.gselect(dg, C)
    np.testing.assert_array_equal(idx, R.gselect(L, C))
    assert (idx[:, -2:] == [11, 4]).all()
    pre = np.tile(np.arange(C)[::-1], (F, 1)).astype(np.int32)
    idx2, glse2 = block.gselect(dg, C, preselect=pre)
    np.testing.assert_array_equal(idx2, idx)
    # selection posteriors over all 17, with and without pruning
    likes = []
    for min_post in (None, 0.01):
        spost, like = block.selection_posteriors(dg, idx, min_post)
        assert not np.isnan(spost).any() and (spost[:, -2:] == 0).all()
        want, _ = R.selection_posteriors(np.take_along_axis(L, idx.astype(np.int64), axis=1)[:, :-2], min_post)
        assert np.abs(spost[:, :-2] - want).max() <= POST_ATOL
        likes.append(like)
    # the E-step: their rows are exactly 0, the others as without them
    stats, tot, alse = block.accumulate(dg, with_lse=True)
    assert not np.isnan(stats).any() and (M.bits(stats[zero]) == 0).all() and np.isfinite(tot)
    occ, m1, m2, tl = R.accumulate(x, L[:, others])
    want = np.concatenate([occ[:, None], m1, m2], axis=1)
    T, floor = M.estep_scale(x, L[:, others])
    ratio = float(np.max(np.abs(stats[others] - want) / (T + floor)))
    assert ratio <= 1.0, ratio
    for name, got in (('posteriors', plse), ('gselect', glse), ('preselect', glse2), ('selection', likes[0]),
                      ('selection, pruned', likes[1]), ('accumulate', alse)):
        assert not np.isnan(got).any(), name
        worst = max(worst, lse_ratio(got, lse))
        np.testing.assert_allclose(got, lse, rtol=LSE_TOL, atol=LSE_TOL, err_msg=name)
    print('zero weights: worst ratio to the bound: log-sum-exps %.3g (of 1e-6 + 1e-6 |lse|), statistics of the '
          'other rows %.3g (derived)' % (worst, ratio))


# ---- E. indices out of range ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad_index', ['C', -1])
def test_an_index_out_of_range_is_refused_and_leaves_no_trace(gpu, bad_index):
    F, C, D = 70, 9, 5
    x, gmm = M.mixture(3, F, D, C)
    block = G.FrameBlock([x])
    dg = G.DeviceGmm(gmm)
    good, _ = block.gselect(dg, 4)
    bad = good.copy()
    bad[37, 2] = C if bad_index == 'C' else -1
    for call in (lambda sel: block.gselect(dg, 2, preselect=sel),
                 lambda sel: block.selection_posteriors(dg, sel),
                 lambda sel: block.selection_posteriors(dg, sel, 0.01)):
        before = call(good)
        with pytest.raises(ValueError, match='index out of range'):
            call(bad)
        after = call(good)
        for a, b in zip(before, after):
            assert np.array_equal(M.bits(a), M.bits(b))
