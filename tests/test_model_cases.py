"""CPU half of tests/test_gmm_seams_gpu.py and tests/test_vtln_seams_gpu.py: the cases of tests/model_cases.py reach
the boundaries they were chosen for (Python restatements of the host scheduling), their derived scales are usable,
and the two-matmul form of lvtln_f64.compute_transform equals the plain one.  numpy only, no device."""

import numpy as np
import pytest

import gmm_f64 as RG
import lvtln_f64 as RV
import model_cases as M


def test_the_chunked_estep_case_has_22_chunks_of_3_tiles():
    F, C, D = M.CHUNKED
    assert (F + 63) // 64 == 65 and F % 64 == 33            # 65 tiles, the last partial
    assert ((C + 63) // 64) * ((2 * D + 1 + 127) // 128) == 64   # workgroups per chunk
    assert M.stats_chunks(F, C, D) == (22, 3, 2)
    # the seam shapes stay in one chunk per tile or fewer: every tile count from 1 to 3 occurs
    assert sorted({M.stats_chunks(F, 129, 64)[0] for F in M.ESTEP_FRAMES}) == [1, 2, 3]
    # two column blocks of gmm_stats_kernel from D = 64 on only
    assert [(2 * D + 1 + 127) // 128 for D in M.GMM_DIMS] == [1, 1, 1, 1, 1, 2]
    # one, one and two k-chunks of dense_block around D = 32
    assert [(((2 * D + 3) & ~3) + 63) // 64 for D in (31, 32, 33)] == [1, 1, 2]


def test_the_scratch_case_crosses_the_block_of_16384_frames():
    F, C, D = M.SCRATCH
    rows = M.gselect_rows(F, C)
    assert rows == 16384
    assert F - rows == 65 and M.SCRATCH_TAIL < rows < F
    assert F - M.SCRATCH_TAIL == 67
    assert M.gselect_rows(67, C) == 128                      # the small block is one scratch block
    # no gselect shape of the seam tests reaches a second block
    assert all(M.gselect_rows(f, c) >= f for f in M.SEAM_FRAMES for c in M.SEAM_GAUSSIANS)


def test_item_counts_around_2048_frames():
    assert [M.item_count(n) for n in M.LONG_LENS] == [1, 1, 2, 2, 3]
    assert [M.item_count(n) for n in (0, 1)] == [0, 1]
    assert [M.item_count(n) for n in M.GRAM_LONG_FRAMES] == [1, 1, 2, 3]
    assert sum(M.item_count(n) > 1 for n in M.MIXED_LENS) == 1
    assert M.MIXED_LENS[0] == M.MIXED_LENS[5] == M.MIXED_LENS[-1] == 0 and len(M.MIXED_LENS) == 12
    # column groups of 64 of the two products: two at V = D + 1 = 65, three at V = 2 D + 1 = 129, at D = 64 only
    assert [(D + 1 + 63) // 64 for D in M.VTLN_DIMS] == [1] * 8 + [2]
    assert [(2 * D + 1 + 63) // 64 for D in M.VTLN_DIMS] == [1] * 5 + [1, 2, 2, 3]
    # passes of 32 classes of the class search
    assert [(c + 31) // 32 for _, c in M.SELECT_CASES] == [1, 1, 1, 2, 2, 3, 2, 2]


def test_the_zero_weight_model_has_two_infinite_gconsts():
    x, gmm = M.zero_weight_case()
    assert x.shape == (65, 3) and gmm.num_gauss() == 17
    gc = gmm.gconsts()
    assert not np.isnan(gc).any()
    assert list(np.nonzero(np.isneginf(gc))[0]) == list(M.ZERO_WEIGHT)
    assert np.isfinite(np.delete(gc, M.ZERO_WEIGHT)).all()
    L = RG.loglikes(x, *M.model64(gmm))
    assert np.isneginf(L[:, M.ZERO_WEIGHT]).all() and not np.isnan(L).any()
    # the reference puts them last, the higher index first
    assert (RG.gselect(L, 17)[:, -2:] == [11, 4]).all()


def test_the_default_configuration_case_has_a_clear_winner():
    case = M.default_config_case()
    lvtln = case['lvtln']
    assert lvtln.num_classes() == 41 == int(1.5 + (1.25 - 0.85) / 0.01)
    assert lvtln.default_class == 15 == int(0.5 + (1 - 0.85) / 0.01)
    assert lvtln.dim() == 39 and len(case['offsets']) == 4
    for objs, best, W in M.default_config_reference(case):
        assert M.top_two_margin(objs) > 1e-6
        assert best == int(np.argmax(objs)) and W.shape == (39, 40)
    # both passes hold a winner somewhere, or the case would not tell a lost carry from a kept one
    winners = [best for _, best, _ in M.default_config_reference(case)]
    assert min(winners) < 32 <= max(winners), winners


def test_the_estep_scales_are_positive_where_a_gaussian_has_occupancy():
    for D in (1, 33, 64):
        for F, C in ((63, 17), (129, 129)):
            x, gmm = M.seam_mixture(F, C, D)
            L = RG.loglikes(x, *M.model64(gmm)).astype(np.float32)
            for w in (None, M.estep_weights(F)):
                occ = RG.accumulate(x, L, w)[0]
                T, floor = M.estep_scale(x, L, w)
                assert T.shape == floor.shape == (C, 2 * D + 1)
                assert (T[occ > 0] > 0).all() and (T >= 0).all() and np.isfinite(T).all()
                # where a Gaussian holds a thousandth of a frame, the floor is nothing beside T
                assert (floor[occ > 1e-3] <= 1e-15 * T[occ > 1e-3]).all()
    w = M.estep_weights(64)
    assert w[0] == 0 and w[-1] == 0 and (w[1:-1] > 0).all() and w.max() < 2


@pytest.mark.parametrize('D', [1, 5, 13])
def test_the_two_matmul_form_equals_the_five_index_sum(D):
    lvtln, gmm, x, sel, post, offsets = M.class_setup(D, 3, 3, 100 + D)
    for s in range(1, 3):
        a, b = offsets[s], offsets[s + 1]
        stats = RV.fmllr_stats(x[a:b], sel[a:b], post[a:b], gmm.means_invvars_, gmm.inv_vars_)
        for A in lvtln.A:
            plain = RV.apply_transform_to_stats(A, stats)
            fast = RV.apply_transform_to_stats(A, stats, fast=True)
            assert plain[0] == fast[0] and np.array_equal(plain[1], fast[1])
            assert np.abs(plain[2] - fast[2]).max() <= 1e-12 * np.abs(plain[2]).max()
        for norm_type in ('none', 'offset', 'diag'):
            want = RV.compute_transform(lvtln.A, lvtln.logdets, stats, norm_type, 0.5, 1)
            got = RV.compute_transform(lvtln.A, lvtln.logdets, stats, norm_type, 0.5, 1, fast=True)
            np.testing.assert_allclose(got[0], want[0], rtol=1e-12)
            assert got[1] == want[1] and got[3] == want[3]
            np.testing.assert_allclose(got[2], want[2], rtol=1e-12, atol=1e-12 * np.abs(want[0]).max())
            np.testing.assert_allclose(got[4], want[4], rtol=1e-12, atol=1e-12 * np.abs(want[4]).max())


@pytest.mark.parametrize('D', [1, 5, 13])
def test_the_matrix_product_form_of_the_fmllr_statistics_equals_the_plain_one(D):
    x, gmm, sel, post, _ = M.fmllr_case(D, 5, 16, (70,))
    plain = RV.fmllr_stats(x, sel, post, gmm.means_invvars_, gmm.inv_vars_)
    fast = RV.fmllr_stats(x, sel, post, gmm.means_invvars_, gmm.inv_vars_, fast=True)
    scale = RV.fmllr_stats(np.abs(x), sel, post, np.abs(gmm.means_invvars_), gmm.inv_vars_)[2]
    assert plain[0] == fast[0] and np.array_equal(plain[1], fast[1])
    assert fast[2].shape == (D, D + 1, D + 1) and (np.abs(plain[2] - fast[2]) <= 1e-12 * scale).all()
    assert RV.fmllr_stats(x[:0], sel[:0], post[:0], gmm.means_invvars_, gmm.inv_vars_, fast=True)[0] == 0.0


def test_the_objective_scale_bounds_the_objective():
    lvtln, gmm, x, sel, post, offsets = M.class_setup(13, 3, 2, 9)
    stats = RV.fmllr_stats(x, sel, post, gmm.means_invvars_, gmm.inv_vars_)
    for norm_type in ('none', 'offset', 'diag'):
        for scale in (0.0, 1.0):
            objs, scales = M.class_reference(lvtln.A, lvtln.logdets, stats, norm_type, scale)
            want = RV.compute_transform(lvtln.A, lvtln.logdets, stats, norm_type, scale, 1)[0]
            np.testing.assert_array_equal(objs, want)
            assert (scales >= np.abs(objs)).all()


def test_the_affine_apply_case_has_leading_trailing_and_consecutive_empty_segments():
    off = np.asarray(M.APPLY_OFFSETS)
    lens = np.diff(off)
    assert len(lens) == 7 and lens[0] == lens[1] == 0 and lens[3] == 0 and lens[-1] == 0
    x, W = M.apply_case(13, off)
    y, tol = M.apply_reference(x, W, off)
    assert y.shape == tol.shape == (300, 13) and (tol > 0).all()
    want = x[5:9].astype(np.float64) @ W[4][:, :13].astype(np.float64).T + W[4][:, 13]
    np.testing.assert_array_equal(y[5:9], want)
