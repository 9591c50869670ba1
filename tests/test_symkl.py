"""The symkl metric and snf_gmm_posteriors without a GPU: the metric is accepted where no device is asked for, the
export refuses bad arguments before any device work, the float64 statement (tests/symkl_f64.py) agrees with itself
and with known values, and the case file (tests/symkl_cases.py) meets the conditions its bounds are derived under."""

import ctypes as C
import os

import numpy as np
import pytest

import dtw_cases
import dtw_f64
import symkl_cases
import symkl_f64
from shennong_amd import _backend, dtw_distances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the metric is accepted ------------------------------------------------------------------------------
def test_the_backend_accepts_symkl_on_the_no_pair_path():
    assert _backend.DTW_METRICS['symkl'] == 2
    assert _backend.dtw_pairs(0, 3, [0, 4], [4, 3], np.zeros((0, 2)), 'symkl', 0, 0) is None


def test_an_empty_pair_list_gives_an_empty_array():
    feats = dtw_cases.collection([np.full((4, 3), 1 / 3, dtype=np.float32)])
    got = dtw_distances(feats, np.zeros((0, 2), np.int64), metric='symkl')
    assert got.shape == (0,) and got.dtype == np.float32
    got, lengths = dtw_distances(feats, [], metric='symkl', normalized=False, return_lengths=True)
    assert got.shape == (0,) and lengths.shape == (0,) and lengths.dtype == np.int32


def test_the_c_call_names_the_metric_and_still_refuses_others():
    first, count = (C.c_int64 * 1)(0), (C.c_int32 * 1)(4)
    lib = _backend.lib()
    assert lib.snf_dtw_pairs(0, None, 3, first, count, 1, None, 0, 2, None, None, None) == 0
    assert lib.snf_dtw_pairs(0, None, 3, first, count, 1, None, 0, 3, None, None, None) == -1
    assert '2 (symkl)' in lib.snf_last_error().decode()


# ---- 2. the export of the dense posteriors --------------------------------------------------------------------
def test_snf_gmm_posteriors_is_exported_and_declared():
    assert 'snf_gmm_posteriors' in _backend.EXPORTS and hasattr(_backend.lib(), 'snf_gmm_posteriors')
    with open(os.path.join(ROOT, 'include', 'shennong_amd.h')) as header:
        text = header.read()
    assert 'int snf_gmm_posteriors(int device_id, const float* d_x, int64_t n_frames, int32_t dim,' in text
    assert '#define SNF_DTW_SYMKL 2' in text and '#define SNF_DTW_SYMKL_FLOOR 0x1p-40f' in text


def test_snf_gmm_posteriors_refuses_bad_arguments_before_any_device_work():
    one = C.c_void_p(16)   # never dereferenced: every check below fails before any device work
    call = _backend.lib().snf_gmm_posteriors

    def refused(*args):
        rc = call(*args)
        return rc, _backend.lib().snf_last_error().decode()
    rc, msg = refused(0, one, 10, 3, None, one, one, 4, one, None, None)
    assert rc == -1 and 'null model buffer' in msg
    rc, msg = refused(0, None, 10, 3, one, one, one, 4, one, None, None)
    assert rc == -1 and 'null frames buffer' in msg
    rc, msg = refused(0, one, 10, 3, one, one, one, 4, None, None, None)
    assert rc == -1 and 'null output buffer' in msg
    rc, msg = refused(0, one, 10, 0, one, one, one, 4, one, None, None)
    assert rc == -1 and 'dimension' in msg
    rc, msg = refused(0, one, 10, 3, one, one, one, 0, one, None, None)
    assert rc == -1 and 'Gaussians' in msg
    rc, msg = refused(0, one, -1, 3, one, one, one, 4, one, None, None)
    assert rc == -1 and 'frames < 0' in msg
    rc, msg = refused(0, one, 10, 3, one, one, one, 4, C.c_void_p(18), None, None)
    assert rc == -1 and 'aligned' in msg
    # (no frames: nothing to do, and no device is asked for)
    assert call(0, None, 0, 3, one, one, one, 4, None, None, None) == 0


# ---- 3. the statement against itself --------------------------------------------------------------------------
@pytest.mark.parametrize('kind', symkl_cases.KINDS)
@pytest.mark.parametrize('dim', [1, 2, 7, 65])
def test_the_loop_form_equals_the_vectorised_form(kind, dim):
    xs, ys = symkl_cases.item_sets(kind, dim, seed=5)
    x, y = xs[2][:9], ys[3][:11]
    loop, fast = symkl_f64.frame_distances_loop(x, y), symkl_f64.frame_distances(x, y)
    assert loop.shape == fast.shape == (9, 11)
    # (the same non-negative terms, added in another order: dim additions of float64)
    assert (np.abs(loop - fast) <= dim * 2.0 ** -52 * loop).all()
    if dim < 8:   # (numpy adds fewer than 8 values in order: the same additions)
        assert np.array_equal(loop, fast)


def test_known_values():
    assert symkl_f64.FLOOR == 2.0 ** -40 and np.float32(symkl_f64.FLOOR) == symkl_f64.FLOOR
    xs, ys = symkl_cases.item_sets('floored', 9)
    for x in (xs[4], ys[7]):
        d = symkl_f64.frame_distances(x, x)
        assert (np.diag(d) == 0).all()   # equal rows: every term is exactly 0
        assert (symkl_f64.frame_distances(x, ys[5]) >= 0).all()
    half, quarter = np.array([[0.5]], np.float32), np.array([[0.25]], np.float32)
    # 0.5 (0.5 - 0.25) (ln 0.5 - ln 0.25) = 0.125 ln 2
    assert abs(symkl_f64.frame_distances(half, quarter)[0, 0] - 0.125 * np.log(2)) <= 1e-16
    assert symkl_f64.dtw(half, quarter, normalized=False) == (symkl_f64.frame_distances(half, quarter)[0, 0], 1)
    # a zero and a negative entry both count as the floor
    y = np.array([[0.2, 0.3, 0.5]], np.float32)
    with_zero, with_negative = np.array([[0.6, 0.0, 0.4]], np.float32), np.array([[0.6, -0.7, 0.4]], np.float32)
    with_floor = np.array([[0.6, 2.0 ** -40, 0.4]], np.float32)
    d = [symkl_f64.frame_distances(x, y)[0, 0] for x in (with_zero, with_negative, with_floor)]
    assert d[0] == d[1] == d[2] > 0
    # rows need not sum to 1
    assert symkl_f64.frame_distances(3 * y, y)[0, 0] > 0


def test_the_recursion_is_the_one_of_the_other_metrics():
    xs, ys = symkl_cases.item_sets('plain', 7)
    x, y = xs[4], ys[2]
    d = symkl_f64.frame_distances(x, y)
    C_loop, L_loop = dtw_f64.tables_loop(d)
    assert symkl_f64.dtw(x, y, normalized=False) == (C_loop[-1, -1], L_loop[-1, -1])
    assert symkl_f64.dtw(x, y) == (C_loop[-1, -1] / L_loop[-1, -1], L_loop[-1, -1])


# ---- 4. the case file checks itself ---------------------------------------------------------------------------
def test_the_recipe_of_the_items():
    for kind in symkl_cases.KINDS:
        xs, ys = symkl_cases.item_sets(kind, 8)
        assert [m.shape for m in xs] == [m.shape for m in ys] == [(n, 8) for n in dtw_cases.LENGTHS]
        rng = np.random.default_rng(0)   # the ten x items first, then the ten y items
        for m in xs + ys:
            z = 2 * rng.standard_normal(m.shape)
            e = np.exp(z - z.max(axis=1, keepdims=True))
            want = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
            assert m.dtype == np.float32
            if kind == 'floored':
                mask = rng.random(m.shape) < 0.2
                mask[np.arange(m.shape[0]), want.argmax(axis=1)] = False
                want[mask] = 0
                assert (m.max(axis=1) > 0).all()
            assert np.array_equal(m, want)
        zeros = sum(int((m == 0).sum()) for m in xs + ys)
        assert (zeros > 0) == (kind == 'floored')


@pytest.mark.parametrize('kind', symkl_cases.KINDS)
@pytest.mark.parametrize('dim', symkl_cases.DIMS)
def test_enough_pairs_qualify_on_the_statement(kind, dim):
    xs, ys, (cost, length, margin, max_a, limit), qualifying = symkl_cases.case(kind, dim)
    shapes = dtw_cases.pair_shapes()
    n, m = shapes[:, 0], shapes[:, 1]
    assert np.array_equal(limit, (n + m - 1) * (2 * dim + 8) * 2.0 ** -24 * max_a + (n + m) * 2.0 ** -24 * cost)
    assert np.array_equal(qualifying, margin >= 2 * limit)
    print(kind, dim, 'qualifying pairs:', int(qualifying.sum()), 'largest bound / cost: %.3g' %
          (limit / np.maximum(cost, 1e-300)).max())
    assert qualifying.sum() >= symkl_cases.MIN_QUALIFYING
    assert (cost >= 0).all() and (length >= np.maximum(n, m)).all() and (length <= n + m - 1).all()


def test_the_long_utterance_selects_the_items():
    from shennong_amd import dtw as dtw_module
    xs, ys = symkl_cases.item_sets('plain', 2)
    feats, items, pairs = symkl_cases.one_long_utterance(xs, ys)
    first, count, got_pairs, dim, _ = dtw_module._select(feats, pairs, items)
    lengths = [m.shape[0] for m in xs + ys]
    assert count.tolist() == lengths and first.tolist() == np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    assert dim == 2 and np.array_equal(got_pairs, pairs)
