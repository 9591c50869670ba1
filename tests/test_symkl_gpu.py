"""The symkl metric of snf_dtw_pairs on the GPU against the float64 statement (tests/symkl_f64.py) within the derived
bound of tests/symkl_cases.py: frame distances alone, the 100 pairs of every case at every seam of the kernel, items
as slices of one utterance from a host and a device collection, the three kernel classes, and ABX scores on top.
Measured worst errors per dim: profiles/symkl_errors.txt (tools/symkl_errors.py)."""

import numpy as np
import pytest

import abx_np
import dtw_cases
import symkl_cases
import symkl_f64
import test_abx_gpu
from shennong_amd import abx_scores, dtw_distances
from shennong_amd.device import DeviceFeaturesCollection

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a).view(np.uint32)


# ---- 1. frame distances alone -----------------------------------------------------------------------------------
def _single_rows(dim):
    """12 rows: 4 plain, 4 floored (zeros), 4 with negative entries where the floored ones have zeros"""
    rng = np.random.default_rng(50 + dim)
    z = 2 * rng.standard_normal((12, dim))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    mask = rng.random((12, dim)) < 0.3
    mask[np.arange(12), p.argmax(axis=1)] = False
    mask[:4] = False
    p[mask] = 0
    p[8:][mask[8:]] = -rng.random(int(mask[8:].sum())).astype(np.float32)
    if dim == 1:   # (a softmax of one entry is 1: rows need not sum to 1)
        p = rng.random((12, 1)).astype(np.float32)
        p[4:8:2] = 0
        p[8::2] *= -1
    return p


@pytest.mark.parametrize('dim', [1, 2, 7, 8, 9, 40, 65])
def test_frame_distances_alone(gpu, dim):
    rows = _single_rows(dim)
    feats = dtw_cases.collection([row[None, :] for row in rows])
    names = list(feats)
    pairs = [(a, b) for a in names for b in names]
    got, length = dtw_distances(feats, pairs, metric='symkl', normalized=False, return_lengths=True)
    want = symkl_f64.frame_distances(rows, rows).reshape(-1)
    limit = symkl_cases.bound(dim, 1, 1, symkl_f64.magnitudes(rows, rows).reshape(-1), want)
    error = np.abs(got.astype(np.float64) - want)
    print('dim', dim, 'worst error %.3g, worst error / bound %.3g' % (error.max(), (error / limit).max()))
    assert (length == 1).all() and (got >= 0).all()
    assert (error <= limit).all(), (np.flatnonzero(error > limit)[:5], error.max())
    # a negative entry counts as the floor, as a zero does
    assert (rows < 0).any() and (rows == 0).any()
    clipped = np.maximum(rows, 0)
    again = dtw_distances(dtw_cases.collection([row[None, :] for row in clipped]), pairs, metric='symkl',
                          normalized=False)
    assert np.array_equal(_bits(again), _bits(got))


def test_equal_one_dimensional_rows_of_one_give_exactly_zero(gpu):
    one = np.ones((1, 1), dtype=np.float32)
    feats = dtw_cases.collection([one, one.copy()])
    got, length = dtw_distances(feats, [('item0', 'item1'), ('item1', 'item0'), ('item0', 'item0')], metric='symkl',
                                normalized=False, return_lengths=True)
    assert _bits(got).tolist() == [0, 0, 0] and length.tolist() == [1, 1, 1]


# ---- 2. the 100 pairs of every case, and the same pairs as slices of one utterance ------------------------------
def _check_case(got, got_length, made, qualifying, what):
    cost, length, margin, max_a, limit = made
    error = np.abs(got.astype(np.float64) - cost)
    print(what, 'worst cost error %.3g, worst error / bound %.3g; qualifying %d' %
          (error.max(), (error / limit).max(), int(qualifying.sum())))
    assert (error <= limit).all(), (np.flatnonzero(error > limit)[:5], error.max())
    q = qualifying
    assert np.array_equal(got_length[q], length[q]), np.flatnonzero(q & (got_length != length))[:5]
    # (the float32 division's half ulp fits: the bound's (N + M) 2^-24 cost covers len - 1 <= N + M - 2 additions)
    normalised = got / got_length.astype(np.float32)
    assert (np.abs(normalised.astype(np.float64) - cost / length)[q] <= (limit / length)[q]).all()


@pytest.mark.parametrize('kind', symkl_cases.KINDS)
@pytest.mark.parametrize('dim', symkl_cases.COST_ONLY_DIMS + symkl_cases.DIMS)
def test_within_the_derived_bound_at_every_seam(gpu, kind, dim):
    xs, ys, made, qualifying = symkl_cases.case(kind, dim)
    if dim in symkl_cases.COST_ONLY_DIMS:   # (near ties abound: costs only)
        qualifying = np.zeros_like(qualifying)
    feats, pairs = dtw_cases.two_set_collection(xs, ys)
    got, got_length = dtw_distances(feats, pairs, metric='symkl', normalized=False, return_lengths=True)
    assert got.dtype == np.float32 and got_length.dtype == np.int32
    _check_case(got, got_length, made, qualifying, '%s dim %d:' % (kind, dim))
    assert np.array_equal(_bits(dtw_distances(feats, pairs, metric='symkl')),
                          _bits(got / got_length.astype(np.float32)))
    # the same pairs as slices of one long utterance, from the host and from the device
    long_feats, items, index_pairs = symkl_cases.one_long_utterance(xs, ys)
    from_host = dtw_distances(long_feats, index_pairs, items=items, metric='symkl', normalized=False,
                              return_lengths=True)
    resident = DeviceFeaturesCollection.from_host(long_feats)
    try:
        on_device = dtw_distances(resident, index_pairs, items=items, metric='symkl', normalized=False,
                                  return_lengths=True)
    finally:
        resident.release()
    assert np.array_equal(_bits(on_device[0]), _bits(from_host[0])) and np.array_equal(on_device[1], from_host[1])
    _check_case(from_host[0], from_host[1], made, qualifying, '%s dim %d, slices:' % (kind, dim))
    # (a pair's result does not depend on where its rows lie in the block)
    assert np.array_equal(_bits(from_host[0]), _bits(got)) and np.array_equal(from_host[1], got_length)


# ---- 3. every class and seam, costs only ------------------------------------------------------------------------
def _probabilities(rng, n, dim, floored):
    z = 2 * rng.standard_normal((n, dim))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    if floored:
        mask = rng.random((n, dim)) < 0.2
        mask[np.arange(n), p.argmax(axis=1)] = False
        p[mask] = 0
    return p


@pytest.mark.parametrize('n,m,dim', [(1000, 900, 3), (4096, 70, 65)])
def test_costs_across_many_strips_tiles_and_classes(gpu, n, m, dim):
    """1000 x 900 at D = 3: 16 strips, 29 column tiles, the class of the longest items.  4096 x 70 and 70 x 4096 at
    D = 65 (an odd D): 64 strips; 128 tiles and the whole seam row.  And every item against itself."""
    rng = np.random.default_rng(n + dim)
    x, y = _probabilities(rng, n, dim, True), _probabilities(rng, m, dim, False)
    feats = dtw_cases.collection([x, y])
    pairs = [('item0', 'item1'), ('item1', 'item0'), ('item0', 'item0'), ('item1', 'item1')]
    got, got_length = dtw_distances(feats, pairs, metric='symkl', normalized=False, return_lengths=True)
    forward = symkl_cases.pair_statement(x, y, margins=False)
    backward = symkl_cases.pair_statement(y, x, margins=False)
    for k, (cost, length, _, _, limit) in enumerate((forward, backward)):
        print(pairs[k], 'cost %.6g error %.3g bound %.3g' % (cost, abs(float(got[k]) - cost), limit))
        assert abs(float(got[k]) - cost) <= limit
        assert max(n, m) <= got_length[k] <= n + m - 1
    # an item against itself: the statement's cost is 0 along the diagonal
    for k, item in ((2, x), (3, y)):
        max_a = max(symkl_f64.magnitudes(item[a:a + 512], item).max() for a in range(0, item.shape[0], 512))
        limit = symkl_cases.bound(dim, item.shape[0], item.shape[0], max_a, 0.0)
        print(pairs[k], 'cost %.3g bound %.3g' % (got[k], limit))
        assert 0 <= got[k] <= limit


# ---- 4. ABX scores on top ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [test_abx_gpu.WITHIN, test_abx_gpu.ACROSS], ids=['within', 'across'])
def test_abx_scores_equal_the_statement_on_the_values_of_dtw_distances(gpu, kind):
    feats, items, mats = test_abx_gpu.corpus('normal')
    # (the rows of that corpus are standard normal: the negative entries count as the floor)
    n = len(items)
    triples = list(zip(items.names, items.onsets.tolist(), items.offsets.tolist()))
    pairs = np.array([(y, x) for y in range(n) for x in range(n)])
    dense = dtw_distances(feats, pairs, items=triples, metric='symkl').reshape(n, n)
    assert np.isfinite(dense).all() and (dense >= 0).all() and (dense > 0).any()
    rows = abx_np.table_rows(items.labels, kind['on'], kind['across'], kind['by'], lambda y, x: dense[y, x])
    table = abx_scores(feats, items, metric='symkl', **kind)
    test_abx_gpu._assert_table_equals_rows(table, rows, kind)
    resident = DeviceFeaturesCollection.from_host(feats)
    try:
        again = abx_scores(resident, items, metric='symkl', **kind)
    finally:
        resident.release()
    assert list(again.columns) == list(table.columns)
    for name in table.columns:
        assert np.array_equal(again[name], table[name]), name
    assert again['score'].tobytes() == table['score'].tobytes()
