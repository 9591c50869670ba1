"""DTW distances, the host side: the float64 statement (tests/dtw_f64.py) against known answers, against the
enumeration of every monotone path, and its two forms against each other; the selection of items by time; every
argument error of ``dtw_distances`` (none needs a device); ``DeviceFeaturesCollection.from_host``'s refusals."""

import types

import numpy as np
import pytest

import dtw_cases
import dtw_f64
from shennong_amd import FeaturesCollection, dtw_distances
from shennong_amd import dtw as dtw_module
from shennong_amd.device import DeviceFeaturesCollection
from shennong_amd.features import Features


# ---- the statement ----------------------------------------------------------------------------------------
def test_known_answers():
    assert dtw_f64.dtw([[1, 0]], [[0, 1]], 'cosine') == (0.5, 1)
    x = np.random.default_rng(1).standard_normal((9, 5)).astype(np.float32)
    distance, length = dtw_f64.dtw(x, x, 'cosine')
    assert length == 9 and abs(distance) < 1e-7   # (float64 arccos near 1: sqrt(2 * 2^-53) / pi per frame)
    assert dtw_f64.dtw(x, x, 'sqeuclidean') == (0.0, 9)
    zeros = np.zeros((2, 3), dtype=np.float32)
    assert dtw_f64.dtw(zeros, zeros, 'sqeuclidean') == (0.0, 2)   # the diagonal wins the tie
    assert dtw_f64.dtw(zeros, zeros, 'sqeuclidean', loop=True) == (0.0, 2)
    # cosine of zero rows: 1 against a nonzero row, 0 against another zero row
    d = dtw_f64.frame_distances([[0, 0], [1, 0]], [[0, 0], [0, 2]], 'cosine')
    assert d.tolist() == [[0.0, 1.0], [1.0, 0.5]]
    assert dtw_f64.dtw([[3, 4]], [[0, 1], [1, 0]], 'sqeuclidean', normalized=False) == (18.0 + 20.0, 2)


def test_up_wins_its_tie_with_left_where_the_diagonal_is_dearer():
    d = np.zeros((3, 4))
    d[1, 2] = 1.0
    for form in (dtw_f64.tables_loop, dtw_f64.tables):
        C, L = form(d)
        # at (2, 3): the diagonal (1, 2) costs 1, (1, 3) and (2, 2) cost 0 with lengths 4 and 3
        assert (C[1, 2], C[1, 3], C[2, 2]) == (1.0, 0.0, 0.0) and (L[1, 3], L[2, 2]) == (4, 3)
        assert (C[2, 3], L[2, 3]) == (0.0, 5)
    assert dtw_f64.path_margin(d) == 0.0
    # ... and with the roles of the items swapped the last two priorities swap: the transposed lattice, read by
    # the same rule, takes (i-1, j) = the other item's step and finds the other length
    C, L = dtw_f64.tables(d.T)
    assert (C[3, 2], L[3, 2]) == (0.0, 4)


def _cheapest_path(d):
    """The minimum cost over every monotone path from (0, 0) to (N-1, M-1), by enumeration"""
    n, m = d.shape

    def walk(i, j):
        if i == n - 1 and j == m - 1:
            return d[i, j]
        tails = [walk(a, b) for a, b in ((i + 1, j + 1), (i + 1, j), (i, j + 1)) if a < n and b < m]
        return d[i, j] + min(tails)
    return walk(0, 0)


def test_statement_finds_the_cheapest_monotone_path():
    rng = np.random.default_rng(5)
    for n in range(1, 6):
        for m in range(1, 6):
            # (small integers: sums are exact in any order, and ties are frequent)
            d = rng.integers(0, 4, size=(n, m)).astype(np.float64)
            C, L = dtw_f64.tables(d)
            assert C[-1, -1] == _cheapest_path(d), (n, m)
            assert max(n, m) <= L[-1, -1] <= n + m - 1


@pytest.mark.parametrize('metric', dtw_f64.METRICS)
def test_loop_form_equals_vectorised_form(metric):
    kind = 'int' if metric == 'sqeuclidean' else 'normal'
    xs, ys = dtw_cases.item_sets(kind, 3, seed=11)
    for a, b in ((0, 0), (1, 2), (2, 5), (4, 3), (6, 7), (7, 4), (3, 8), (8, 2)):   # up to 129 x 31
        d = dtw_f64.frame_distances(xs[a], ys[b], metric)
        loop, fast = dtw_f64.tables_loop(d), dtw_f64.tables(d)
        assert np.array_equal(loop[0], fast[0]) and np.array_equal(loop[1], fast[1])


def test_exact_cases_hold_ties_on_the_path():
    """The integer data of the GPU suite's exact test really exercises the tie rule"""
    shapes = dtw_cases.pair_shapes().tolist()
    _, _, (cost, length, margin, _) = dtw_cases.exact_case(1)
    assert margin[shapes.index([33, 129])] == 0.0 and margin[shapes.index([129, 33])] == 0.0
    for dim, tied in ((1, 50), (3, 20)):   # pairs whose optimal path passes a tie between different lengths
        _, _, (cost, length, margin, _) = dtw_cases.exact_case(dim)
        assert (margin == 0).sum() >= tied
        assert (cost == np.round(cost)).all() and cost.max() < 2 ** 24


def test_cosine_cases_keep_their_conditions():
    """The seeds of the GPU suite's cosine test: no pair near |cos| = 1, no path near a change of length"""
    for dim in (7, 13):
        _, _, (_, _, margin, cosine) = dtw_cases.cosine_case(dim)
        assert cosine.max() <= dtw_cases.MAX_COS and margin.min() >= dtw_cases.MIN_MARGIN


# ---- items by time ----------------------------------------------------------------------------------------
def _two_layouts():
    rng = np.random.default_rng(2)
    data = rng.standard_normal((20, 4)).astype(np.float32)
    start = np.arange(20) / 64.0   # (binary fractions: the centre times below are exact)
    pairs = Features(data, np.stack([start, start + 2 / 64.0], axis=1), validate=False)   # centres 1/64, 2/64, ...
    single = Features(data.copy(), start + 1 / 64.0, validate=False)                        # the same centres
    return FeaturesCollection([('pad', dtw_cases.features(data[:3])), ('a', pairs), ('b', single)])


def test_item_selection_by_times_is_inclusive_in_both_layouts():
    feats = _two_layouts()
    centre = lambda k: (k + 1) / 64.0   # noqa: E731
    items = [('a', centre(2), centre(5)),          # both ends are centre times: rows 2 .. 5
             ('b', centre(2), centre(5)),
             ('a', centre(2) + 1e-9, centre(5) - 1e-9),   # just inside: rows 3 .. 4
             ('b', 0.0, 10.0),                     # everything
             ('a', centre(7), centre(7))]          # one frame
    first, count, pairs, dim, block = dtw_module._select(feats, np.array([[0, 1], [2, 3]]), items)
    # (rows of the one block in collection order: 'pad' has 3, 'a' starts at 3, 'b' at 23)
    assert first.tolist() == [3 + 2, 23 + 2, 3 + 3, 23, 3 + 7]
    assert count.tolist() == [4, 4, 2, 20, 1] and count.dtype == np.int32
    assert pairs.tolist() == [[0, 1], [2, 3]] and pairs.dtype == np.int32
    assert dim == 4 and block is None


def test_items_default_to_whole_utterances():
    feats = _two_layouts()
    first, count, pairs, dim, _ = dtw_module._select(feats, [('b', 'a'), ('b', 'pad'), ('a', 'b')], None)
    assert first.tolist() == [23, 3, 0] and count.tolist() == [20, 20, 3]
    assert pairs.tolist() == [[0, 1], [0, 2], [1, 0]]


# ---- argument errors: all before any device work ----------------------------------------------------------
def _fake_device_collection(dims):
    """A device collection over blocks that have no memory behind them"""
    template = FeaturesCollection()
    blocks = []
    for k, dim in enumerate(dims):
        name = 'utt{}'.format(k)
        template[name] = Features._of_batch(np.broadcast_to(np.float32(0), (5, dim)),
                                            0.01 * np.arange(5), {}, None)
        blocks.append((types.SimpleNamespace(ptr=4096, device=0, free=lambda: None), [name], dim))
    return DeviceFeaturesCollection._build(template, blocks)


def test_argument_errors_name_the_offender():
    feats = _two_layouts()
    with pytest.raises(ValueError, match='invalid metric "kl"'):
        dtw_distances(feats, [('a', 'b')], metric='kl')
    with pytest.raises(ValueError, match='utterance "nope" is not in the collection'):
        dtw_distances(feats, [('a', 'nope')])
    with pytest.raises(ValueError, match='item 1: utterance "nope" is not in the collection'):
        dtw_distances(feats, np.array([[0, 1]]), items=[('a', 0, 1), ('nope', 0, 1)])
    with pytest.raises(ValueError, match=r'pair 1 \(0, 2\) is out of range for 2 items'):
        dtw_distances(feats, np.array([[0, 1], [0, 2]]), items=[('a', 0, 1), ('b', 0, 1)])
    with pytest.raises(ValueError, match=r'pair 0 \(-1, 0\) is out of range'):
        dtw_distances(feats, np.array([[-1, 0]]), items=[('a', 0, 1), ('b', 0, 1)])
    with pytest.raises(ValueError, match='integer array'):
        dtw_distances(feats, np.array([[0.0, 1.0]]), items=[('a', 0, 1), ('b', 0, 1)])
    with pytest.raises(ValueError, match=r'item 1 \("b", 0.5, 0.6\) has no frames'):
        dtw_distances(feats, np.array([[0, 1]]), items=[('a', 0, 1), ('b', 0.5, 0.6)])
    empty = FeaturesCollection([('a', dtw_cases.features(np.zeros((4, 3)))),
                                ('e', Features(np.zeros((0, 0), dtype=np.float32), np.zeros((0, 2)),
                                               validate=False))])
    with pytest.raises(ValueError, match='utterance "e" has no frames'):
        dtw_distances(empty, [('a', 'e')])
    long = FeaturesCollection([('a', dtw_cases.features(np.zeros((dtw_module.MAX_FRAMES + 1, 2)))),
                               ('b', dtw_cases.features(np.zeros((4, 2))))])
    with pytest.raises(ValueError, match='utterance "a" has 4097 frames, the limit is 4096'):
        dtw_distances(long, [('b', 'a')])
    mixed = FeaturesCollection([('a', dtw_cases.features(np.zeros((4, 3)))),
                                ('b', dtw_cases.features(np.zeros((4, 5))))])
    with pytest.raises(ValueError, match=r'items have different ndims: \[3, 5\]'):
        dtw_distances(mixed, [('a', 'b')])
    with pytest.raises(ValueError, match=r'items have different ndims: \[3, 5\]'):
        dtw_distances(_fake_device_collection([3, 5]), [('utt0', 'utt1')])
    with pytest.raises(ValueError, match=r'the utterances lie in 2 device blocks \(one per sample rate\)'):
        dtw_distances(_fake_device_collection([3, 3]), [('utt0', 'utt1')])


def test_no_pairs_give_empty_arrays():
    feats = _two_layouts()
    distances, lengths = dtw_distances(feats, [], return_lengths=True)
    assert distances.shape == (0,) and distances.dtype == np.float32
    assert lengths.shape == (0,) and lengths.dtype == np.int32
    got = dtw_distances(feats, np.zeros((0, 2), dtype=np.int64), items=[('a', 0, 1)], metric='sqeuclidean')
    assert got.shape == (0,) and got.dtype == np.float32


def test_from_host_refuses_mixed_ndims_and_other_types():
    mixed = FeaturesCollection([('a', dtw_cases.features(np.zeros((4, 3)))),
                                ('b', dtw_cases.features(np.zeros((4, 5))))])
    with pytest.raises(ValueError, match=r'utterances have different ndims: \[3, 5\]'):
        DeviceFeaturesCollection.from_host(mixed)
    doubles = FeaturesCollection([('a', Features(np.zeros((4, 3)), 0.01 * np.arange(4), validate=False))])
    with pytest.raises(ValueError, match='utterance "a": data must be a float32 matrix'):
        DeviceFeaturesCollection.from_host(doubles)


def test_abi_refuses_bad_arguments_before_any_device_work():
    """snf_dtw_pairs returns SNF_E_INVALID (a ValueError here) without asking for a device: this runs anywhere"""
    from shennong_amd import _backend
    ok_first, ok_count, ok_pairs = [0, 4], [4, 3], [[0, 1]]
    cases = [
        (dict(dim=0), 'dim must be in'),
        (dict(item_count=[4, 0]), 'item 1 has no frames'),
        (dict(item_count=[4, 4097]), 'item 1 has 4097 frames, the limit is 4096'),
        (dict(item_first=[-1, 4]), 'item 0 starts outside the block'),
        (dict(pairs=[[0, 2]]), r'pair 0 \(0, 2\) is out of range for 2 items'),
        (dict(pairs=[[0, 1], [-1, 0]]), r'pair 1 \(-1, 0\) is out of range'),
        (dict(item_first=[], item_count=[], pairs=np.zeros((0, 2))), 'number of items out of range'),
    ]
    for change, message in cases:
        args = dict(dim=3, item_first=ok_first, item_count=ok_count, pairs=ok_pairs)
        args.update(change)
        with pytest.raises(ValueError, match=message):
            _backend.dtw_pairs(4096, args['dim'], args['item_first'], args['item_count'], args['pairs'],
                               'cosine', 4096, 8192)
    with pytest.raises(ValueError, match='invalid metric'):
        _backend.dtw_pairs(4096, 3, ok_first, ok_count, ok_pairs, 'kl', 4096, 8192)
    # (no pair: nothing to do, whatever the pointers are - and no device is asked for)
    _backend.dtw_pairs(0, 3, ok_first, ok_count, np.zeros((0, 2)), 'cosine', 0, 0)
