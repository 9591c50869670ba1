"""Subsequence DTW search, the host side: the float64 statement (tests/dtw_search_f64.py) against answers worked by
hand, its two forms against each other, a planted copy, the margins of the ends; the selection of queries and
targets by time; every argument error of ``dtw_search`` and of snf_dtw_search (none needs a device); ``DtwMatches``."""

import numpy as np
import pytest

import dtw_cases
import dtw_search_cases
import dtw_search_f64
import test_dtw
from shennong_amd import DtwMatches, FeaturesCollection, dtw_search
from shennong_amd import dtw as dtw_module
from shennong_amd.features import Features

# d of the cases worked by hand below: at (1, 2) the left neighbour (1, 1) is the cheapest predecessor
HAND = np.array([[0, 4, 5], [3, 1, 0.25], [1, 1, 1]], dtype=np.float64)


# ---- the statement ----------------------------------------------------------------------------------------
def test_a_query_of_one_frame_is_the_arg_min_of_its_frame_distances():
    # d[0] = (3 - y)^2 = [4, 1, 1, 1]: every end has L = 1, the first of the minimal ones wins
    for normalized in (True, False):
        assert dtw_search_f64.search([[3]], [[5], [2], [4], [2]], 'sqeuclidean', normalized) == (1.0, 1.0, 1, 1, 1)
        assert dtw_search_f64.search([[3]], [[5], [2], [4], [2]], 'sqeuclidean', normalized, loop=True) == \
            (1.0, 1.0, 1, 1, 1)
    # cosine: [1, 0] against [0, 1], [1, 0], [1, 0]: d[0] = [0.5, 0, 0]
    assert dtw_search_f64.search([[1, 0]], [[0, 1], [1, 0], [1, 0]], 'cosine') == (0.0, 0.0, 1, 1, 1)
    # a target of one frame: every cell lies in column 0
    assert dtw_search_f64.search([[1], [2], [4]], [[2]], 'sqeuclidean') == (5.0 / 3.0, 5.0, 3, 0, 0)


def test_a_target_shorter_than_the_query():
    # x = 0, 1, 2 and y = 0, 2: d = [[0, 4], [1, 1], [4, 0]]
    #   row 0: C = [0, 4], L = [1, 1], B = [0, 1]
    #   (1, 0): up, C = 1, L = 2, B = 0;  (1, 1): the diagonal (0, 0) = 0 beats (0, 1) = 4 and (1, 0) = 1: C = 1, L = 2, B = 0
    #   (2, 0): up, C = 5, L = 3, B = 0;  (2, 1): the diagonal (1, 0) = 1 ties with up (1, 1) = 1 and wins: C = 1, L = 3
    x, y = [[0], [1], [2]], [[0], [2]]
    for form in (dtw_search_f64.tables_loop, dtw_search_f64.tables):
        C, L, B = form(dtw_search_f64.frame_distances(x, y, 'sqeuclidean'))
        assert C.tolist() == [[0, 4], [1, 1], [5, 1]]
        assert L.tolist() == [[1, 1], [2, 2], [3, 3]] and B.tolist() == [[0, 1], [0, 0], [0, 0]]
    assert dtw_search_f64.search(x, y, 'sqeuclidean') == (1.0 / 3.0, 1.0, 3, 0, 1)
    assert dtw_search_f64.search(x, y, 'sqeuclidean', normalized=False) == (1.0, 1.0, 3, 0, 1)


def test_normalisation_ranks_the_ends_and_does_not_change_the_paths():
    d = HAND[:2]
    for form in (dtw_search_f64.tables_loop, dtw_search_f64.tables):
        C, L, B = form(d)
        # (1, 1): the diagonal (0, 0) = 0.  (1, 2): the diagonal (0, 1) = 4, up (0, 2) = 5, left (1, 1) = 1: left
        assert C[1].tolist() == [3, 1, 1.25] and L[1].tolist() == [2, 2, 3] and B[1].tolist() == [0, 0, 0]
        # the cheaper end is 1; the longer path to end 2 has the smaller mean, 1.25 / 3 < 1 / 2
        assert dtw_search_f64.best_end(C[1], L[1], B[1], normalized=False) == (1.0, 1.0, 2, 0, 1)
        assert dtw_search_f64.best_end(C[1], L[1], B[1], normalized=True) == (1.25 / 3, 1.25, 3, 0, 2)
    # float32: the quotient and the comparison of the device
    got = dtw_search_f64.best_end(C[1], L[1], B[1], True, np.float32)
    assert got[0].dtype == np.float32 and got[0] == np.float32(1.25) / np.float32(3) and got[1:] == (1.25, 3, 0, 2)


def test_equal_scores_go_to_the_smallest_end_and_ties_to_the_diagonal():
    C, L, B = dtw_search_f64.tables(np.zeros((2, 3)))
    assert L[1].tolist() == [2, 2, 2] and B[1].tolist() == [0, 0, 1]
    assert dtw_search_f64.best_end(C[1], L[1], B[1]) == (0.0, 0.0, 2, 0, 0)


def test_loop_form_equals_diagonal_form_on_integer_distances_full_of_ties():
    rng = np.random.default_rng(12)
    ties = 0
    for n, m in ((1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (9, 5), (33, 20), (20, 65)):
        d = rng.integers(0, 3, size=(n, m)).astype(np.float64)
        loop, fast = dtw_search_f64.tables_loop(d), dtw_search_f64.tables(d)
        for a, b in zip(loop, fast):
            assert a.dtype == b.dtype and np.array_equal(a, b), (n, m)
        margin = dtw_search_f64.end_margins(*fast)
        assert np.array_equal(margin, dtw_search_f64.end_margins_loop(*fast)), (n, m)
        ties += int((margin == 0).sum())
    assert ties >= 20   # (ends whose path passes a tie between different lengths or starts)
    xs, ys = dtw_cases.item_sets('normal', 3, seed=11)
    for a, b in ((0, 0), (1, 2), (2, 5), (4, 3), (6, 1)):   # float distances, up to 64 x 32
        d = dtw_search_f64.frame_distances(xs[a], ys[b], 'cosine')
        loop, fast = dtw_search_f64.tables_loop(d), dtw_search_f64.tables(d)
        assert all(np.array_equal(u, v) for u, v in zip(loop, fast))
        assert np.array_equal(dtw_search_f64.end_margins(*fast), dtw_search_f64.end_margins_loop(*fast))


@pytest.mark.parametrize('n,before,after', [(1, 0, 0), (1, 3, 2), (5, 0, 4), (5, 4, 0), (40, 37, 61)])
def test_a_planted_copy_is_found_exactly(n, before, after):
    query, target = dtw_search_cases.planted(n, before, after, dim=3, seed=n)
    for normalized in (True, False):
        for loop in (True, False):
            if loop and n > 5:
                continue
            got = dtw_search_f64.search(query, target, 'sqeuclidean', normalized, loop)
            # (a row of 9s is at least 3 * 7^2 away from any row of the query: no other path costs 0)
            assert got == (0.0, 0.0, n, before, before + n - 1), (normalized, loop)


def test_end_margins_on_a_case_worked_by_hand():
    C, L, B = dtw_search_f64.tables(HAND)
    assert C[2].tolist() == [4, 2, 2] and L[2].tolist() == [3, 3, 3] and B[2].tolist() == [0, 0, 0]
    # end 0: column 0 has one predecessor per cell, nothing to decide
    # end 1: (2, 1) takes up (1, 1) = 1; the diagonal (1, 0) = 3 has the same (L, B) = (2, 0) and does not count,
    #        left (2, 0) = 4 has L = 3: gap 3.  (1, 1) takes the diagonal (0, 0) = 0; up (0, 1) = 4, left (1, 0) = 3:
    #        gap 3
    # end 2: (2, 2) takes the diagonal (1, 1) = 1; up (1, 2) = 1.25 has L = 3: gap 0.25
    for form in (dtw_search_f64.end_margins_loop, dtw_search_f64.end_margins):
        assert form(C, L, B).tolist() == [np.inf, 3.0, 0.25]
    # ... and of the two upper rows alone: (1, 2) takes left (1, 1) = 1 against the diagonal 4 and up 5
    assert dtw_search_f64.end_margins(C[:2], L[:2], B[:2]).tolist() == [np.inf, 3.0, 3.0]
    # a tie between predecessors of different starts: margin 0
    C, L, B = dtw_search_f64.tables(np.zeros((2, 2)))
    assert dtw_search_f64.end_margins(C, L, B).tolist() == [np.inf, 0.0]


def test_shared_cases_hold_ties_and_keep_their_conditions():
    """The integer data of the GPU suite's exact test exercises the tie rule and stays exact in float32; the cosine
    data keeps the conditions that the GPU test asserts before it looks at the device"""
    _, _, answers = dtw_search_cases.exact_case(3)
    assert len(answers) == 100 and max(a.max_cost for a in answers) < 2 ** 24
    different = sum(a.best(True, np.float32)[4] != a.best(False, np.float32)[4] for a in answers)
    assert different >= 10   # (pairs whose best end depends on the normalisation)
    _, _, answers = dtw_search_cases.cosine_case(7)
    margins = np.concatenate([a.margin for a in answers])
    assert margins.size == 6200 and (margins >= dtw_cases.MIN_MARGIN).mean() >= dtw_search_cases.MIN_QUALIFYING_ENDS
    assert max(a.max_cos for a in answers) <= dtw_cases.MAX_COS


# ---- queries and targets by time --------------------------------------------------------------------------
def test_selection_of_queries_and_targets_in_both_times_layouts():
    feats = test_dtw._two_layouts()
    centre = lambda k: (k + 1) / 64.0   # noqa: E731
    queries = [('a', centre(2), centre(5)),                  # both ends are centre times: rows 2 .. 5
               ('b', centre(2) + 1e-9, centre(5) - 1e-9),    # just inside: rows 3 .. 4
               ('a', centre(7), centre(7))]                  # one frame
    targets = ['b', ('a', 0.0, 10.0), ('b', centre(4), centre(19)), 'pad']
    first, count, pairs, n_queries, where, dim, block = dtw_module._select_search(feats, queries, targets, None)
    # (rows of the one block in collection order: 'pad' has 3, 'a' starts at 3, 'b' at 23)
    assert first.tolist() == [3 + 2, 23 + 3, 3 + 7, 23, 3, 23 + 4, 0] and first.dtype == np.int64
    assert count.tolist() == [4, 2, 1, 20, 20, 16, 3] and count.dtype == np.int32
    assert n_queries == 3 and dim == 4 and block is None
    assert where == [('b', 0), ('a', 0), ('b', 4), ('pad', 0)]
    # every query against every target, query-major
    assert pairs.dtype == np.int32 and pairs.tolist() == [[q, t] for q in range(3) for t in range(4)]
    chosen = dtw_module._select_search(feats, queries, targets, np.array([[2, 0], [0, 3]], dtype=np.int64))[2]
    assert chosen.dtype == np.int32 and chosen.tolist() == [[2, 0], [0, 3]]


# ---- argument errors: all before any device work ----------------------------------------------------------
def test_argument_errors_name_the_offender():
    feats = test_dtw._two_layouts()
    with pytest.raises(ValueError, match='invalid metric "kl"'):
        dtw_search(feats, ['a'], ['b'], metric='kl')
    with pytest.raises(ValueError, match='query 1: utterance "nope" is not in the collection'):
        dtw_search(feats, ['a', 'nope'], ['b'])
    with pytest.raises(ValueError, match='target 0: utterance "nope" is not in the collection'):
        dtw_search(feats, ['a'], [('nope', 0, 1)])
    with pytest.raises(ValueError, match=r'target 1: not an utterance name or \(name, onset, offset\)'):
        dtw_search(feats, ['a'], ['b', ('b', 0.5)])
    with pytest.raises(ValueError, match=r'pair 1 \(0, 2\) is out of range for 1 queries and 2 targets'):
        dtw_search(feats, ['a'], ['b', 'pad'], pairs=np.array([[0, 1], [0, 2]]))
    with pytest.raises(ValueError, match=r'pair 0 \(1, 0\) is out of range for 1 queries and 2 targets'):
        dtw_search(feats, ['a'], ['b', 'pad'], pairs=np.array([[1, 0]]))
    with pytest.raises(ValueError, match=r'pair 0 \(-1, 0\) is out of range'):
        dtw_search(feats, ['a'], ['b'], pairs=np.array([[-1, 0]]))
    with pytest.raises(ValueError, match='integer array'):
        dtw_search(feats, ['a'], ['b'], pairs=np.array([[0.0, 0.0]]))
    with pytest.raises(ValueError, match=r'query 0 \("b", 0.5, 0.6\) has no frames'):
        dtw_search(feats, [('b', 0.5, 0.6)], ['a'])
    empty = FeaturesCollection([('a', dtw_cases.features(np.zeros((4, 3)))),
                                ('e', Features(np.zeros((0, 0), dtype=np.float32), np.zeros((0, 2)),
                                               validate=False))])
    with pytest.raises(ValueError, match=r'target 0 \("e"\) has no frames'):
        dtw_search(empty, ['a'], ['e'])
    long = FeaturesCollection([('a', dtw_cases.features(np.zeros((dtw_module.MAX_FRAMES + 1, 2)))),
                               ('b', dtw_cases.features(np.zeros((4, 2))))])
    with pytest.raises(ValueError, match=r'target 0 \("a"\) has 4097 frames, the limit is 4096'):
        dtw_search(long, ['b'], ['a'])
    with pytest.raises(ValueError, match=r'query 0 \("a"\) has 4097 frames, the limit is 4096'):
        dtw_search(long, ['a'], ['b'])
    mixed = FeaturesCollection([('a', dtw_cases.features(np.zeros((4, 3)))),
                                ('b', dtw_cases.features(np.zeros((4, 5))))])
    with pytest.raises(ValueError, match=r'items have different ndims: \[3, 5\]'):
        dtw_search(mixed, ['a'], ['b'])
    with pytest.raises(ValueError, match=r'items have different ndims: \[3, 5\]'):
        dtw_search(test_dtw._fake_device_collection([3, 5]), ['utt0'], ['utt1'])
    with pytest.raises(ValueError, match=r'the utterances lie in 2 device blocks \(one per sample rate\)'):
        dtw_search(test_dtw._fake_device_collection([3, 3]), ['utt0'], ['utt1'])
    # curves of 2^31 elements or more: 4096 frames per pair, 2^19 pairs (the one target 2^19 times over)
    wide = FeaturesCollection([('q', dtw_cases.features(np.zeros((2, 2)))),
                               ('t', dtw_cases.features(np.zeros((4096, 2))))])
    pairs = np.zeros((2 ** 19, 2), dtype=np.int32)
    with pytest.raises(ValueError, match=r'the curves of the 524288 pairs hold 2147483648 elements'):
        dtw_search(wide, ['q'], ['t'], pairs=pairs, return_curves=True)


def test_no_pairs_give_empty_columns():
    feats = test_dtw._two_layouts()
    for kwargs in (dict(pairs=np.zeros((0, 2), dtype=np.int64)), dict(pairs=[]), dict(return_curves=True, pairs=[])):
        found = dtw_search(feats, ['a'], ['b'], **kwargs)
        assert len(found) == 0
        for name in DtwMatches.columns:
            assert getattr(found, name).shape == (0,), name
        assert found.score.dtype == found.cost.dtype == np.float32 and found.onset.dtype == np.float64
        assert found.query.dtype == found.end_frame.dtype == np.int32
    assert len(dtw_search(feats, [], ['b'])) == 0 and len(dtw_search(feats, ['a'], [])) == 0


def test_abi_refuses_bad_arguments_before_any_device_work():
    """snf_dtw_search returns SNF_E_INVALID (a ValueError here) without asking for a device: this runs anywhere"""
    from shennong_amd import _backend
    ok = dict(dim=3, item_first=[0, 4, 7], item_count=[4, 3, 5], pairs=[[0, 1], [0, 2]], metric='cosine')
    outputs = (4096, 8192, 12288, 16384)
    curves = dict(d_curve_cost=4096, d_curve_len=8192, d_curve_start=12288)
    cases = [
        (dict(dim=0), {}, 'dtw_search: dim must be in'),
        (dict(item_count=[4, 0, 5]), {}, 'item 1 has no frames'),
        (dict(item_count=[4, 4097, 5]), {}, 'item 1 has 4097 frames, the limit is 4096'),
        (dict(item_first=[-1, 4, 7]), {}, 'item 0 starts outside the block'),
        (dict(pairs=[[0, 3]]), {}, r'pair 0 \(0, 3\) is out of range for 3 items'),
        (dict(pairs=[[0, 1], [-1, 0]]), {}, r'pair 1 \(-1, 0\) is out of range'),
        (dict(item_first=[], item_count=[], pairs=np.zeros((0, 2))), {}, 'number of items out of range'),
        # curves: all pointers or none; every stretch inside [0, 2^31) and apart from the others
        ({}, dict(curve_first=[0, 3]), 'curve pointers must be all set or all null'),
        ({}, dict(curves, curve_first=None), 'curve pointers must be all set or all null'),
        ({}, dict(curves, d_curve_len=None, curve_first=[0, 3]), 'curve pointers must be all set or all null'),
        ({}, dict(curves, curve_first=[0, 2]), 'the curves of the pairs 0 and 1 overlap'),       # pair 0 has 3 ends
        ({}, dict(curves, curve_first=[5, 1]), 'the curves of the pairs 0 and 1 overlap'),       # pair 1 has 5 ends
        ({}, dict(curves, curve_first=[7, 7]), 'the curves of the pairs 0 and 1 overlap'),
        ({}, dict(curves, curve_first=[-1, 3]), r'the curve of pair 0 \(3 elements at -1\) lies outside'),
        ({}, dict(curves, curve_first=[0, 2 ** 31 - 4]),
         r'the curve of pair 1 \(5 elements at 2147483644\) lies outside \[0, 2\^31\)'),
        ({}, dict(curves, d_curve_cost=4097, curve_first=[0, 3]), 'a curve array is not 4-byte aligned'),
    ]
    for change, keywords, message in cases:
        args = dict(ok)
        args.update(change)
        with pytest.raises(ValueError, match=message):
            _backend.dtw_search(4096, args['dim'], args['item_first'], args['item_count'], args['pairs'],
                                args['metric'], True, *outputs, **keywords)
    with pytest.raises(ValueError, match='invalid metric'):
        _backend.dtw_search(4096, 3, ok['item_first'], ok['item_count'], ok['pairs'], 'kl', True, *outputs)
    with pytest.raises(ValueError, match='curve_first has 1 entries for 2 pairs'):
        _backend.dtw_search(4096, 3, ok['item_first'], ok['item_count'], ok['pairs'], 'cosine', True, *outputs,
                            curve_first=[0], **curves)
    with pytest.raises(ValueError, match='d_cost, d_len, d_start or d_end is null or not 4-byte aligned'):
        _backend.dtw_search(4096, 3, ok['item_first'], ok['item_count'], ok['pairs'], 'cosine', True, 4096, 8192, 0,
                            16384)
    # (no pair: nothing to do, whatever the pointers are - and no device is asked for)
    _backend.dtw_search(0, 3, ok['item_first'], ok['item_count'], np.zeros((0, 2)), 'cosine', True, 0, 0, 0, 0)
    _backend.dtw_search(0, 3, ok['item_first'], ok['item_count'], np.zeros((0, 2)), 'cosine', False, 0, 0, 0, 0,
                        curve_first=[], **curves)


# ---- DtwMatches -------------------------------------------------------------------------------------------
def _matches(curves):
    return DtwMatches(query=[0, 1, 0, 0, 1], target=[0, 0, 1, 2, 1], score=[0.5, 0.1, 0.25, 0.25, 0.1],
                      cost=[1.0, 0.2, 0.5, 0.5, 0.3], length=[2, 2, 2, 2, 3], start_frame=[0, 1, 2, 3, 4],
                      end_frame=[1, 2, 3, 4, 6], onset=[0.0, 0.01, 0.02, 0.03, 0.04],
                      offset=[0.035, 0.045, 0.055, 0.065, 0.085], curves=curves)


def test_ranked_and_curve_of_hand_built_matches():
    first = np.array([0, 2, 4, 7, 8, 11])
    cost = np.arange(11, dtype=np.float32)
    length, start = np.arange(11, dtype=np.int32) + 100, np.arange(11, dtype=np.int32) + 200
    found = _matches((first, cost, length, start))
    assert len(found) == 5 and found.score.dtype == np.float32 and found.length.dtype == np.int32
    # by ascending score, equal scores in the order of the pairs
    assert found.ranked(0).tolist() == [2, 3, 0] and found.ranked(1).tolist() == [1, 4]
    assert found.ranked(7).tolist() == []
    got = found.curve(2)
    assert got[0].tolist() == [4, 5, 6] and got[1].tolist() == [104, 105, 106] and got[2].tolist() == [204, 205, 206]
    assert found.curve(3)[0].tolist() == [7] and found.curve(-1)[0].tolist() == [8, 9, 10]
    with pytest.raises(IndexError, match='pair 5 is out of range for 5 pairs'):
        found.curve(5)
    with pytest.raises(ValueError, match='no curves: call dtw_search with return_curves=True'):
        _matches(None).curve(0)
    with pytest.raises(ValueError, match='one length'):
        DtwMatches([0], [0, 1], [0.0], [0.0], [1], [0], [0], [0.0], [0.0])
