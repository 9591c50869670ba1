"""Detections and top-k, the host side: the statement (tests/dtw_detect_f64.py) in its two forms, against the search's
best end, its properties and the counts it gives on the shared cases, a hand-worked top-k; three planted copies;
every argument error of ``dtw_detect``, snf_dtw_detect and snf_dtw_topk (none needs a device); ``DtwDetections``."""

import collections

import numpy as np
import pytest

import dtw_detect_cases
import dtw_detect_f64
import dtw_search_cases
import dtw_search_f64
import test_dtw
from shennong_amd import DtwDetections, dtw_detect
from shennong_amd import dtw as dtw_module


# ---- the statement ----------------------------------------------------------------------------------------
def test_loop_form_equals_array_form_on_integer_distances_full_of_ties():
    rng = np.random.default_rng(21)
    several = tied = 0
    for n, m in ((1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (9, 5), (33, 20), (20, 65), (3, 70), (2, 40), (4, 100),
                 (5, 64)):
        C, L, B = dtw_search_f64.tables(rng.integers(0, 3, size=(n, m)).astype(np.float64))
        for normalized in (True, False):
            for dtype in (np.float64, np.float32):
                for k, max_score in ((1, None), (3, None), (64, None), (64, 0.5), (64, 0.0), (4, -1.0)):
                    loop = dtw_detect_f64.detections_loop(C[-1], L[-1], B[-1], k, normalized, max_score, dtype)
                    fast = dtw_detect_f64.detections(C[-1], L[-1], B[-1], k, normalized, max_score, dtype)
                    assert loop == fast, (n, m, normalized, dtype, k, max_score)
                    assert len(fast) <= min(k, m)
                    if max_score is not None:
                        assert all(found[0] <= max_score for found in fast)
                    several += len(fast) >= 3
                    scores = [found[0] for found in fast]
                    tied += len(set(scores)) < len(scores)
    assert several >= 20 and tied >= 20   # (the data does exercise several rounds and equal scores)


def test_one_detection_is_the_best_end_of_the_search():
    _, _, answers = dtw_search_cases.exact_case(3)
    for answer in answers:
        for normalized in (True, False):
            for dtype in (np.float64, np.float32):
                found = dtw_detect_f64.detections(answer.cost, answer.length, answer.start, 1, normalized, None, dtype)
                assert found == [answer.best(normalized, dtype)]


@pytest.mark.parametrize('dim', dtw_search_cases.EXACT_DIMS)
def test_detections_ascend_are_disjoint_and_the_cases_hold_every_count(dim):
    _, _, answers = dtw_search_cases.exact_case(dim)
    for normalized in (True, False):
        counts = collections.Counter()
        most = 0
        for answer in answers:
            found = dtw_detect_f64.detections(answer.cost, answer.length, answer.start, 64, normalized, None,
                                              np.float32)
            most = max(most, len(found))
            counts[min(len(found), 4)] += 1
            scores = [f[0] for f in found]
            assert scores == sorted(scores)
            taken = np.zeros(answer.shape[1], dtype=int)
            for _, _, _, start, end in found:
                assert 0 <= start <= end < answer.shape[1]
                taken[start:end + 1] += 1
            assert taken.max() == 1   # (pairwise disjoint)
            # k = 4 is the first four of k = 64: the greedy does not look ahead
            assert dtw_detect_f64.detections(answer.cost, answer.length, answer.start, 4, normalized, None,
                                             np.float32) == found[:4]
            # (nothing is left alive when it stops short of k)
            if len(found) < 64:
                dead = np.zeros(answer.shape[1], dtype=bool)
                for _, _, _, start, end in found:
                    dead |= (answer.start <= end) & (np.arange(answer.shape[1]) >= start)
                assert dead.all()
        assert sum(counts.values()) == 100 and all(counts[n] >= 10 for n in (1, 2, 3, 4)), counts
        assert most == 64


def test_top_k_on_a_case_worked_by_hand():
    third = float(np.float32(1.0) / np.float32(3.0))   # 1/3 and its float32 value: one score in float32
    found = [
        [(0.5, 1.0, 2, 0, 1), (0.75, 3.0, 4, 5, 8)],                             # pair 0, query 1
        [(0.25, 1.0, 4, 0, 3), (0.5, 1.0, 2, 7, 8)],                             # pair 1, query 0
        [(0.5, 2.0, 4, 2, 5)],                                                   # pair 2, query 1
        [(0.25, 0.5, 2, 0, 1), (0.25, 0.75, 3, 4, 6), (1.0, 2.0, 2, 8, 9)],      # pair 3, query 0
        [],                                                                      # pair 4, query 2: nothing found
        [(1.0 / 3.0, 1.0, 3, 0, 2)],                                             # pair 5, query 3
        [(third, 1.0, 3, 0, 2)],                                                 # pair 6, query 3
    ]
    query = [1, 0, 1, 0, 2, 3, 3]
    everything = {0: [(1, 0), (3, 0), (3, 1), (1, 1), (3, 2)], 1: [(0, 0), (2, 0), (0, 1)], 2: [],
                  3: [(5, 0), (6, 0)]}
    assert dtw_detect_f64.top_k(found, query, 10) == everything
    assert dtw_detect_f64.top_k(found, query, 2) == {q: rows[:2] for q, rows in everything.items()}
    assert dtw_detect_f64.top_k(found, query, 1) == {0: [(1, 0)], 1: [(0, 0)], 2: [], 3: [(5, 0)]}
    # (in the caller's order: the other way round, pair 5 is still first, its score is equal in float32)
    found[5], found[6] = found[6], found[5]
    assert dtw_detect_f64.top_k(found, query, 1)[3] == [(5, 0)]


# ---- three planted copies -----------------------------------------------------------------------------------
@pytest.mark.parametrize('gaps', dtw_detect_cases.PLANTED_GAPS)
@pytest.mark.parametrize('seed', [1, 2])
def test_three_planted_copies_are_the_three_detections_of_cost_zero(gaps, seed):
    query, target, firsts = dtw_detect_cases.planted_three(gaps, seed)
    n = dtw_detect_cases.PLANTED_FRAMES
    assert target.shape[0] == sum(gaps) + 3 * n
    C, L, B = dtw_search_f64.tables(dtw_search_f64.frame_distances(query, target, 'sqeuclidean'))
    for normalized in (True, False):
        for dtype in (np.float64, np.float32):
            found = dtw_detect_f64.detections(C[-1], L[-1], B[-1], 5, normalized, 0.0, dtype)
            # (a row of 9s is at least 3 * 7^2 away from any row of the query: no other path costs 0)
            assert found == [(0.0, 0.0, n, first, first + n - 1) for first in firsts], (normalized, dtype)
            free = dtw_detect_f64.detections(C[-1], L[-1], B[-1], 5, normalized, None, dtype)
            assert free[:3] == found
            # the fourth and the fifth lie in the 9s and overlap nothing; between copies that are one row apart
            # every other end's path touches a copy, and there is none
            assert len(free) == (3 if max(gaps) == 1 else 5)
            nines = np.ones(target.shape[0], dtype=bool)
            for first in firsts:
                nines[first:first + n] = False
            for k, (score, _, _, start, end) in enumerate(free[3:]):
                assert score > 0 and nines[start:end + 1].all(), (k, start, end)
            if len(free) == 5:
                assert free[3][4] < free[4][3] or free[4][4] < free[3][3]


# ---- argument errors: all before any device work ----------------------------------------------------------
def test_argument_errors_name_the_offender():
    feats = test_dtw._two_layouts()
    with pytest.raises(ValueError, match='invalid metric "kl"'):
        dtw_detect(feats, ['a'], ['b'], metric='kl')
    for bad in (0, 65, -1, 2.0, '4', None, True):
        with pytest.raises(ValueError, match=r'max_detections must be an int in \[1, 64\], not ' + repr(bad)):
            dtw_detect(feats, ['a'], ['b'], max_detections=bad)
    for bad in (0, 1025, -3, 5.0, 'all', False):
        with pytest.raises(ValueError, match=r'top_k must be None or an int in \[1, 1024\], not ' + repr(bad)):
            dtw_detect(feats, ['a'], ['b'], top_k=bad)
    for bad in (float('nan'), np.float32('nan')):
        with pytest.raises(ValueError, match='max_score must be None or a number, not nan'):
            dtw_detect(feats, ['a'], ['b'], max_score=bad)
    with pytest.raises(ValueError, match='top_k=3 with return_curves=True'):
        dtw_detect(feats, ['a'], ['b'], top_k=3, return_curves=True)
    # what dtw_search raises
    with pytest.raises(ValueError, match='query 1: utterance "nope" is not in the collection'):
        dtw_detect(feats, ['a', 'nope'], ['b'])
    with pytest.raises(ValueError, match=r'target 1: not an utterance name or \(name, onset, offset\)'):
        dtw_detect(feats, ['a'], ['b', ('b', 0.5)])
    with pytest.raises(ValueError, match=r'pair 1 \(0, 2\) is out of range for 1 queries and 2 targets'):
        dtw_detect(feats, ['a'], ['b', 'pad'], pairs=np.array([[0, 1], [0, 2]]))
    with pytest.raises(ValueError, match='integer array'):
        dtw_detect(feats, ['a'], ['b'], pairs=np.array([[0.0, 0.0]]))
    with pytest.raises(ValueError, match=r'query 0 \("b", 0.5, 0.6\) has no frames'):
        dtw_detect(feats, [('b', 0.5, 0.6)], ['a'])
    with pytest.raises(ValueError, match=r'items have different ndims: \[3, 5\]'):
        dtw_detect(test_dtw._fake_device_collection([3, 5]), ['utt0'], ['utt1'])
    with pytest.raises(ValueError, match=r'the utterances lie in 2 device blocks \(one per sample rate\)'):
        dtw_detect(test_dtw._fake_device_collection([3, 3]), ['utt0'], ['utt1'], top_k=2)


def test_detect_abi_refuses_bad_arguments_before_any_device_work():
    """snf_dtw_detect returns SNF_E_INVALID (a ValueError here) without asking for a device: this runs anywhere"""
    from shennong_amd import _backend
    ok = dict(dim=3, item_first=[0, 4, 7], item_count=[4, 3, 5], pairs=[[0, 1], [0, 2]], metric='cosine', k=4,
              max_score=None)
    outputs = (4096, 8192, 12288, 16384, 20480)
    curves = dict(d_curve_cost=4096, d_curve_len=8192, d_curve_start=12288)
    cases = [
        (dict(dim=0), {}, 'dtw_detect: dim must be in'),
        (dict(item_count=[4, 0, 5]), {}, 'item 1 has no frames'),
        (dict(item_count=[4, 4097, 5]), {}, 'item 1 has 4097 frames, the limit is 4096'),
        (dict(pairs=[[0, 3]]), {}, r'pair 0 \(0, 3\) is out of range for 3 items'),
        (dict(k=0), {}, r'dtw_detect: max_detections must be in \[1, 64\], not 0'),
        (dict(k=65), {}, r'dtw_detect: max_detections must be in \[1, 64\], not 65'),
        (dict(k=-4), {}, r'max_detections must be in \[1, 64\], not -4'),
        (dict(max_score=float('nan')), {}, 'dtw_detect: max_score is not a number'),
        ({}, dict(curve_first=[0, 3]), 'curve pointers must be all set or all null'),
        ({}, dict(curves, curve_first=[0, 2]), 'the curves of the pairs 0 and 1 overlap'),
        ({}, dict(curves, curve_first=[-1, 3]), r'the curve of pair 0 \(3 elements at -1\) lies outside'),
        ({}, dict(curves, d_curve_cost=4097, curve_first=[0, 3]), 'a curve array is not 4-byte aligned'),
    ]
    for change, keywords, message in cases:
        args = dict(ok)
        args.update(change)
        with pytest.raises(ValueError, match=message):
            _backend.dtw_detect(4096, args['dim'], args['item_first'], args['item_count'], args['pairs'],
                                args['metric'], True, args['k'], args['max_score'], *outputs, **keywords)
    with pytest.raises(ValueError, match='invalid metric'):
        _backend.dtw_detect(4096, 3, ok['item_first'], ok['item_count'], ok['pairs'], 'kl', True, 4, None, *outputs)
    with pytest.raises(ValueError, match='d_count, d_cost, d_len, d_start or d_end is null or not 4-byte aligned'):
        _backend.dtw_detect(4096, 3, ok['item_first'], ok['item_count'], ok['pairs'], 'cosine', True, 4, None, 0, 4096,
                            8192, 12288, 16384)
    with pytest.raises(ValueError, match='d_count, d_cost, d_len, d_start or d_end is null or not 4-byte aligned'):
        _backend.dtw_detect(4096, 3, ok['item_first'], ok['item_count'], ok['pairs'], 'cosine', True, 4, -1.0, 4096,
                            4096, 8194, 12288, 16384)
    # (the arguments are refused for an empty pair table too; a good call without pairs does nothing anywhere)
    with pytest.raises(ValueError, match='max_detections must be in'):
        _backend.dtw_detect(0, 3, ok['item_first'], ok['item_count'], np.zeros((0, 2)), 'cosine', True, 0, None, 0, 0,
                            0, 0, 0)
    _backend.dtw_detect(0, 3, ok['item_first'], ok['item_count'], np.zeros((0, 2)), 'cosine', True, 64, 0.5, 0, 0, 0,
                        0, 0)
    _backend.dtw_detect(0, 3, ok['item_first'], ok['item_count'], np.zeros((0, 2)), 'cosine', False, 1, None, 0, 0, 0,
                        0, 0, curve_first=[], **curves)


def test_topk_abi_refuses_bad_arguments_before_any_device_work():
    """snf_dtw_topk returns SNF_E_INVALID (a ValueError here) without asking for a device: this runs anywhere"""
    from shennong_amd import _backend
    detected = (4096, 8192, 12288, 16384, 20480)
    best = (24576, 28672, 32768, 36864, 40960, 45056, 49152)
    ok = dict(n_pairs=5, k=4, group_pairs=[1, 3, 0, 2, 4], group_first=[0, 2, 2, 5], top_k=3)
    cases = [
        (dict(n_pairs=-1), {}, 'dtw_topk: number of pairs out of range'),
        (dict(k=0), {}, r'dtw_topk: max_detections must be in \[1, 64\], not 0'),
        (dict(k=65), {}, r'max_detections must be in \[1, 64\], not 65'),
        (dict(top_k=0), {}, r'dtw_topk: top_k must be in \[1, 1024\], not 0'),
        (dict(top_k=1025), {}, r'top_k must be in \[1, 1024\], not 1025'),
        (dict(group_first=[1, 2, 2, 5]), {}, 'the first group must start at 0'),
        (dict(group_first=[0, 3, 2, 5]), {}, 'the group of query 1 ends before it starts'),
        (dict(group_pairs=[1, 3, 0, 5, 4]), {}, r'grouped pair 3 \(5\) is out of range for 5 pairs'),
        (dict(group_pairs=[-1, 3, 0, 2, 4]), {}, r'grouped pair 0 \(-1\) is out of range for 5 pairs'),
        ({}, dict(detected=(4096, 8192, 0, 16384, 20480)), 'd_count, d_cost, d_len, d_start or d_end is null'),
        ({}, dict(best=best[:3] + (36865,) + best[4:]), 'an output array is null or not 4-byte aligned'),
        ({}, dict(best=(0,) + best[1:]), 'an output array is null or not 4-byte aligned'),
    ]
    for change, pointers, message in cases:
        args = dict(ok)
        args.update(change)
        with pytest.raises(ValueError, match=message):
            _backend.dtw_topk(*pointers.get('detected', detected), args['n_pairs'], args['k'], True,
                              args['group_pairs'], args['group_first'], args['top_k'], *pointers.get('best', best))
    with pytest.raises(ValueError, match=r'group_first must hold the boundaries of the groups'):
        _backend.dtw_topk(*detected, 5, 4, True, [], [], 3, *best)
    # (no query: nothing to do, whatever the pointers are - and no device is asked for)
    _backend.dtw_topk(0, 0, 0, 0, 0, 0, 4, True, [], [0], 3, 0, 0, 0, 0, 0, 0, 0)


def test_no_pairs_give_empty_columns():
    feats = test_dtw._two_layouts()
    for kwargs in (dict(pairs=np.zeros((0, 2), dtype=np.int64)), dict(pairs=[]), dict(return_curves=True, pairs=[]),
                   dict(pairs=[], top_k=5), dict(pairs=[], max_detections=64, max_score=0.25)):
        found = dtw_detect(feats, ['a'], ['b'], **kwargs)
        assert len(found) == 0
        for name in DtwDetections.columns:
            assert getattr(found, name).shape == (0,), name
        assert found.score.dtype == found.cost.dtype == np.float32 and found.onset.dtype == np.float64
        assert found.pair.dtype == found.rank.dtype == found.end_frame.dtype == np.int32
        assert found.counts.tolist() == ([0] if 'top_k' in kwargs else [])   # (per query; per pair)
        assert found.ranked(0).shape == (0,) and found.of_pair(0).shape == (0,)
    assert len(dtw_detect(feats, [], ['b'])) == 0 and len(dtw_detect(feats, ['a'], [])) == 0


# ---- DtwDetections ----------------------------------------------------------------------------------------
def _detections(curves=None):
    # pairs (query, target): 0 = (0, 0), 1 = (1, 0), 2 = (0, 1); pair 1 has no detection
    return DtwDetections(pair=[0, 0, 2, 2, 2], query=[0, 0, 0, 0, 0], target=[0, 0, 1, 1, 1], rank=[0, 1, 0, 1, 2],
                         score=[0.25, 0.5, 0.25, 0.25, 0.75], cost=[0.5, 1.0, 0.5, 0.75, 3.0], length=[2, 2, 2, 3, 4],
                         start_frame=[0, 4, 1, 3, 7], end_frame=[1, 5, 2, 5, 9],
                         onset=[0.0, 0.04, 0.01, 0.03, 0.07], offset=[0.035, 0.075, 0.045, 0.075, 0.115],
                         counts=[2, 0, 3], curves=curves)


def test_rows_of_hand_built_detections(tmp_path):
    first = np.array([0, 6, 12, 22])
    cost = np.arange(22, dtype=np.float32)
    length, start = np.arange(22, dtype=np.int32) + 100, np.arange(22, dtype=np.int32) + 200
    found = _detections((first, cost, length, start))
    assert len(found) == 5 and found.score.dtype == np.float32 and found.rank.dtype == np.int32
    assert found.columns == ('pair', 'query', 'target', 'rank', 'score', 'cost', 'length', 'start_frame', 'end_frame',
                             'onset', 'offset')
    assert found.of_pair(0).tolist() == [0, 1] and found.of_pair(1).tolist() == [] and \
        found.of_pair(2).tolist() == [2, 3, 4]
    # by (score, pair, rank)
    assert found.ranked(0).tolist() == [0, 2, 3, 1, 4] and found.ranked(1).tolist() == []
    assert [a.tolist() for a in found.curve(1)] == [list(range(6, 12)), list(range(106, 112)), list(range(206, 212))]
    assert found.curve(-1)[0].tolist() == list(range(12, 22))
    with pytest.raises(IndexError, match='pair 3 is out of range for 3 pairs'):
        found.curve(3)
    with pytest.raises(ValueError, match='no curves: call dtw_detect with return_curves=True'):
        _detections().curve(0)
    with pytest.raises(ValueError, match='one-dimensional and of one length'):
        DtwDetections([0], [0, 1], [0], [0], [0.0], [0.0], [1], [0], [0], [0.0], [0.0], counts=[1])
    with pytest.raises(ValueError, match='counts must be one-dimensional and sum to the 5 rows'):
        DtwDetections(*[getattr(found, name) for name in found.columns], counts=[2, 2])
    path = tmp_path / 'found.csv'
    found.save_csv(str(path))
    lines = path.read_text().splitlines()
    assert lines[0] == ','.join(found.columns) and len(lines) == 6
    assert lines[1] == '0,0,0,0,0.25,0.5,2,0,1,0.0,0.035'
    back = np.array([[float(v) for v in line.split(',')] for line in lines[1:]])
    for k, name in enumerate(found.columns):   # (every value comes back as it was)
        assert np.array_equal(back[:, k].astype(getattr(found, name).dtype), getattr(found, name)), name
    # a top-k result keeps its order: rows by query, then by key
    best = DtwDetections(pair=[1, 3, 3, 0], query=[0, 0, 0, 1], target=[1, 0, 0, 0], rank=[0, 0, 1, 0],
                         score=[0.25, 0.25, 0.25, 0.5], cost=[1.0, 0.5, 0.75, 1.0], length=[4, 2, 3, 2],
                         start_frame=[0, 0, 4, 0], end_frame=[3, 1, 6, 1], onset=[0, 0, 0, 0], offset=[1, 1, 1, 1],
                         counts=[3, 1], top_k=3)
    assert best.ranked(0).tolist() == [0, 1, 2] and best.ranked(1).tolist() == [3] and best.top_k == 3
    assert best.of_pair(3).tolist() == [1, 2]


def test_search_returns_what_it_returned_through_the_shared_time_mapping():
    """``_times`` (factored out of ``dtw_search``): the start time of the start row, the stop time of the end row, in
    both layouts of the times and for a target that starts inside its utterance"""
    feats = test_dtw._two_layouts()
    _, _, _, _, where, _, _ = dtw_module._select_search(feats, ['a'], ['b', ('a', 0.0, 10.0), ('b', 5 / 64.0, 1.0)],
                                                        None)
    assert where == [('b', 0), ('a', 0), ('b', 4)]
    onset, offset = dtw_module._times(feats, where, np.array([0, 1, 2, 2]), np.array([1, 2, 0, 3]),
                                      np.array([4, 2, 5, 3]))
    for k, (name, lo, hi) in enumerate((('b', 1, 4), ('a', 2, 2), ('b', 4, 9), ('b', 7, 7))):
        stamps = np.asarray(feats[name].times, dtype=np.float64)
        begin, end = (stamps[:, 0], stamps[:, 1]) if stamps.ndim == 2 else (stamps, stamps)
        assert onset[k] == begin[lo] and offset[k] == end[hi], k
    none = dtw_module._times(feats, where, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32),
                             np.zeros(0, dtype=np.int32))
    assert none[0].shape == none[1].shape == (0,)
