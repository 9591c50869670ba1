"""The warping paths without a GPU: the float64 statement (tests/dtw_align_f64.py) against itself and against the
statements underneath, the properties of its paths, the argument checks of snf_dtw_align (which precede any device
work) and of ``dtw_align``, and the host logic of ``DtwPaths`` and of the paths of ``DtwMatches`` and
``DtwDetections`` on hand-made arrays."""

import numpy as np
import pytest

import dtw_align_cases
import dtw_align_f64
import dtw_cases
import dtw_f64
import dtw_search_f64
import test_dtw
from shennong_amd import DtwPaths, dtw_align, dtw_detect, dtw_search
from shennong_amd import dtw as dtw_module
from shennong_amd.dtw import DtwDetections, DtwMatches


# ---- the statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1), (2, 2), (17, 23), (40, 7)])
def test_loop_form_equals_diagonal_form_and_the_statements_underneath(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for d in (rng.integers(0, 3, size=shape).astype(np.float64), rng.random(shape)):   # (full of ties; none)
        made, loop = dtw_align_f64.global_tables(d), dtw_align_f64.global_tables_loop(d)
        for a, b in zip(made, loop):
            assert np.array_equal(a, b)
        for a, b in zip(made[:2], dtw_f64.tables(d)):
            assert np.array_equal(a, b)
        made, loop = dtw_align_f64.sub_tables(d), dtw_align_f64.sub_tables_loop(d)
        for a, b in zip(made, loop):
            assert np.array_equal(a, b)
        for a, b in zip(made[:3], dtw_search_f64.tables(d)):
            assert np.array_equal(a, b)
        # the origins, and nothing else, hold a 3
        assert (made[3][0] == 3).all() and (made[3][1:] != 3).all()
        K = dtw_align_f64.global_tables(d)[2]
        assert K[0, 0] == 3 and (K == 3).sum() == 1


def test_ties_go_to_the_first_of_the_order():
    K = dtw_align_f64.global_tables(np.zeros((3, 3)))[2]
    assert K.tolist() == [[3, 2, 2], [1, 0, 0], [1, 0, 0]]   # (all equal: the diagonal where it exists)
    assert dtw_align_f64.traceback(K).tolist() == [[0, 0], [1, 1], [2, 2]]
    K = dtw_align_f64.sub_tables(np.zeros((2, 3)))[3]
    assert K.tolist() == [[3, 3, 3], [1, 0, 0]]
    assert dtw_align_f64.traceback(K, 0).tolist() == [[0, 0], [1, 0]]
    assert dtw_align_f64.traceback(K, 2).tolist() == [[0, 1], [1, 2]]


@pytest.mark.parametrize('dim', dtw_align_cases.EXACT_DIMS)
def test_paths_are_monotone_of_length_L_and_sum_to_C_on_integer_data(dim):
    xs, ys, answers = dtw_align_cases.exact_case(dim)
    _, _, (cost, length, _, _) = dtw_cases.exact_case(dim)
    for k, answer in enumerate(answers):
        n, m = answer.shape
        assert dtw_align_f64.is_valid_path(answer.path, n, m, first=(0, 0), last=(n - 1, m - 1)), k
        assert answer.path.dtype == np.int32 and answer.path.shape == (answer.length, 2)
        assert (answer.cost, answer.length) == (cost[k], length[k])
        assert dtw_align_cases.cost_along(answer.d, answer.path) == answer.cost   # (integers: exact)


@pytest.mark.parametrize('dim', dtw_align_cases.SEARCH_DIMS)
def test_subsequence_paths_start_at_B_end_at_the_end_and_have_L_cells(dim):
    xs, ys, answers = dtw_align_cases.search_case(dim)
    for k, answer in enumerate(answers):
        n, m = answer.shape
        for end in sorted({0, m // 2, m - 1, answer.best(True)[4], answer.best(False)[4]}):
            path = answer.path(end)
            assert dtw_align_f64.is_valid_path(path, n, m, first=(0, answer.start[end]), last=(n - 1, end)), (k, end)
            assert path.shape[0] == answer.length[end]
            d = dtw_align_f64.frame_distances(xs[k // len(ys)], ys[k % len(ys)], 'sqeuclidean')
            assert dtw_align_cases.cost_along(d, path) == answer.cost[end]


def test_the_detections_of_the_planted_copies_cover_them():
    for answer in dtw_align_cases.detect_case()[2]:
        found = answer.detections(4)
        assert len(found) >= 3
        taken = []
        for _, cost, length, start, end in found:
            path = answer.path(end)
            assert path.shape[0] == length and path[0].tolist() == [0, start]
            assert sorted(set(path[:, 1].tolist())) == list(range(start, end + 1))
            taken.append(set(range(start, end + 1)))
        assert all(not (a & b) for i, a in enumerate(taken) for b in taken[i + 1:])


def test_the_gap_of_a_path_is_the_smallest_lead_of_its_decisions():
    d = np.array([[0.0, 5.0, 9.0], [4.0, 1.0, 3.0], [9.0, 2.5, 1.0]])
    C, L, K = dtw_align_f64.global_tables(d)
    assert dtw_align_f64.traceback(K).tolist() == [[0, 0], [1, 1], [2, 2]]
    # at (2, 2): C[1, 1] = 1 leads C[1, 2] = 4 and C[2, 1] = 3.5; at (1, 1): C[0, 0] = 0 leads 5 and 4
    assert dtw_align_f64.path_gap(C, K) == 2.5
    assert dtw_align_f64.path_gap(*dtw_align_f64.global_tables(np.zeros((2, 2)))[::2]) == 0.0


# ---- the C ABI: every refusal comes before any device work ---------------------------------------------------
def test_align_abi_refuses_bad_arguments_before_any_device_work():
    """snf_dtw_align returns SNF_E_INVALID (a ValueError here) without asking for a device: this runs anywhere"""
    from shennong_amd import _backend
    ok = dict(dim=3, item_first=[0, 4, 7], item_count=[4, 3, 5], pairs=[[0, 1], [0, 2]], metric='cosine',
              mode='global', d_cost=4096, d_len=8192, path_first=[0, 6], d_path_x=12288, d_path_y=16384)
    detect = dict(mode='subsequence', max_detections=2, d_count=20480, d_start=24576, d_end=28672,
                  path_first=[0, 6, 12, 20])
    cases = [
        (dict(dim=0), 'dtw_align: dim must be in'),
        (dict(item_count=[4, 0, 5]), 'item 1 has no frames'),
        (dict(item_count=[4, 4097, 5]), 'item 1 has 4097 frames, the limit is 4096'),
        (dict(pairs=[[0, 3]], path_first=[0]), r'pair 0 \(0, 3\) is out of range for 3 items'),
        (dict(d_cost=0), 'dtw_align: d_cost or d_len is null or not 4-byte aligned'),
        (dict(d_len=8193), 'd_cost or d_len is null or not 4-byte aligned'),
        (dict(d_path_x=0), 'dtw_align: d_path_x or d_path_y is null or not 4-byte aligned'),
        (dict(d_path_y=16386), 'd_path_x or d_path_y is null or not 4-byte aligned'),
        (dict(path_first=[0, 5]), 'the paths of pair 0, slot 0 and pair 1, slot 0 overlap'),
        (dict(path_first=[8, 0]), None),                                     # (any order will do)
        (dict(path_first=[7, 0]), 'the paths of pair 0, slot 0 and pair 1, slot 0 overlap'),
        (dict(path_first=[-1, 6]), r'the path of pair 0, slot 0 \(6 elements at -1\) lies outside'),
        (dict(path_first=[0, 2 ** 31 - 7]), r'the path of pair 1, slot 0 \(8 elements at 2147483641\) lies outside'),
        (dict(path_first=[0, 2 ** 31 - 8]), None),
        (dict(scratch_bytes=-1), 'dtw_align: scratch_bytes is negative'),
        # 4 x 5: one strip of 4 + 5 - 1 steps, 16 bytes each
        (dict(scratch_bytes=127), 'scratch_bytes 127 is below the 128 bytes of records of the largest pair'),
        (dict(scratch_bytes=128), None),
        (dict(detect, normalized=2), None),                                  # (the wrapper makes it a bool)
        (dict(detect, max_detections=0, path_first=[]), r'dtw_align: max_detections must be in \[1, 64\], not 0'),
        (dict(detect, max_detections=65, path_first=[0] * 130), r'max_detections must be in \[1, 64\], not 65'),
        (dict(detect, max_score=float('nan')), 'dtw_align: max_score is not a number'),
        (dict(detect, d_count=0), 'dtw_align: d_count, d_start or d_end is null or not 4-byte aligned'),
        (dict(detect, d_end=28673), 'd_count, d_start or d_end is null or not 4-byte aligned'),
        (dict(detect, path_first=[0, 6, 12, 19]), 'the paths of pair 1, slot 0 and pair 1, slot 1 overlap'),
        (dict(detect), None),
    ]
    for change, message in cases:
        args = dict(ok)
        args.update(change)
        call = lambda: _backend.dtw_align(4096, args.pop('dim'), args.pop('item_first'), args.pop('item_count'),  # noqa
                                          args.pop('pairs'), args.pop('metric'), args.pop('mode'), args.pop('d_cost'),
                                          args.pop('d_len'), args.pop('path_first'), args.pop('d_path_x'),
                                          args.pop('d_path_y'), **args)
        if message is None:
            # every check has passed: the next thing the call does is ask for a device (on a machine with one it would
            # go on to launch kernels on pointers that are no memory, so it is made only where there is none)
            if _backend.device_count() < 1:
                with pytest.raises(Exception) as caught:
                    call()
                assert not isinstance(caught.value, ValueError), caught.value
            continue
        with pytest.raises(ValueError, match=message):
            call()
    with pytest.raises(ValueError, match='invalid metric'):
        _backend.dtw_align(4096, 3, [0, 4], [4, 3], [[0, 1]], 'kl', 'global', 4096, 8192, [0], 4096, 8192)
    with pytest.raises(ValueError, match='invalid mode "local"'):
        _backend.dtw_align(4096, 3, [0, 4], [4, 3], [[0, 1]], 'cosine', 'local', 4096, 8192, [0], 4096, 8192)
    with pytest.raises(ValueError, match='path_first has 1 entries for 1 pairs of 2 slots'):
        _backend.dtw_align(4096, 3, [0, 4], [4, 3], [[0, 1]], 'cosine', 'subsequence', 4096, 8192, [0], 4096, 8192,
                           max_detections=2)
    # an unknown mode, straight at the C ABI
    import ctypes as C
    first, count = np.array([0, 4], dtype=np.int64), np.array([4, 3], dtype=np.int32)
    pairs, path_first = np.array([[0, 1]], dtype=np.int32), np.zeros(1, dtype=np.int64)
    rc = _backend.lib().snf_dtw_align(0, C.c_void_p(4096), 3, first.ctypes.data_as(C.POINTER(C.c_int64)),
                                      count.ctypes.data_as(C.POINTER(C.c_int32)), 2,
                                      pairs.ctypes.data_as(C.POINTER(C.c_int32)), 1, 0, 2, 1, 1, 0.0, None,
                                      C.c_void_p(4096), C.c_void_p(8192), None, None,
                                      path_first.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(4096),
                                      C.c_void_p(8192), 0, None)
    with pytest.raises(ValueError, match=r'dtw_align: mode must be 0 \(global\) or 1 \(subsequence\), not 2'):
        _backend.check(rc)
    # (the arguments are refused for an empty pair table too; a good call without pairs does nothing anywhere)
    with pytest.raises(ValueError, match='max_detections must be in'):
        _backend.dtw_align(0, 3, [0, 4], [4, 3], np.zeros((0, 2)), 'cosine', 'subsequence', 0, 0, [], 0, 0,
                           max_detections=0)
    _backend.dtw_align(0, 3, [0, 4], [4, 3], np.zeros((0, 2)), 'cosine', 'global', 0, 0, [], 0, 0)
    _backend.dtw_align(0, 3, [0, 4], [4, 3], np.zeros((0, 2)), 'symkl', 'subsequence', 0, 0, [], 0, 0,
                       max_detections=64, max_score=0.5)


def test_record_bytes_of_the_two_sizes_that_the_documents_quote():
    from shennong_amd import _backend
    assert _backend.dtw_record_bytes(298, 298) == 16 * (298 + 5 * 297) == 28528         # "29 KB"
    assert _backend.dtw_record_bytes(4096, 4096) == 16 * (4096 + 64 * 4095) == 4258816   # "4.3 MB"
    assert _backend.dtw_record_bytes(np.array([1, 64, 65]), np.array([1, 1, 2])).tolist() == [16, 1024, 16 * 67]


# ---- dtw_align: the checks of dtw_distances, before any device work ------------------------------------------
def test_argument_errors_name_the_offender():
    feats = test_dtw._two_layouts()
    with pytest.raises(ValueError, match='invalid metric "kl"'):
        dtw_align(feats, [('a', 'b')], metric='kl')
    with pytest.raises(ValueError, match='utterance "nope" is not in the collection'):
        dtw_align(feats, [('a', 'nope')])
    with pytest.raises(ValueError, match='item 1: utterance "nope" is not in the collection'):
        dtw_align(feats, np.array([[0, 1]]), items=[('a', 0, 1), ('nope', 0, 1)])
    with pytest.raises(ValueError, match=r'pair 1 \(0, 2\) is out of range for 2 items'):
        dtw_align(feats, np.array([[0, 1], [0, 2]]), items=[('a', 0, 1), ('b', 0, 1)])
    with pytest.raises(ValueError, match='pairs must be pairs of utterance names'):
        dtw_align(feats, [('a', 'b', 'pad')])
    with pytest.raises(ValueError, match=r'item 0 \("b", 0.5, 0.6\) has no frames'):
        dtw_align(feats, np.array([[0, 1]]), items=[('b', 0.5, 0.6), ('a', 0, 1)])
    with pytest.raises(ValueError, match=r'items have different ndims: \[3, 5\]'):
        dtw_align(test_dtw._fake_device_collection([3, 5]), [('utt0', 'utt1')])
    with pytest.raises(ValueError, match=r'the utterances lie in 2 device blocks \(one per sample rate\)'):
        dtw_align(test_dtw._fake_device_collection([3, 3]), [('utt0', 'utt1')])
    for bad in (-1, 2.5, '1G', None, True):
        with pytest.raises(ValueError, match='scratch_bytes must be a non-negative int, not ' + repr(bad)):
            dtw_align(feats, [('a', 'b')], scratch_bytes=bad)
    # 20 x 20: one strip of 39 steps
    with pytest.raises(ValueError, match='scratch_bytes 623 is below the 624 bytes that the largest pair needs'):
        dtw_align(feats, [('pad', 'a'), ('a', 'b')], scratch_bytes=623)


def test_no_pairs_give_empty_paths():
    feats = test_dtw._two_layouts()
    for pairs, items in (([], None), (np.zeros((0, 2), dtype=np.int64), [('a', 0, 1)])):
        paths = dtw_align(feats, pairs, items=items)
        assert len(paths) == 0 and paths.first.tolist() == [0]
        assert paths.cost.shape == paths.length.shape == paths.distance.shape == paths.x_frame.shape == (0,)
        assert paths.cost.dtype == np.float32 and paths.x_frame.dtype == paths.y_frame.dtype == np.int32
    for found in (dtw_search(feats, ['a'], ['b'], pairs=[], return_paths=True),
                  dtw_detect(feats, ['a'], ['b'], pairs=[], return_paths=True),
                  dtw_detect(feats, ['a'], ['b'], pairs=[], return_paths=True, top_k=3)):
        assert len(found) == 0
        with pytest.raises(IndexError):
            found.path(0)


# ---- DtwPaths on hand-made arrays ----------------------------------------------------------------------------
def _paths(**kwargs):
    # pair 0: 3 x 4 frames, pair 1: 2 x 1
    x = [0, 0, 1, 2, 2, 0, 1]
    y = [0, 1, 2, 2, 3, 0, 0]
    centres = [np.array([0.5, 1.5, 2.5]), np.array([10.0, 11.0, 12.0, 13.0]), np.array([7.0])]
    return DtwPaths([2.5, 1.0], [5, 2], [0, 5, 7], x, y, centres=centres, pairs=[[0, 1], [0, 2]], **kwargs)


def test_paths_of_hand_built_arrays(tmp_path):
    paths = _paths()
    assert len(paths) == 2 and paths.distance.tolist() == [0.5, 0.5] and paths.distance.dtype == np.float32
    assert _paths(normalized=False).distance.tolist() == [2.5, 1.0]
    assert paths.path(0).tolist() == [[0, 0], [0, 1], [1, 2], [2, 2], [2, 3]] and paths.path(0).dtype == np.int32
    assert paths.path(1).tolist() == paths.path(-1).tolist() == [[0, 0], [1, 0]]
    assert paths.y_range_of_x(0).tolist() == [[0, 1], [2, 2], [2, 3]] and paths.y_range_of_x(0).dtype == np.int32
    assert paths.y_range_of_x(1).tolist() == [[0, 0], [0, 0]]
    assert paths.times(0).tolist() == [[0.5, 10.0], [0.5, 11.0], [1.5, 12.0], [2.5, 12.0], [2.5, 13.0]]
    assert paths.times(1).tolist() == [[0.5, 7.0], [1.5, 7.0]] and paths.times(1).dtype == np.float64
    for bad in (2, -3):
        with pytest.raises(IndexError, match='pair {} is out of range for 2'.format(bad)):
            paths.path(bad)
    where = tmp_path / 'paths.csv'
    paths.save_csv(str(where))
    assert where.read_text().splitlines() == ['pair,x_frame,y_frame', '0,0,0', '0,0,1', '0,1,2', '0,2,2', '0,2,3',
                                              '1,0,0', '1,1,0']
    with pytest.raises(ValueError, match='no times'):
        DtwPaths([1.0], [1], [0, 1], [0], [0]).times(0)
    with pytest.raises(ValueError, match=r'first must count length\[p\] cells'):
        DtwPaths([1.0, 2.0], [1, 2], [0, 2, 3], [0, 0, 1], [0, 0, 0])
    with pytest.raises(ValueError, match='must hold the 3 frames that first counts'):
        DtwPaths([1.0], [3], [0, 3], [0, 0], [0, 0])
    with pytest.raises(ValueError, match='first must hold ascending offsets'):
        DtwPaths([1.0], [3], [1, 4], [0, 0, 0], [0, 0, 0])


def test_times_follow_the_rule_of_the_item_selection():
    """The centre of a [n, 2] (start, stop) row is its mean, that of a [n] row its value: layouts 'a' and 'b' of
    tests/test_dtw.py have the same centres"""
    feats = test_dtw._two_layouts()
    centre = lambda k: (k + 1) / 64.0   # noqa: E731
    for name in ('a', 'b'):
        got = dtw_module._item_centres(feats, [name, name], [0, 4], [20, 3])
        assert got[0].tolist() == [centre(k) for k in range(20)]
        assert got[1].tolist() == [centre(4), centre(5), centre(6)]


def test_matches_and_detections_give_their_paths_only_when_asked():
    columns = dict(query=[0, 1], target=[0, 0], score=[0.5, 0.25], cost=[1.0, 0.5], length=[2, 2],
                   start_frame=[3, 0], end_frame=[4, 0], onset=[0.0, 0.0], offset=[1.0, 1.0])
    with pytest.raises(ValueError, match='no paths: call dtw_search with return_paths=True'):
        DtwMatches(**columns).path(0)
    with pytest.raises(ValueError, match='no paths: call dtw_search with return_paths=True'):
        DtwMatches(**columns).times(0)
    centres = [np.array([0.0, 1.0]), np.array([5.0, 6.0]), np.arange(20.0, 30.0)]
    store = dtw_module._PathStore([0, 2, 4], [0, 1, 0, 1], [3, 4, 0, 0], centres, [0, 1], [2, 2])
    found = DtwMatches(paths=store, **columns)
    assert found.path(0).tolist() == [[0, 3], [1, 4]] and found.path(1).tolist() == [[0, 0], [1, 0]]
    assert found.times(0).tolist() == [[0.0, 23.0], [1.0, 24.0]] and found.times(1).tolist() == [[5.0, 20.0], [6.0, 20.0]]
    rows = dict(columns, pair=[0, 1], rank=[0, 0], counts=[1, 1])
    with pytest.raises(ValueError, match='no paths: call dtw_detect with return_paths=True'):
        DtwDetections(**rows).path(0)
    hits = DtwDetections(paths=store, **rows)
    assert hits.path(1).tolist() == [[0, 0], [1, 0]] and hits.times(0).tolist() == [[0.0, 23.0], [1.0, 24.0]]
    with pytest.raises(IndexError, match='row 2 is out of range for 2'):
        hits.path(2)
    # (_compact: the first length[s] elements of every stretch, one behind the other)
    first, x, y = dtw_module._compact([4, 0], [2, 3], np.arange(10, 20), np.arange(20, 30))
    assert first.tolist() == [0, 2, 5] and x.tolist() == [14, 15, 10, 11, 12] and y.tolist() == [24, 25, 20, 21, 22]
