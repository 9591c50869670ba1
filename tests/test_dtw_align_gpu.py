"""Warping paths on the GPU (snf_dtw_align through ``dtw_align`` and the ``return_paths`` of ``dtw_search`` and
``dtw_detect``) against the float64 statement (tests/dtw_align_f64.py): element for element where float32 is exact,
ties included; valid, near-optimal and - where every decision is clear of the rounding - equal on float data; across
strips, tiles and the limits; the paths of search hits and of detections; the scratch runs; batch independence and
the elements that are written; the device route against the host route."""

import numpy as np
import pytest

import dtw_align_cases
import dtw_align_f64
import dtw_cases
import dtw_search_cases
from shennong_amd import Audio, dtw_align, dtw_detect, dtw_distances, dtw_search, synth
from shennong_amd import dtw as dtw_module
from shennong_amd.device import DeviceFeaturesCollection
from shennong_amd.processor import MfccProcessor
from shennong_amd.utterances import Utterances

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a).view(np.uint32)


def _same(a, b):
    """Two DtwPaths hold the same bits"""
    return (np.array_equal(_bits(a.cost), _bits(b.cost)) and np.array_equal(a.length, b.length)
            and np.array_equal(a.first, b.first) and np.array_equal(a.x_frame, b.x_frame)
            and np.array_equal(a.y_frame, b.y_frame))


# ---- 1. exact, ties included --------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', dtw_align_cases.EXACT_DIMS)
def test_integer_sqeuclidean_paths_are_the_statements_ties_included(gpu, dim):
    xs, ys, answers = dtw_align_cases.exact_case(dim)
    feats, pairs = dtw_cases.two_set_collection(xs, ys)
    got = dtw_align(feats, pairs, metric='sqeuclidean', normalized=False)
    cost, length = dtw_distances(feats, pairs, metric='sqeuclidean', normalized=False, return_lengths=True)
    assert got.cost.dtype == np.float32 and got.length.dtype == got.x_frame.dtype == got.y_frame.dtype == np.int32
    assert np.array_equal(_bits(got.cost), _bits(cost)) and np.array_equal(got.length, length)
    assert np.array_equal(np.diff(got.first), length)
    wrong = [k for k, answer in enumerate(answers) if not np.array_equal(got.path(k), answer.path)]
    print('dim', dim, 'cells of the 100 paths:', int(got.first[-1]))
    assert not wrong, wrong[:5]
    assert [answer.cost for answer in answers] == got.cost.tolist()


# ---- 2. strip crossings and limits --------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1000, 900), (4096, 70)])
def test_paths_across_many_strips_and_tiles_and_at_the_limits(gpu, shape):
    """1000 x 900: 16 strips and 29 column tiles; 4096 x 70: 64 strips, turned round the whole seam row - both
    orientations of each, D = 3, every float32 sum exact"""
    x, y, (cost, path), (cost_turned, path_turned) = dtw_align_cases.long_case(shape[0], shape[1], seed=shape[1])
    feats = dtw_cases.collection([x, y])
    got = dtw_align(feats, [('item0', 'item1'), ('item1', 'item0')], metric='sqeuclidean', normalized=False)
    assert got.cost.tolist() == [cost, cost_turned] and got.length.tolist() == [len(path), len(path_turned)]
    assert np.array_equal(got.path(0), path) and np.array_equal(got.path(1), path_turned)


# ---- 3. float data, cosine ----------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', dtw_cases.COSINE_DIMS)
def test_cosine_paths_are_valid_near_optimal_and_equal_where_the_decisions_are_clear(gpu, dim):
    xs, ys, answers = dtw_align_cases.cosine_case(dim)
    feats, pairs = dtw_cases.two_set_collection(xs, ys)
    got = dtw_align(feats, pairs)
    cost, length = dtw_distances(feats, pairs, normalized=False, return_lengths=True)
    assert np.array_equal(_bits(got.cost), _bits(cost)) and np.array_equal(got.length, length)
    decided, worst = 0, 0.0
    for k, answer in enumerate(answers):
        n, m = answer.shape
        path = got.path(k)
        # (a) valid, of the returned length, which is the statement's
        assert dtw_align_f64.is_valid_path(path, n, m, first=(0, 0), last=(n - 1, m - 1)), k
        assert path.shape[0] == got.length[k] == answer.length, k
        # (b) near-optimal: the float64 cost along it is within the bound of the float64 optimum
        bound = dtw_align_cases.path_bound(dim, n, m)
        excess = dtw_align_cases.cost_along(answer.d, path) - answer.cost
        worst = max(worst, excess / bound)
        assert excess <= bound, (k, excess, bound)
        # (c) equal where every decision of the float64 path leads by more than the bound
        if answer.gap > bound:
            decided += 1
            assert np.array_equal(path, answer.path), k
    print('dim', dim, 'pairs whose every decision leads by more than the bound:', decided,
          'of 100; worst excess / bound %.3g' % worst)
    assert decided >= dtw_align_cases.MIN_DECIDED_PAIRS


# ---- 4. subsequence: the paths of search hits ---------------------------------------------------------------
@pytest.mark.parametrize('dim', dtw_align_cases.SEARCH_DIMS)
@pytest.mark.parametrize('normalized', [True, False])
def test_search_paths_are_the_statements_traceback_from_the_searchs_end(gpu, dim, normalized):
    xs, ys, answers = dtw_align_cases.search_case(dim)
    feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
    plain = dtw_search(feats, queries, targets, metric='sqeuclidean', normalized=normalized)
    got = dtw_search(feats, queries, targets, metric='sqeuclidean', normalized=normalized, return_paths=True)
    for name in ('score', 'cost'):
        assert np.array_equal(_bits(getattr(got, name)), _bits(getattr(plain, name))), name
    for name in ('length', 'start_frame', 'end_frame'):
        assert np.array_equal(getattr(got, name), getattr(plain, name)), name
    with pytest.raises(ValueError, match='no paths'):
        plain.path(0)
    for k, answer in enumerate(answers):
        _, cost, length, start, end = answer.best(normalized)
        assert (got.cost[k], got.length[k], got.start_frame[k], got.end_frame[k]) == (cost, length, start, end), k
        path = got.path(k)
        assert np.array_equal(path, answer.path(end)), k
        assert path[0].tolist() == [0, start] and path[-1].tolist() == [answer.shape[0] - 1, end]


def test_the_path_of_a_planted_query_is_the_diagonal_through_its_copy(gpu):
    query, target, answer = dtw_align_cases.planted_case()
    feats = dtw_cases.collection([query, target])
    got = dtw_search(feats, ['item0'], ['item1'], metric='sqeuclidean', return_paths=True)
    assert (got.cost[0], got.length[0], got.start_frame[0], got.end_frame[0]) == (0.0, 37, 70, 106)
    assert np.array_equal(got.path(0), answer.path(106))
    assert got.path(0).tolist() == [[i, 70 + i] for i in range(37)]
    # the centre times of the two frames of every cell (a 25 ms window every 10 ms)
    assert np.allclose(got.times(0), np.stack([0.0125 + 0.01 * np.arange(37), 0.0125 + 0.01 * np.arange(70, 107)], 1),
                       rtol=0, atol=1e-12)


# ---- 5. detections ------------------------------------------------------------------------------------------
def test_every_detection_has_its_path_and_top_k_keeps_those_of_the_survivors(gpu):
    query, planted, answers = dtw_align_cases.detect_case()
    feats = dtw_cases.collection([query] + planted)
    queries, targets = ['item0'], ['item1', 'item2', 'item3']
    plain = dtw_detect(feats, queries, targets, metric='sqeuclidean', max_detections=4)
    got = dtw_detect(feats, queries, targets, metric='sqeuclidean', max_detections=4, return_paths=True)
    for name in got.columns:
        assert np.array_equal(getattr(got, name), getattr(plain, name)), name
    assert np.array_equal(got.counts, plain.counts) and len(got) >= 3
    for p, answer in enumerate(answers):
        found = answer.detections(4)
        rows = got.of_pair(p)
        assert len(rows) == len(found) == got.counts[p]
        taken = []
        for row, (_, cost, length, start, end) in zip(rows, found):
            assert (got.cost[row], got.length[row], got.start_frame[row], got.end_frame[row]) == (cost, length, start,
                                                                                                 end)
            path = got.path(row)
            assert np.array_equal(path, answer.path(end)), (p, row)
            assert sorted(set(path[:, 1].tolist())) == list(range(start, end + 1))
            taken.append(set(path[:, 1].tolist()))
        assert all(not (a & b) for i, a in enumerate(taken) for b in taken[i + 1:])
    # top_k: the first pass as it is, the paths from a second call over the pairs of the survivors
    best = dtw_detect(feats, queries, targets, metric='sqeuclidean', max_detections=4, top_k=2, return_paths=True)
    same = dtw_detect(feats, queries, targets, metric='sqeuclidean', max_detections=4, top_k=2)
    assert len(best) == 2 and np.array_equal(best.pair, same.pair) and np.array_equal(best.rank, same.rank)
    for row in range(len(best)):
        twin = np.flatnonzero((got.pair == best.pair[row]) & (got.rank == best.rank[row]))
        assert twin.shape == (1,)
        assert np.array_equal(best.path(row), got.path(int(twin[0])))
        assert np.array_equal(best.times(row), got.times(int(twin[0])))


# ---- 6. scratch runs ----------------------------------------------------------------------------------------
def test_runs_cut_by_the_scratch_give_the_same_bits(gpu):
    xs, ys, answers = dtw_align_cases.exact_case(3)
    feats, pairs = dtw_cases.two_set_collection(xs, ys)
    resident = DeviceFeaturesCollection.from_host(feats)
    whole = dtw_align(resident, pairs, metric='sqeuclidean', normalized=False)
    shapes = dtw_cases.pair_shapes()
    need = gpu.dtw_record_bytes(shapes[:, 0], shapes[:, 1])
    largest = int(need.max())
    # the largest pair's need: no two pairs fit (the smallest needs 16 bytes, but a run never holds the largest and
    # another; most runs hold one pair)
    one_by_one = dtw_align(resident, pairs, metric='sqeuclidean', normalized=False, scratch_bytes=largest)
    assert _same(one_by_one, whole)
    # the class of M in (32, 512] holds 50 pairs: half of its records cut it in the middle, and the other classes too
    middle = need[(shapes[:, 1] > 32)].sum() // 2
    assert largest < middle < need.sum()
    halves = dtw_align(resident, pairs, metric='sqeuclidean', normalized=False, scratch_bytes=int(middle))
    assert _same(halves, whole)
    assert all(np.array_equal(whole.path(k), answer.path) for k, answer in enumerate(answers))
    resident.release()


# ---- 7. batch independence and written elements -------------------------------------------------------------
def test_a_path_does_not_depend_on_its_batch(gpu):
    xs, ys, _ = dtw_cases.cosine_case(39)
    feats, pairs = dtw_cases.two_set_collection(xs, ys)
    resident = DeviceFeaturesCollection.from_host(feats)
    batch = dtw_align(resident, pairs)
    order = np.random.default_rng(3).permutation(len(pairs))
    shuffled = dtw_align(resident, [pairs[k] for k in order])
    assert np.array_equal(_bits(shuffled.cost), _bits(batch.cost[order]))
    assert all(np.array_equal(shuffled.path(at), batch.path(k)) for at, k in enumerate(order))
    for k in (0, 5, 37, 44, 58, 99):   # 1 x 1, 1 x 63, 32 x 65, 33 x 33, 63 x 129, 200 x 200
        alone = dtw_align(resident, [pairs[k]])
        assert _bits(alone.cost)[0] == _bits(batch.cost)[k] and np.array_equal(alone.path(0), batch.path(k)), k
    resident.release()


def test_the_first_L_elements_of_a_stretch_are_written_and_nothing_else(gpu):
    xs, ys, answers = dtw_align_cases.exact_case(3)
    rows = np.concatenate(xs + ys, axis=0)
    count = np.array([m.shape[0] for m in xs + ys], dtype=np.int32)
    first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    pairs = np.array([(a, len(xs) + b) for a in range(len(xs)) for b in range(len(ys))], dtype=np.int32)
    room = count[pairs[:, 0]].astype(np.int64) + count[pairs[:, 1]] - 1
    # (a gap of 3 elements between the stretches, in an order that is not the pairs')
    order = np.random.default_rng(5).permutation(len(pairs))
    path_first = np.zeros(len(pairs), dtype=np.int64)
    path_first[order] = np.concatenate([[0], np.cumsum(room[order] + 3)[:-1]]) + 2
    total = int((room + 3).sum()) + 2
    d_rows = gpu.DeviceBuffer(rows.nbytes)
    d_rows.upload(rows)
    outputs = []
    for size in (len(pairs), len(pairs), total, total):   # (out of the pool: full of NaN bit patterns)
        gpu.DeviceBuffer(4 * size).free()
        block = gpu.DeviceBuffer(4 * size)
        probe = np.zeros(size, dtype=np.uint32)
        block.download(probe)
        assert (probe == 0xFFFFFFFF).all()
        outputs.append(block)
    d_cost, d_len, d_x, d_y = outputs
    gpu.dtw_align(d_rows.ptr, 3, first, count, pairs, 'sqeuclidean', 'global', d_cost.ptr, d_len.ptr, path_first,
                  d_x.ptr, d_y.ptr)
    cost = d_cost.download(np.zeros(len(pairs), dtype=np.float32))
    length = d_len.download(np.zeros(len(pairs), dtype=np.int32))
    x = d_x.download(np.zeros(total, dtype=np.int32))
    y = d_y.download(np.zeros(total, dtype=np.int32))
    for block in [d_rows] + outputs:
        block.free()
    written = np.zeros(total, dtype=bool)
    for k, answer in enumerate(answers):
        lo = int(path_first[k])
        assert (cost[k], length[k]) == (answer.cost, answer.length)
        assert np.array_equal(x[lo:lo + length[k]], answer.path[:, 0]), k
        assert np.array_equal(y[lo:lo + length[k]], answer.path[:, 1]), k
        written[lo:lo + length[k]] = True
    assert (x[~written] == -1).all() and (y[~written] == -1).all()   # (the poison pattern, untouched)
    assert int(written.sum()) == int(length.sum())


# ---- 8. device route against host route ---------------------------------------------------------------------
def test_device_collection_and_its_host_copy_give_the_same_paths(gpu, audio):
    waves = synth.ragged_utterances(21, 3, min_s=0.4, max_s=0.9)
    audios = [audio] + [Audio(np.ascontiguousarray(w), 16000) for w in waves]
    utts = Utterances([('utt%d' % i, a) for i, a in enumerate(audios)])
    resident = MfccProcessor(dither=0).process_all_device(utts)
    assert isinstance(resident, DeviceFeaturesCollection)
    host = resident.to_host()
    items = [('utt0', 0.0, 0.42), ('utt0', 0.35, 1.2), ('utt0', 0.0, 9.0), ('utt1', 0.1, 0.3),
             ('utt2', 0.0, 0.33), ('utt3', 0.05, 0.4), ('utt1', 0.0, 9.0)]
    pairs = np.array([(a, b) for a in range(len(items)) for b in range(len(items)) if a != b])
    for metric in ('cosine', 'sqeuclidean'):
        on_device = dtw_align(resident, pairs, items=items, metric=metric)
        from_host = dtw_align(host, pairs, items=items, metric=metric)
        assert _same(on_device, from_host)
        cost, length = dtw_distances(resident, pairs, items=items, metric=metric, normalized=False,
                                     return_lengths=True)
        assert np.array_equal(_bits(on_device.cost), _bits(cost)) and np.array_equal(on_device.length, length)
        assert np.array_equal(_bits(on_device.distance), _bits(dtw_distances(resident, pairs, items=items,
                                                                             metric=metric)))
        # the times of a cell are the centre times of its two rows in their utterances
        k = 1   # item 0 against item 2: rows 0 .. of utt0 against the whole of utt0
        a, b = items[pairs[k, 0]], items[pairs[k, 1]]
        centres = dtw_module._centres(host['utt0'].times)
        lo_a = int(np.searchsorted(centres, a[1], side='left'))
        lo_b = int(np.searchsorted(centres, b[1], side='left'))
        path = on_device.path(k)
        assert np.array_equal(on_device.times(k), np.stack([centres[lo_a + path[:, 0]], centres[lo_b + path[:, 1]]],
                                                           axis=1))
        # whole utterances by name
        named = dtw_align(resident, [('utt1', 'utt2'), ('utt2', 'utt1')], metric=metric)
        n, m = host['utt1'].nframes, host['utt2'].nframes
        assert dtw_align_f64.is_valid_path(named.path(0), n, m, first=(0, 0), last=(n - 1, m - 1))
        ranges = named.y_range_of_x(0)
        assert ranges.shape == (n, 2) and ranges[0, 0] == 0 and ranges[-1, 1] == m - 1
        assert (ranges[1:, 0] >= ranges[:-1, 1]).all() and (ranges[1:, 0] <= ranges[:-1, 1] + 1).all()
    resident.release()
