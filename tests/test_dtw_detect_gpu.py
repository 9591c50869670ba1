"""Detections and top-k on the GPU (snf_dtw_detect, snf_dtw_topk, ``dtw_detect``) against the statement
(tests/dtw_detect_f64.py): the count and every slot of every pair, sentinels included, bit for bit where float32 is
exact; under the float metrics bit for bit the statement's greedy on the kernel's own curve, which is the curve of
``dtw_search``; the three kernel classes, kills across the 64-end stride of the lanes, pairs with fewer than K
detections, the threshold at a float32 score and one below it; batch independence; every output element written and
no other; the top-k against the host's stable sort of the same call's detections; the device route against the host
route.  Nothing here has a tolerance: the accuracy of the curve itself is bounded in tests/test_dtw_search_gpu.py."""

import numpy as np
import pytest

import dtw_cases
import dtw_detect_cases
import dtw_detect_f64
import dtw_search_cases
import test_dtw_gpu
from shennong_amd import dtw_detect, dtw_search
from shennong_amd.device import DeviceFeaturesCollection

pytestmark = pytest.mark.gpu

FILL = 0xDEADBEEF   # (not the pool's 0xFFFFFFFF: a sentinel start or end is -1)
GUARD = 64          # words in front of and behind every output array


class _Items:
    """Item matrices as one block of rows on the device, for the calls of the C ABI"""

    def __init__(self, gpu, mats):
        self.gpu = gpu
        self.dim = mats[0].shape[1]
        rows = np.ascontiguousarray(np.concatenate(mats, axis=0), dtype=np.float32)
        self.count = np.array([m.shape[0] for m in mats], dtype=np.int32)
        self.first = np.concatenate([[0], np.cumsum(self.count)[:-1]]).astype(np.int64)
        self.rows = gpu.DeviceBuffer(rows.nbytes)
        self.rows.upload(rows)

    def _filled(self, words):
        block = self.gpu.DeviceBuffer(4 * (words + 2 * GUARD))
        block.upload(np.full(words + 2 * GUARD, FILL, dtype=np.uint32))
        return block

    @staticmethod
    def _inner(block, words, dtype):
        """The `words` elements behind the guard; the guards are untouched and every element is written"""
        got = block.download(np.zeros(words + 2 * GUARD, dtype=np.uint32))
        block.free()
        assert (got[:GUARD] == FILL).all() and (got[GUARD + words:] == FILL).all()
        assert not (got[GUARD:GUARD + words] == FILL).any()
        return got[GUARD:GUARD + words].view(dtype).copy()

    def detect(self, pairs, metric, normalized, k, max_score=None):
        """(count [P], cost, length, start, end [P, k]) as snf_dtw_detect writes them"""
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        n = pairs.shape[0]
        blocks = [self._filled(n)] + [self._filled(n * k) for _ in range(4)]
        self.gpu.dtw_detect(self.rows.ptr, self.dim, self.first, self.count, pairs, metric, normalized, k, max_score,
                            *[b.ptr + 4 * GUARD for b in blocks])
        got = [self._inner(b, n if i == 0 else n * k, np.float32 if i == 1 else np.int32)
               for i, b in enumerate(blocks)]
        return [got[0]] + [a.reshape(n, k) for a in got[1:]]

    def search(self, pairs, metric, normalized):
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        blocks = [self._filled(pairs.shape[0]) for _ in range(4)]
        self.gpu.dtw_search(self.rows.ptr, self.dim, self.first, self.count, pairs, metric, normalized,
                            *[b.ptr + 4 * GUARD for b in blocks])
        return [self._inner(b, pairs.shape[0], np.float32 if i == 0 else np.int32) for i, b in enumerate(blocks)]

    def free(self):
        self.rows.free()


def _assert_slots(got, answers, k, normalized, max_score=None, what=''):
    """count and every slot of every pair, sentinels included, are the statement's (float32 division on its exact
    integers), bit for bit"""
    count, cost, length, start, end = got
    assert count.shape == (len(answers),) and cost.shape == (len(answers), k)
    for p, answer in enumerate(answers):
        assert answer.max_cost < 2 ** 24
        want = dtw_detect_cases.slots(answer, k, normalized, max_score)
        assert count[p] == want[0], (what, p, count[p], want[0])
        assert cost[p].tobytes() == want[1].tobytes(), (what, p, cost[p], want[1])
        assert np.array_equal(length[p], want[2]) and np.array_equal(start[p], want[3]) and \
            np.array_equal(end[p], want[4]), (what, p, length[p], start[p], end[p], want[2:])


def _answers(mats, pairs):
    return [dtw_search_cases.Answer(mats[a], mats[b], 'sqeuclidean', margins=False) for a, b in pairs]


def _integer_rows(rng, n, dim):
    return rng.integers(-2, 3, size=(n, dim)).astype(np.float32)


# ---- 1. exact, every slot -----------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', dtw_search_cases.EXACT_DIMS)
def test_every_slot_of_the_integer_cases_is_the_statement(gpu, dim):
    xs, ys, answers = dtw_search_cases.exact_case(dim)
    assert sorted({m.shape[0] for m in xs}) == sorted({m.shape[0] for m in ys}) == \
        [1, 2, 31, 32, 33, 63, 64, 65, 129, 200]
    items = _Items(gpu, xs + ys)
    pairs = [(a, len(xs) + b) for a in range(len(xs)) for b in range(len(ys))]
    try:
        for normalized in (False, True):
            for k in (1, 4, 64):
                got = items.detect(pairs, 'sqeuclidean', normalized, k)
                _assert_slots(got, answers, k, normalized, what=(normalized, k))
                if k == 1:   # the match of the search
                    found = items.search(pairs, 'sqeuclidean', normalized)
                    assert (got[0] == 1).all()
                    for a, b in zip(got[1:], found):
                        assert a[:, 0].tobytes() == b.tobytes()
    finally:
        items.free()


# ---- 2. the float metrics: the greedy on the kernel's own curve -----------------------------------------------
def _assert_greedy_on_own_curve(found, searched, n_pairs, k, normalized):
    assert found.counts.shape == (n_pairs,) and int(found.counts.sum()) == len(found)
    for p in range(n_pairs):
        curve = found.curve(p)
        assert curve[0].dtype == np.float32 and curve[1].dtype == curve[2].dtype == np.int32
        assert all(u.tobytes() == v.tobytes() for u, v in zip(curve, searched.curve(p))), p
        want = dtw_detect_f64.detections(*curve, k, normalized, None, np.float32)
        rows = found.of_pair(p)
        assert found.counts[p] == len(want) == rows.shape[0], (p, found.counts[p], len(want))
        assert found.rank[rows].tolist() == list(range(len(want)))
        for row, (score, cost, length, start, end) in zip(rows, want):
            got = (int(found.length[row]), int(found.start_frame[row]), int(found.end_frame[row]))
            assert got == (length, start, end), (p, got)
            assert found.cost[row:row + 1].tobytes() == np.float32(cost).tobytes(), p
            assert found.score[row:row + 1].tobytes() == np.float32(score).tobytes(), p


@pytest.mark.parametrize('dim', dtw_search_cases.COSINE_DIMS)
def test_cosine_detections_are_the_greedy_on_the_kernels_own_curve(gpu, dim):
    xs, ys, _ = dtw_cases.cosine_case(dim)
    feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
    resident = DeviceFeaturesCollection.from_host(feats)
    try:
        found = dtw_detect(resident, queries, targets, max_detections=4, return_curves=True)
        searched = dtw_search(resident, queries, targets, return_curves=True)
        _assert_greedy_on_own_curve(found, searched, 100, 4, True)
        assert found.query.tolist() == searched.query[found.pair].tolist()
        assert found.target.tolist() == searched.target[found.pair].tolist()
    finally:
        resident.release()


@pytest.mark.parametrize('kind,dim', dtw_search_cases.SYMKL_CASES)
def test_symkl_detections_are_the_greedy_on_the_kernels_own_curve(gpu, kind, dim):
    import symkl_cases
    xs, ys = symkl_cases.item_sets(kind, dim)
    feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
    resident = DeviceFeaturesCollection.from_host(feats)
    try:
        for normalized in (True, False):
            found = dtw_detect(resident, queries, targets, metric='symkl', normalized=normalized, max_detections=4,
                               return_curves=True)
            searched = dtw_search(resident, queries, targets, metric='symkl', normalized=normalized,
                                  return_curves=True)
            _assert_greedy_on_own_curve(found, searched, 100, 4, normalized)
    finally:
        resident.release()


# ---- 3. classes and seams -----------------------------------------------------------------------------------
@pytest.mark.parametrize('n,m,dim', [(1000, 900, 3), (4096, 70, 257)])
def test_strips_tiles_and_limits(gpu, n, m, dim):
    """1000 x 900 and 900 x 1000 at D = 3: 16 strips, the class of the longest targets; 4096 x 70 and 70 x 4096 at
    D = 257: 64 strips, the whole seam row, 64 ends per lane"""
    rng = np.random.default_rng(n + dim)
    mats = [_integer_rows(rng, n, dim), _integer_rows(rng, m, dim)]
    pairs = [(0, 1), (1, 0)]
    answers = _answers(mats, pairs)
    items = _Items(gpu, mats)
    try:
        for normalized in (False, True):
            _assert_slots(items.detect(pairs, 'sqeuclidean', normalized, 8), answers, 8, normalized)
    finally:
        items.free()


def test_class_boundaries_and_kills_across_the_stride_of_the_lanes(gpu):
    """Targets of 32, 33, 512 and 513 frames (the last and the first of a kernel class), queries of one strip and of
    two; and a target of 600 frames, rows of 9s but for a copy of an 11-frame query at its frames 60 .. 70 and of a
    13-frame query at 508 .. 520: the ends that those detections kill lie on both sides of a multiple of 64, in the
    words of different lanes' turns"""
    rng = np.random.default_rng(64)
    queries = [_integer_rows(rng, n, 3) for n in (5, 70, 11, 13)]
    targets = [_integer_rows(rng, m, 3) for m in (32, 33, 512, 513)]
    planted = np.full((600, 3), 9, dtype=np.float32)
    planted[60:71], planted[508:521] = queries[2], queries[3]
    mats = queries + targets + [planted]
    pairs = [(q, 4 + t) for q in range(4) for t in range(5)]
    answers = _answers(mats, pairs)
    for q, (first, last) in ((2, (60, 70)), (3, (508, 520))):
        answer = answers[pairs.index((q, 8))]
        for normalized in (False, True):
            assert dtw_detect_f64.detections(answer.cost, answer.length, answer.start, 8, normalized, None,
                                             np.float32)[0][1:] == (0.0, last - first + 1, first, last)
        # (the detection kills ends on both sides of a multiple of 64, and beyond the copy)
        dead = (answer.start <= last) & (np.arange(600) >= first)
        assert dead[first:last + 2].all() and first < 64 * ((last + 1) // 64) <= last
    items = _Items(gpu, mats)
    try:
        for normalized in (False, True):
            _assert_slots(items.detect(pairs, 'sqeuclidean', normalized, 8), answers, 8, normalized)
    finally:
        items.free()


# ---- 4. fewer than K ----------------------------------------------------------------------------------------
def test_fewer_detections_than_asked_for(gpu):
    rng = np.random.default_rng(4)
    mats = [_integer_rows(rng, 5, 3), _integer_rows(rng, 1, 3), _integer_rows(rng, 2, 3), _integer_rows(rng, 3, 3),
            np.ones((3, 3), dtype=np.float32), np.full((70, 3), 2, dtype=np.float32)]
    # a target of 1 and of 2 frames; a query longer than its target; a constant query in a constant target
    pairs = [(0, 1), (1, 1), (0, 2), (1, 2), (0, 3), (4, 5)]
    answers = _answers(mats, pairs)
    # every end of the constant pair is tied (d = 3 everywhere): the smallest end wins each round
    tied = answers[-1]
    assert np.unique(tied.cost).size == 1 and np.unique(tied.length).size == 1
    rounds = dtw_detect_f64.detections(tied.cost, tied.length, tied.start, 64, True, None, np.float32)
    assert [found[4] for found in rounds] == sorted(found[4] for found in rounds) and rounds[0][4] == 0
    items = _Items(gpu, mats)
    try:
        for normalized in (False, True):
            for k in (4, 64):
                got = items.detect(pairs, 'sqeuclidean', normalized, k)
                _assert_slots(got, answers, k, normalized, what=(normalized, k))
                assert got[0][0] == 1 and got[0][1] == 1 and (got[0][:5] <= 3).all()
    finally:
        items.free()


# ---- 5. the threshold ---------------------------------------------------------------------------------------
def test_threshold_keeps_an_equal_score_and_drops_the_next_float_below(gpu):
    xs, ys, answers = dtw_search_cases.exact_case(3)
    items = _Items(gpu, xs + ys)
    pairs = [(a, len(xs) + b) for a in range(len(xs)) for b in range(len(ys))]
    try:
        # three pairs whose second detection scores above their first
        free = [dtw_detect_f64.detections(a.cost, a.length, a.start, 4, True, None, np.float32) for a in answers]
        chosen = [p for p in range(100) if len(free[p]) >= 3 and free[p][1][0] > free[p][0][0]][:3]
        assert len(chosen) == 3
        for p in chosen:
            score = np.float32(free[p][1][0])   # a float32 quotient
            assert score.dtype == np.float32 and float(score) == float(free[p][1][0])
            below = np.nextafter(score, np.float32(-np.inf), dtype=np.float32)
            kept = items.detect([pairs[p]], 'sqeuclidean', True, 4, max_score=float(score))
            _assert_slots(kept, [answers[p]], 4, True, float(score))
            dropped = items.detect([pairs[p]], 'sqeuclidean', True, 4, max_score=float(below))
            _assert_slots(dropped, [answers[p]], 4, True, float(below))
            assert kept[0][0] >= 2 and dropped[0][0] == 1, (p, kept[0], dropped[0])
        # one threshold over a whole batch, both rankings; and below every score: nothing but sentinels
        for normalized, max_score in ((True, 2.5), (False, 40.0), (True, 0.0), (False, 0.0)):
            got = items.detect(pairs, 'sqeuclidean', normalized, 4, max_score=max_score)
            _assert_slots(got, answers, 4, normalized, max_score, what=(normalized, max_score))
        nothing = items.detect(pairs, 'sqeuclidean', True, 4, max_score=-1.0)
        _assert_slots(nothing, answers, 4, True, -1.0)
        assert (nothing[0] == 0).all() and np.isinf(nothing[1]).all() and (nothing[2] == 0).all()
        assert (nothing[3] == -1).all() and (nothing[4] == -1).all()
    finally:
        items.free()


@pytest.mark.parametrize('gaps', dtw_detect_cases.PLANTED_GAPS)
def test_three_planted_copies_are_found_and_nothing_else_at_score_zero(gpu, gaps):
    query, target, firsts = dtw_detect_cases.planted_three(gaps, seed=1)
    feats = dtw_cases.collection([query, target])
    n = dtw_detect_cases.PLANTED_FRAMES
    for normalized in (True, False):
        found = dtw_detect(feats, ['item0'], ['item1'], metric='sqeuclidean', normalized=normalized,
                           max_detections=5, max_score=0.0)
        assert found.counts.tolist() == [3] and found.rank.tolist() == [0, 1, 2]
        assert found.start_frame.tolist() == firsts and found.end_frame.tolist() == [f + n - 1 for f in firsts]
        assert found.cost.tolist() == [0.0] * 3 and found.length.tolist() == [n] * 3
        times = np.asarray(feats['item1'].times)
        assert found.onset.tolist() == times[firsts, 0].tolist()
        assert found.offset.tolist() == times[[f + n - 1 for f in firsts], 1].tolist()


# ---- 6. batches, and what is written --------------------------------------------------------------------------
def test_a_pair_does_not_depend_on_its_batch(gpu):
    xs, ys, _ = dtw_search_cases.exact_case(3)
    rng = np.random.default_rng(6)
    mats = xs + ys + [_integer_rows(rng, 600, 3), _integer_rows(rng, 40, 3)]   # (a target of the third class)
    items = _Items(gpu, mats)
    pairs = np.array([(a, len(xs) + b) for a in range(len(xs)) for b in range(len(ys))], dtype=np.int32)
    try:
        batch = items.detect(pairs, 'sqeuclidean', True, 4)
        # shuffled, and beside pairs of the other class
        others = np.array([(21, 20), (3, 20), (9, 20), (20, 21)], dtype=np.int32)
        mixed = np.concatenate([pairs, others])
        order = rng.permutation(len(mixed))
        shuffled = items.detect(mixed[order], 'sqeuclidean', True, 4)
        where = np.argsort(order)[:len(pairs)]   # pair p of the batch is row where[p] of the shuffled call
        for a, b in zip(shuffled, batch):
            assert a[where].tobytes() == b.tobytes()
        for p in (0, 5, 37, 44, 58, 99):   # 1 x 1, 1 x 63, 32 x 65, 33 x 33, 63 x 129, 200 x 200
            alone = items.detect(pairs[p:p + 1], 'sqeuclidean', True, 4)
            for a, b in zip(alone, batch):
                assert a.tobytes() == b[p:p + 1].tobytes(), p
    finally:
        items.free()


def test_every_output_element_is_written_and_no_other(gpu):
    """_Items.detect fills the five arrays and a guard stretch on either side of each with a pattern and asserts that
    the call replaces the pattern in all P (+ P K) elements and nowhere else; here with curves too, laid out with
    gaps in reversed pair order"""
    xs, ys, answers = dtw_search_cases.exact_case(3)
    items = _Items(gpu, xs + ys)
    pairs = np.array([(a, len(xs) + b) for a in range(len(xs)) for b in range(len(ys))], dtype=np.int32)
    columns = items.count[pairs[:, 1]].astype(np.int64)
    curve_first = np.zeros(len(pairs), dtype=np.int64)
    curve_first[::-1] = 5 + np.concatenate([[0], np.cumsum(columns[::-1] + 3)[:-1]])
    total = int(5 + (columns + 3).sum())
    owned = np.zeros(total, dtype=bool)
    for p in range(len(pairs)):
        owned[curve_first[p]:curve_first[p] + columns[p]] = True
    assert owned.sum() == 6200
    k = 3
    try:
        blocks = [items._filled(len(pairs))] + [items._filled(len(pairs) * k) for _ in range(4)]
        curves = [items._filled(total) for _ in range(3)]
        gpu.dtw_detect(items.rows.ptr, 3, items.first, items.count, pairs, 'sqeuclidean', True, k, None,
                       *[b.ptr + 4 * GUARD for b in blocks], curve_first=curve_first,
                       d_curve_cost=curves[0].ptr + 4 * GUARD, d_curve_len=curves[1].ptr + 4 * GUARD,
                       d_curve_start=curves[2].ptr + 4 * GUARD)
        got = [items._inner(b, len(pairs) * (k if i else 1), np.float32 if i == 1 else np.int32)
               for i, b in enumerate(blocks)]
        _assert_slots([got[0]] + [a.reshape(-1, k) for a in got[1:]], answers, k, True)
        for block, want in zip(curves, ('cost', 'length', 'start')):
            words = block.download(np.zeros(total + 2 * GUARD, dtype=np.uint32))
            block.free()
            assert (words[:GUARD] == FILL).all() and (words[GUARD + total:] == FILL).all()
            words = words[GUARD:GUARD + total]
            assert (words[~owned] == FILL).all() and not (words[owned] == FILL).any()
            for p, answer in enumerate(answers):
                stretch = words[int(curve_first[p]):int(curve_first[p] + columns[p])]
                values = stretch.view(np.float32) if want == 'cost' else stretch.view(np.int32)
                assert np.array_equal(values, getattr(answer, want)), (want, p)
    finally:
        items.free()


# ---- 7. top-k -----------------------------------------------------------------------------------------------
def test_top_k_is_the_hosts_stable_sort_of_the_detections(gpu):
    xs, ys, _ = dtw_search_cases.exact_case(3)
    feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
    rng = np.random.default_rng(7)
    # every query against every target and target 5 a second time (equal scores: the pair's index decides), shuffled
    pairs = np.array([(q, t) for q in range(10) for t in list(range(10)) + [5]], dtype=np.int32)
    pairs = pairs[rng.permutation(len(pairs))]
    assert (np.diff(pairs[:, 0]) != 0).sum() > 50   # (the queries are not contiguous)
    resident = DeviceFeaturesCollection.from_host(feats)
    try:
        for normalized in (True, False):
            every = dtw_detect(resident, queries, targets, pairs=pairs, metric='sqeuclidean', normalized=normalized,
                               max_detections=4)
            statement = dtw_detect_f64.top_k(
                [[(every.score[r],) for r in every.of_pair(p)] for p in range(len(pairs))], pairs[:, 0], 1000)
            tied = 0
            for t in (1, 5, 1000):
                best = dtw_detect(resident, queries, targets, pairs=pairs, metric='sqeuclidean',
                                  normalized=normalized, max_detections=4, top_k=t)
                assert best.counts.shape == (10,) and best.top_k == t
                rows = []
                for q in range(10):
                    mine = every.ranked(q)
                    assert [(int(every.pair[r]), int(every.rank[r])) for r in mine] == statement[q]
                    assert best.counts[q] == min(t, len(mine)) and len(mine) < 1000   # (T = 1000: all of them)
                    rows.extend(mine[:t].tolist())
                    scores = every.score[mine[:t]]
                    tied += int((scores[1:] == scores[:-1]).sum())
                assert len(best) == len(rows)
                for name in best.columns:   # every record, in the order of the queries and then of the key
                    assert getattr(best, name).tobytes() == getattr(every, name)[rows].tobytes(), (t, name)
            assert tied >= 10   # (equal scores across pairs: the doubled target alone gives that many)
    finally:
        resident.release()


def test_top_k_writes_every_place_and_sentinels_beyond_the_count(gpu):
    xs, ys, answers = dtw_search_cases.exact_case(3)
    items = _Items(gpu, xs + ys)
    pairs = np.array([(a, len(xs) + b) for a in range(len(xs)) for b in range(len(ys))], dtype=np.int32)
    k, t, n_queries = 4, 50, 12   # (queries 10 and 11 have no pair)
    try:
        arrays = [gpu.DeviceBuffer(4 * len(pairs))] + [gpu.DeviceBuffer(4 * len(pairs) * k) for _ in range(4)]
        gpu.dtw_detect(items.rows.ptr, 3, items.first, items.count, pairs, 'sqeuclidean', True, k, None,
                       *[b.ptr for b in arrays])
        count = arrays[0].download(np.zeros(len(pairs), dtype=np.int32))
        group_first = np.concatenate([np.arange(0, 101, 10), [100, 100]])
        blocks = [items._filled(n_queries)] + [items._filled(n_queries * t) for _ in range(6)]
        gpu.dtw_topk(*[b.ptr for b in arrays], len(pairs), k, True, np.arange(100), group_first, t,
                     *[b.ptr + 4 * GUARD for b in blocks])
        for b in arrays:
            b.free()
        got = [items._inner(b, n_queries * (t if i else 1), np.float32 if i == 3 else np.int32)
               for i, b in enumerate(blocks)]
        top_count, (pair, rank, cost, length, start, end) = got[0], [a.reshape(n_queries, t) for a in got[1:]]
        found = [dtw_detect_f64.detections(a.cost, a.length, a.start, k, True, None, np.float32) for a in answers]
        assert count.tolist() == [len(f) for f in found]
        want = dtw_detect_f64.top_k(found, pairs[:, 0], t)
        for q in range(n_queries):
            mine = want.get(q, [])
            assert top_count[q] == len(mine) < t, q
            n = len(mine)
            assert list(zip(pair[q, :n].tolist(), rank[q, :n].tolist())) == mine, q
            for i, (p, r) in enumerate(mine):
                _, c, le, b, e = found[p][r]
                assert (cost[q, i], length[q, i], start[q, i], end[q, i]) == (c, le, b, e), (q, i)
            assert (pair[q, n:] == -1).all() and (rank[q, n:] == -1).all() and np.isinf(cost[q, n:]).all()
            assert (length[q, n:] == 0).all() and (start[q, n:] == -1).all() and (end[q, n:] == -1).all()
        assert top_count[10] == top_count[11] == 0 and top_count[:10].min() >= 10
    finally:
        items.free()


# ---- 8. routes ----------------------------------------------------------------------------------------------
def test_device_collection_and_its_host_copy_give_the_same_bits(gpu, audio):
    resident = test_dtw_gpu._resident('mfcc', audio)
    assert isinstance(resident, DeviceFeaturesCollection)
    host = resident.to_host()
    queries = [('utt0', 0.40, 0.80), ('utt1', 0.1, 0.3), ('utt2', 0.0, 0.33)]
    targets = ['utt0', 'utt1', ('utt0', 0.35, 1.2), 'utt3']
    try:
        for metric in ('cosine', 'sqeuclidean'):
            for kwargs in (dict(return_curves=True), dict(top_k=5), dict(normalized=False, max_detections=2)):
                on_device = dtw_detect(resident, queries, targets, metric=metric, **kwargs)
                from_host = dtw_detect(host, queries, targets, metric=metric, **kwargs)
                assert len(on_device) == len(from_host) >= 12
                for name in on_device.columns:
                    assert getattr(on_device, name).tobytes() == getattr(from_host, name).tobytes(), name
                assert on_device.counts.tobytes() == from_host.counts.tobytes()
                if 'return_curves' in kwargs:
                    for p in range(12):
                        assert all(u.tobytes() == v.tobytes()
                                   for u, v in zip(on_device.curve(p), from_host.curve(p)))
        # times: the start time of the start row, the stop time of the end row of the target's utterance
        found = dtw_detect(resident, queries, targets)
        times = host['utt0'].times
        for row in found.of_pair(0):
            assert found.onset[row] == times[found.start_frame[row], 0]
            assert found.offset[row] == times[found.end_frame[row], 1]
    finally:
        resident.release()
