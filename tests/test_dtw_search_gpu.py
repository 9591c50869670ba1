"""Subsequence DTW search on the GPU (snf_dtw_search through ``dtw_search``) against the float64 statement
(tests/dtw_search_f64.py): bit for bit where float32 is exact, ties included, at every end of every pair; within the
derived bounds of tests/dtw_cases.py and tests/symkl_cases.py elsewhere, lengths and starts wherever the statement's
margin decides them; the item lengths sit on every seam of the kernel (tile of 32 columns, strip of 64 rows, ring of
3 tiles, the three kernel classes); the returned best against the kernel's own curve; the device route against the
host route; batch independence; every output element written and no other.  Every threshold comes from the
statement and the derived bounds.  Measured worst errors per D: profiles/dtw_search_errors.txt
(tools/dtw_search_errors.py)."""

import numpy as np
import pytest

import dtw_cases
import dtw_search_cases
import dtw_search_f64
import test_dtw_gpu
from shennong_amd import dtw as dtw_module
from shennong_amd import dtw_search
from shennong_amd.device import DeviceFeaturesCollection

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a).view(np.uint32)


def _assert_self_consistent(found, normalized):
    """4. The returned best of every pair is bit for bit the first arg-min of the float32 quotient over the
    kernel's own curve"""
    for p in range(len(found)):
        cost, length, start = found.curve(p)
        assert cost.dtype == np.float32 and length.dtype == start.dtype == np.int32
        score = cost / length.astype(np.float32) if normalized else cost
        end = int(np.argmin(score))
        got = (int(found.end_frame[p]), int(found.start_frame[p]), int(found.length[p]))
        assert got == (end, int(start[end]), int(length[end])), (p, got)
        assert _bits(found.cost)[p] == _bits(cost)[end] and _bits(found.score)[p] == _bits(score)[end], p


def _assert_exact(found, answers, normalized):
    """Every end of every curve and the best of every pair equal the statement, whose costs are float32 integers"""
    for p, answer in enumerate(answers):
        assert answer.max_cost < 2 ** 24
        cost, length, start = found.curve(p)
        assert np.array_equal(_bits(cost), _bits(answer.cost.astype(np.float32))), p
        assert np.array_equal(length, answer.length) and np.array_equal(start, answer.start), p
        score, best_cost, best_length, best_start, best_end = answer.best(normalized, np.float32)
        got = (int(found.end_frame[p]), int(found.start_frame[p]), int(found.length[p]), float(found.cost[p]))
        assert got == (best_end, best_start, best_length, best_cost), (p, got)
        assert _bits(found.score)[p] == _bits(np.float32(score)), p


# ---- 1. exact, ties included --------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', dtw_search_cases.EXACT_DIMS)
def test_integer_sqeuclidean_is_exact_at_every_end_ties_included(gpu, dim):
    xs, ys, answers = dtw_search_cases.exact_case(dim)
    feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
    resident = DeviceFeaturesCollection.from_host(feats)
    try:
        for normalized in (False, True):
            found = dtw_search(resident, queries, targets, metric='sqeuclidean', normalized=normalized,
                               return_curves=True)
            assert found.query.tolist() == [q for q in range(10) for _ in range(10)]
            assert found.target.tolist() == list(range(10)) * 10
            _assert_exact(found, answers, normalized)
            _assert_self_consistent(found, normalized)
    finally:
        resident.release()


# ---- 2. strips, tiles, limits -------------------------------------------------------------------------------
@pytest.mark.parametrize('n,m,dim', [(1000, 900, 3), (4096, 70, 257)])
def test_strips_tiles_and_limits_are_exact(gpu, n, m, dim):
    """1000 x 900 at D = 3: 16 strips, 29 column tiles, the class of the longest targets, and the other order.
    4096 x 70 and 70 x 4096 at D = 257 (an odd D): 64 strips; 128 tiles and the whole seam row."""
    rng = np.random.default_rng(n + dim)
    x = rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
    y = rng.integers(-2, 3, size=(m, dim)).astype(np.float32)
    answers = [dtw_search_cases.Answer(x, y, 'sqeuclidean', margins=False),
               dtw_search_cases.Answer(y, x, 'sqeuclidean', margins=False)]
    feats = dtw_cases.collection([x, y])
    resident = DeviceFeaturesCollection.from_host(feats)
    try:
        for normalized in (False, True):
            found = dtw_search(resident, ['item0', 'item1'], ['item0', 'item1'], pairs=np.array([[0, 1], [1, 0]]),
                               metric='sqeuclidean', normalized=normalized, return_curves=True)
            _assert_exact(found, answers, normalized)
            _assert_self_consistent(found, normalized)
            bare = dtw_search(resident, ['item0', 'item1'], ['item0', 'item1'], pairs=np.array([[0, 1], [1, 0]]),
                              metric='sqeuclidean', normalized=normalized)
            for name in found.columns:   # (the same without curves)
                assert getattr(bare, name).tobytes() == getattr(found, name).tobytes(), name
    finally:
        resident.release()


# ---- 3. cosine at every seam --------------------------------------------------------------------------------
def _assert_within(found, answers, bound_of, qualifies, normalized, min_share, what):
    """`bound_of(answer)`: the bound of the score of every end [M]; `qualifies(answer, bound)`: the ends [M] whose
    L and B the statement's margin decides.  The conditions on the statement come first."""
    bounds = [np.broadcast_to(bound_of(a), a.cost.shape) for a in answers]
    masks = [qualifies(a, b) for a, b in zip(answers, bounds)]
    ends = sum(m.size for m in masks)
    share = sum(int(m.sum()) for m in masks) / ends
    truth = [dtw_search_f64.scores(a.cost, a.length, normalized) for a in answers]
    decided = []
    for a, b, s in zip(answers, bounds, truth):
        ranked = np.sort(s)
        decided.append(s.size >= 2 and ranked[1] - ranked[0] >= 2 * b.max())
    many = [k for k, a in enumerate(answers) if a.shape[1] >= 2]
    print(what, 'ends', ends, 'qualifying share %.4f' % share, 'decided pairs', sum(decided), 'of', len(many))
    assert ends == 6200 and len(many) == 90
    assert share >= min_share and sum(decided) >= dtw_search_cases.MIN_DECIDED_PAIRS
    worst = worst_ratio = 0.0
    for p, (a, b, mask, s) in enumerate(zip(answers, bounds, masks, truth)):
        cost, length, start = found.curve(p)
        got = cost.astype(np.float64) / length if normalized else cost.astype(np.float64)
        error = np.abs(got - s)
        worst, worst_ratio = max(worst, error.max()), max(worst_ratio, (error / b).max())
        assert (error <= b).all(), (p, np.flatnonzero(error > b)[:5], error.max())
        assert np.array_equal(length[mask], a.length[mask]), (p, np.flatnonzero(mask & (length != a.length))[:5])
        assert np.array_equal(start[mask], a.start[mask]), (p, np.flatnonzero(mask & (start != a.start))[:5])
        # the best end: the minimum of perturbed values moves by at most the perturbation
        want = a.best(normalized)
        assert abs(float(found.score[p]) - want[0]) <= b.max(), p
        if decided[p] or a.shape[1] == 1:
            got_best = (int(found.length[p]), int(found.start_frame[p]), int(found.end_frame[p]))
            assert got_best == want[2:], (p, got_best, want)
    print(what, 'worst error %.3g, worst error / bound %.3g' % (worst, worst_ratio))


@pytest.mark.parametrize('dim', dtw_search_cases.COSINE_DIMS)
def test_cosine_within_the_derived_bound_at_every_end_of_every_seam(gpu, dim):
    xs, ys, answers = dtw_search_cases.cosine_case(dim)
    assert max(a.max_cos for a in answers) <= dtw_cases.MAX_COS
    feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
    found = dtw_search(feats, queries, targets, return_curves=True)
    _assert_within(found, answers, lambda a: dtw_cases.cosine_bound(dim, *a.shape),
                   lambda a, b: a.margin >= dtw_cases.MIN_MARGIN, True, dtw_search_cases.MIN_QUALIFYING_ENDS,
                   'cosine dim %d:' % dim)
    _assert_self_consistent(found, True)


# ---- 5. symkl -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,dim', dtw_search_cases.SYMKL_CASES)
def test_symkl_within_the_derived_bound_at_every_end_of_every_seam(gpu, kind, dim):
    """The bound of tests/symkl_cases.py holds for the cost of every end; an end qualifies, as a pair does there, when
    its margin is at least twice its bound.  The bound grows with N + M and with D, so fewer ends qualify than under
    cosine: the statement alone gives 95.2 % (plain, 7) and 89.2 % (floored, 64) of the 6200 ends, and the share
    asserted before looking at the device is 85 %.  Costs are compared unnormalised, as the bound is stated."""
    xs, ys, answers = dtw_search_cases.symkl_case(kind, dim)
    feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
    found = dtw_search(feats, queries, targets, metric='symkl', normalized=False, return_curves=True)
    _assert_within(found, answers, lambda a: dtw_search_cases.symkl_bound(a, dim), lambda a, b: a.margin >= 2 * b,
                   False, 0.85, 'symkl %s dim %d:' % (kind, dim))
    _assert_self_consistent(found, False)
    normalised = dtw_search(feats, queries, targets, metric='symkl', return_curves=True)
    _assert_self_consistent(normalised, True)
    for p in (0, 37, 99):   # (the curves do not depend on the ranking)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(normalised.curve(p), found.curve(p)))


# ---- 6. routes and batches ----------------------------------------------------------------------------------
def _assert_same(a, b, order=None):
    for name in a.columns[2:]:
        want = getattr(b, name) if order is None else getattr(b, name)[order]
        assert getattr(a, name).tobytes() == want.tobytes(), name


@pytest.mark.parametrize('kind', ['mfcc', 'mfcc+delta'])
def test_device_collection_and_its_host_copy_give_the_same_bits(gpu, audio, kind):
    resident = test_dtw_gpu._resident(kind, audio)
    assert isinstance(resident, DeviceFeaturesCollection)
    host = resident.to_host()
    dim = host['utt0'].ndims
    assert dim == (13 if kind == 'mfcc' else 39)
    queries = [('utt0', 0.40, 0.80), ('utt1', 0.1, 0.3), ('utt2', 0.0, 0.33)]
    targets = ['utt0', 'utt1', ('utt0', 0.35, 1.2), 'utt3']
    for metric in ('cosine', 'sqeuclidean'):
        for normalized in (True, False):
            on_device = dtw_search(resident, queries, targets, metric=metric, normalized=normalized,
                                   return_curves=True)
            from_host = dtw_search(host, queries, targets, metric=metric, normalized=normalized, return_curves=True)
            assert len(on_device) == 12
            _assert_same(on_device, from_host)
            for p in range(12):
                assert all(u.tobytes() == v.tobytes() for u, v in zip(on_device.curve(p), from_host.curve(p)))
            _assert_self_consistent(on_device, normalized)
    # the item ('utt0', 0.40, 0.80) in the whole of utt0: its own first and last row wherever the statement says so
    found = dtw_search(resident, queries, targets)
    first, count, _, n_queries, where, _, _ = dtw_module._select_search(host, queries, targets, None)
    assert where[0] == ('utt0', 0) and count[n_queries] == host['utt0'].nframes
    lo, n = int(first[0] - first[n_queries]), int(count[0])
    rows = host['utt0'].data
    want = dtw_search_f64.search(rows[lo:lo + n], rows, 'cosine')
    print(kind, 'statement', want, 'device', found.score[0], found.length[0], found.start_frame[0], found.end_frame[0])
    assert 30 <= n <= 50 and lo > 0
    if want[3:] == (lo, lo + n - 1):
        assert (int(found.start_frame[0]), int(found.end_frame[0])) == (lo, lo + n - 1)
    # (the slope of arccos at 1, as in test_dtw_gpu.py: a cosine of 1 - (dim + 4) 2^-24)
    assert 0 <= found.score[0] <= np.sqrt((dim + 4) * 2.0 ** -22) / np.pi
    # times: the start time of the start row, the stop time of the end row of the target utterance
    times = host['utt0'].times
    assert found.onset[0] == times[found.start_frame[0], 0] and found.offset[0] == times[found.end_frame[0], 1]
    lo2 = int(first[n_queries + 2] - first[n_queries])   # (target 2 starts inside utt0)
    assert lo2 > 0 and found.onset[2] == times[lo2 + found.start_frame[2], 0]
    assert found.offset[2] == times[lo2 + found.end_frame[2], 1]
    resident.release()


def test_a_pair_does_not_depend_on_its_batch(gpu):
    xs, ys, _ = dtw_search_cases.cosine_case(39)
    feats, queries, targets = dtw_search_cases.names_and_pairs(xs, ys)
    resident = DeviceFeaturesCollection.from_host(feats)
    try:
        batch = dtw_search(resident, queries, targets, return_curves=True)
        pairs = np.stack([batch.query, batch.target], axis=1)
        order = np.random.default_rng(3).permutation(len(pairs))
        shuffled = dtw_search(resident, queries, targets, pairs=pairs[order], return_curves=True)
        assert np.array_equal(shuffled.query, batch.query[order])
        assert np.array_equal(shuffled.target, batch.target[order])
        _assert_same(shuffled, batch, order)
        for k, p in enumerate(order.tolist()):
            assert all(u.tobytes() == v.tobytes() for u, v in zip(shuffled.curve(k), batch.curve(p)))
        for p in (0, 5, 37, 44, 58, 99):   # 1 x 1, 1 x 63, 32 x 65, 33 x 33, 63 x 129, 200 x 200
            alone = dtw_search(resident, queries, targets, pairs=pairs[p:p + 1], return_curves=True)
            _assert_same(alone, batch, [p])
            assert all(u.tobytes() == v.tobytes() for u, v in zip(alone.curve(0), batch.curve(p)))
    finally:
        resident.release()


# ---- 7. poisoned buffers ------------------------------------------------------------------------------------
def test_every_output_element_is_written_and_no_other(gpu):
    xs, ys, answers = dtw_search_cases.exact_case(3)
    rows = np.concatenate(xs + ys, axis=0)
    count = np.array([m.shape[0] for m in xs + ys], dtype=np.int32)
    first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    pairs = np.array([(a, len(xs) + b) for a in range(len(xs)) for b in range(len(ys))], dtype=np.int32)
    # the curve of pair p: 5 unused words, then every stretch with 3 unused words behind it, in reversed pair order
    columns = count[pairs[:, 1]].astype(np.int64)
    curve_first = np.zeros(len(pairs), dtype=np.int64)
    curve_first[::-1] = 5 + np.concatenate([[0], np.cumsum(columns[::-1] + 3)[:-1]])
    total = int(5 + (columns + 3).sum())
    owned = np.zeros(total, dtype=bool)
    for p in range(len(pairs)):
        owned[curve_first[p]:curve_first[p] + columns[p]] = True
    assert owned.sum() == columns.sum() == 6200
    d_rows = gpu.DeviceBuffer(rows.nbytes)
    d_rows.upload(rows)

    def poisoned(words):   # (out of the pool: full of NaN bit patterns, the `gpu` fixture)
        gpu.DeviceBuffer(4 * words).free()
        block = gpu.DeviceBuffer(4 * words)
        probe = np.zeros(words, dtype=np.uint32)
        block.download(probe)
        assert (probe == 0xFFFFFFFF).all()
        return block
    results = [poisoned(len(pairs)) for _ in range(4)]
    curves = [poisoned(total) for _ in range(3)]
    gpu.dtw_search(d_rows.ptr, 3, first, count, pairs, 'sqeuclidean', True, *[b.ptr for b in results],
                   curve_first=curve_first, d_curve_cost=curves[0].ptr, d_curve_len=curves[1].ptr,
                   d_curve_start=curves[2].ptr)
    got = [b.download(np.zeros(len(pairs), dtype=np.uint32)) for b in results]
    got_curves = [b.download(np.zeros(total, dtype=np.uint32)) for b in curves]
    for block in [d_rows] + results + curves:
        block.free()
    for column in got:
        assert not (column == 0xFFFFFFFF).any()
    for column in got_curves:
        assert (column[~owned] == 0xFFFFFFFF).all() and not (column[owned] == 0xFFFFFFFF).any()
    for p, answer in enumerate(answers):
        stretch = slice(int(curve_first[p]), int(curve_first[p] + columns[p]))
        assert np.array_equal(got_curves[0][stretch].view(np.float32), answer.cost.astype(np.float32)), p
        assert np.array_equal(got_curves[1][stretch].view(np.int32), answer.length), p
        assert np.array_equal(got_curves[2][stretch].view(np.int32), answer.start), p
        _, best_cost, best_length, best_start, best_end = answer.best(True, np.float32)
        assert (got[0].view(np.float32)[p], got[1].view(np.int32)[p], got[2].view(np.int32)[p],
                got[3].view(np.int32)[p]) == (best_cost, best_length, best_start, best_end), p
