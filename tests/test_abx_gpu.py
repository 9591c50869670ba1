"""ABX scores on the GPU: snf_abx_cells alone on synthetic distances against the statement (tests/abx_np.py) -
every count exact, with the cell shapes on every seam of the kernel (one lane per cell, one wave per cell, a cell
split over waves; 64 lanes; the tile of the B-row), non-finite values, counts beyond 2^32, the normalised route -
and ``abx_scores`` end to end against the statement fed with the float64 DTW (exact data) or with the values of
``dtw_distances``; run independence; every output element written."""

import functools
import itertools

import numpy as np
import pytest

import abx_np
import dtw_cases
import dtw_f64
from shennong_amd import abx_scores, dtw_distances
from shennong_amd.abx import AbxItems, build_task
from shennong_amd.device import DeviceFeaturesCollection
from shennong_amd.features import FeaturesCollection

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 129)
WITHIN = dict(on='phone', across=None, by=['talker', 'context'])
ACROSS = dict(on='phone', across='talker', by=['context'])


def _count(gpu, values, records, lengths=None, d_counts=None):
    """The counts [cells, 3] of snf_abx_cells over `values` (and `lengths`) uploaded for the call"""
    held = [gpu.DeviceBuffer(values.nbytes)]
    held[0].upload(values)
    if lengths is not None:
        held.append(gpu.DeviceBuffer(lengths.nbytes))
        held[1].upload(lengths)
    out = d_counts or gpu.DeviceBuffer(24 * len(records))
    try:
        gpu.abx_cells(held[0].ptr, held[1].ptr if lengths is not None else None, values.shape[0], records, out.ptr)
        return out.download(np.zeros((len(records), 3), dtype=np.uint64))
    finally:
        for one in held + ([] if d_counts else [out]):
            one.free()


# ---- 1. the kernel alone --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kernel_case():
    """(values, records, counts of the statement): every shape of SIZES^3 and every same-shape of SIZES^2, each on
    distances of its own with strides larger than the rows and offA != offB, and 20 000 cells of 1 x 1 x 1 on a
    shared pool, all in shuffled order; the distances are small integers, so ties are frequent"""
    rng = np.random.default_rng(11)
    shapes = [(a, b, x, 0) for a, b, x in itertools.product(SIZES, repeat=3)]
    shapes += [(a, b, a, 1) for a, b in itertools.product(SIZES, repeat=2)]
    records, base = [], 0
    for n_a, n_b, n_x, same in shapes:
        stride = n_a + n_b + 7
        records.append([base, base + n_a + 3, stride, n_a, n_b, n_x, same, 0])
        base += n_x * stride
    pool = 4000
    for _ in range(20000):
        off_a, off_b = rng.choice(pool, size=2, replace=False) + base
        records.append([off_a, off_b, int(rng.integers(0, 5)), 1, 1, 1, 0, 0])
    values = rng.integers(0, 6, size=base + pool).astype(np.float32)
    records = np.array(records, dtype=np.int64)[rng.permutation(len(records))]
    want = np.array([abx_np.cell_counts(values, record) for record in records], dtype=np.uint64)
    return values, records, want


def test_counts_are_exact_on_every_cell_shape_in_one_shuffled_call(gpu):
    values, records, want = kernel_case()
    # (the statement's two counting routines agree where the loop is affordable)
    for record in records[(records[:, 3] * records[:, 4] * records[:, 5] <= 130)][:300]:
        assert abx_np.cell_counts(values, record) == abx_np.cell_counts_loop(values, record)
    n = records[:, 3] * records[:, 4] * (records[:, 5] - records[:, 6])
    assert (want[:, 1] > 0).sum() > len(records) // 8 and (want[:, 2] == 0).all()
    assert (want[:, 0].astype(np.int64) + want[:, 1].astype(np.int64) <= n).all()
    got = _count(gpu, values, records)
    wrong = np.flatnonzero((got != want).any(axis=1))
    assert wrong.size == 0, (records[wrong[:3]], got[wrong[:3]], want[wrong[:3]])


# ---- 2. bad triplets ------------------------------------------------------------------------------------------
def test_non_finite_distances_are_counted_as_bad_and_touch_nothing_else(gpu):
    rng = np.random.default_rng(12)
    shapes = [(1, 1, 1, 0), (2, 3, 2, 1), (3, 4, 5, 0), (65, 129, 3, 0), (64, 70, 64, 1), (129, 1100, 2, 0),
              (70, 5, 9, 0)]
    records, base = [], 0
    for n_a, n_b, n_x, same in shapes:
        stride = n_a + n_b + 5
        records.append([base, base + n_a + 2, stride, n_a, n_b, n_x, same, 0])
        base += n_x * stride
    records = np.array(records, dtype=np.int64)
    values = rng.integers(0, 6, size=base).astype(np.float32)
    clean = _count(gpu, values, records)
    assert np.array_equal(clean, np.array([abx_np.cell_counts(values, r) for r in records], dtype=np.uint64))
    assert (clean[:, 2] == 0).all()
    planted = values.copy()
    for record in records[:-1]:   # NaN, +inf and -inf in the A and in the B stretch of every cell but the last
        off_a, off_b, stride, n_a, n_b, n_x = record[:6].tolist()
        for x in range(n_x):
            planted[off_a + x * stride + rng.integers(0, n_a)] = [np.nan, np.inf, -np.inf][x % 3]
            planted[off_b + x * stride + rng.integers(0, n_b, size=2)] = [np.inf, np.nan, -np.inf][x % 3]
    want = np.array([abx_np.cell_counts(planted, r) for r in records], dtype=np.uint64)
    for record, counts in zip(records[:5], want[:5]):
        assert abx_np.cell_counts_loop(planted, record) == tuple(counts.tolist())
    assert (want[:-1, 2] > 0).all()
    got = _count(gpu, planted, records)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(got[-1], clean[-1])   # the cell that the planted values do not touch


# ---- 3. counts beyond 2^32, a cell split over waves ------------------------------------------------------------
def test_a_cell_of_more_than_2_32_triplets(gpu):
    n_a = n_b = 2048
    n_x = 1100
    stride = n_a + n_b + 8
    rng = np.random.default_rng(13)
    # distances in {0 .. 7}: the A-stretches draw from {0, 1, 2} and the B-stretches from {2 .. 7}, so that `less`
    # itself (17 / 18 of the triplets), not only n, lies above 2^32
    values = rng.integers(0, 8, size=(n_x, stride)).astype(np.float32)
    values[:, 4:4 + n_a] = rng.integers(0, 3, size=(n_x, n_a))
    values[:, n_a + 8:n_a + 8 + n_b] = rng.integers(2, 8, size=(n_x, n_b))
    values = values.reshape(-1)
    record = np.array([[4, n_a + 8, stride, n_a, n_b, n_x, 0, 0]], dtype=np.int64)
    want = abx_np.cell_counts(values, record[0])
    n = n_a * n_b * n_x
    assert n > 2 ** 32 and want[0] > 2 ** 32 and want[1] > 0 and want[2] == 0
    got = _count(gpu, values, record)[0].tolist()
    assert got[0] + got[1] <= n
    assert tuple(got) == want


# ---- 4. the normalised route ----------------------------------------------------------------------------------
def test_the_quotient_compared_is_float32_cost_over_length(gpu):
    """Integer items: the costs are integers and the path lengths differ, so the quotients tie and nearly tie"""
    xs, ys = dtw_cases.item_sets('int', 3, seed=21)
    mats = [m for m in xs + ys if m.shape[0] <= 65]
    feats = dtw_cases.collection(mats)
    m = len(mats)
    labels = {'phone': np.array(['p%d' % (k % 3) for k in range(m)])}
    task = build_task(labels, 'phone')
    (blocks,) = task.runs(1 << 20)
    pairs, records, cells = task.tables(blocks)
    names = [('item%d' % a, 'item%d' % b) for a, b in pairs.tolist()]
    cost, length = dtw_distances(feats, names, metric='sqeuclidean', normalized=False, return_lengths=True)
    quotient = cost / length.astype(np.float32)
    assert quotient.dtype == np.float32 and np.unique(length).size > 10
    want = np.array([abx_np.cell_counts_loop(quotient, r) for r in records], dtype=np.uint64)
    want_raw = np.array([abx_np.cell_counts_loop(cost, r) for r in records], dtype=np.uint64)
    assert not np.array_equal(want, want_raw) and want[:, 1].sum() > 0
    assert np.array_equal(_count(gpu, cost, records, lengths=length), want)
    assert np.array_equal(_count(gpu, cost, records), want_raw)


# ---- 5. and 6. end to end -------------------------------------------------------------------------------------
LENGTHS = (1, 31, 32, 33, 64, 65)


@functools.lru_cache(maxsize=None)
def corpus(kind):
    """36 items, two per (phone, talker, context) of 3 x 3 x 2, two items per utterance, selected by time:
    (host collection, AbxItems, the matrices of the items)"""
    rng = np.random.default_rng(31)
    combos = list(itertools.product(range(3), range(3), range(2))) * 2
    combos = [combos[k] for k in rng.permutation(len(combos))]
    lengths = [LENGTHS[k % len(LENGTHS)] for k in rng.permutation(len(combos))]
    if kind == 'int':
        make = lambda n: rng.integers(-2, 3, size=(n, 1)).astype(np.float32)   # noqa: E731  (D = 1: ties)
    else:
        make = lambda n: rng.standard_normal((n, 13)).astype(np.float32)      # noqa: E731
    mats = [make(n) for n in lengths]
    centre = lambda k: 0.01 * k + 0.0125   # noqa: E731  (dtw_cases.features: a 25 ms window every 10 ms)
    utts, names, onsets, offsets = [], [], [], []
    for u in range(len(mats) // 2):
        first, second = mats[2 * u], mats[2 * u + 1]
        utts.append(('utt%d' % u, dtw_cases.features(np.concatenate([first, second], axis=0))))
        names += ['utt%d' % u] * 2
        onsets += [0.0, centre(first.shape[0]) - 0.001]
        offsets += [centre(first.shape[0] - 1) + 0.001, 1e9]
    labels = {'phone': np.array(['p%d' % c[0] for c in combos]), 'talker': np.array(['t%d' % c[1] for c in combos]),
              'context': np.array(['c%d' % c[2] for c in combos])}
    return FeaturesCollection(utts), AbxItems(names, onsets, offsets, labels), mats


def _assert_table_equals_rows(table, rows, kind):
    assert len(table) == len(rows) > 0
    names = kind['by'] + ['phone_1', 'phone_2'] + (['talker_1', 'talker_2'] if kind['across'] else [])
    for k, (key, score, n, less, equal, bad) in enumerate(rows):
        assert bad == 0
        assert tuple(table[name][k] for name in names) == key, k
        assert (table['n'][k], table['less'][k], table['equal'][k]) == (n, less, equal), key
        assert table['score'][k].tobytes() == np.float64(score).tobytes(), key


@functools.lru_cache(maxsize=None)
def exact_distance():
    _, _, mats = corpus('int')

    @functools.lru_cache(maxsize=None)
    def distance(y, x):
        return dtw_f64.dtw(mats[y], mats[x], 'sqeuclidean', normalized=False)[0]
    return distance


@pytest.mark.parametrize('kind', [WITHIN, ACROSS], ids=['within', 'across'])
def test_end_to_end_on_exact_data_equals_the_statement_on_the_float64_dtw(gpu, kind):
    feats, items, mats = corpus('int')
    rows = abx_np.table_rows(items.labels, kind['on'], kind['across'], kind['by'], exact_distance())
    table = abx_scores(feats, items, metric='sqeuclidean', normalized=False, **kind)
    print('triplets', sum(row[2] for row in rows), 'of them tied', sum(row[4] for row in rows))
    _assert_table_equals_rows(table, rows, kind)


@pytest.mark.parametrize('kind', [WITHIN, ACROSS], ids=['within', 'across'])
def test_end_to_end_cosine_equals_the_statement_on_the_values_of_dtw_distances(gpu, kind):
    feats, items, mats = corpus('normal')
    n = len(items)
    triples = list(zip(items.names, items.onsets.tolist(), items.offsets.tolist()))
    pairs = np.array([(y, x) for y in range(n) for x in range(n)])
    dense = dtw_distances(feats, pairs, items=triples).reshape(n, n)
    rows = abx_np.table_rows(items.labels, kind['on'], kind['across'], kind['by'], lambda y, x: dense[y, x])
    table = abx_scores(feats, items, **kind)
    _assert_table_equals_rows(table, rows, kind)
    resident = DeviceFeaturesCollection.from_host(feats)
    try:
        again = abx_scores(resident, items, **kind)
    finally:
        resident.release()
    assert list(again.columns) == list(table.columns)
    for name in table.columns:
        assert np.array_equal(again[name], table[name]), name


# ---- 7. run independence --------------------------------------------------------------------------------------
def test_the_table_does_not_depend_on_the_runs(gpu):
    feats, items, _ = corpus('normal')
    task = build_task(items.labels, **WITHIN)
    need = int(task.block_size.max()) ** 2
    assert len(task.runs(2 * need)) >= 3 and len(task.runs(1 << 26)) == 1
    whole = abx_scores(feats, items, **WITHIN)
    for max_pairs in (2 * need, need):
        parts = abx_scores(feats, items, max_pairs=max_pairs, **WITHIN)
        for name in whole.columns:
            assert np.array_equal(parts[name], whole[name]), name
        assert parts['score'].tobytes() == whole['score'].tobytes()
    with pytest.raises(ValueError, match='needs {} pairs, max_pairs is {}'.format(need, need - 1)):
        abx_scores(feats, items, max_pairs=need - 1, **WITHIN)


# ---- 8. poisoned buffers --------------------------------------------------------------------------------------
def test_every_count_is_written_and_a_second_call_gives_the_same(gpu):
    values, records, want = kernel_case()
    gpu.DeviceBuffer(24 * len(records)).free()
    d_counts = gpu.DeviceBuffer(24 * len(records))   # (out of the pool: full of 0xFF, the `gpu` fixture)
    probe = d_counts.download(np.zeros((len(records), 3), dtype=np.uint64))
    assert (probe == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    try:
        first = _count(gpu, values, records, d_counts=d_counts)
        second = _count(gpu, values, records, d_counts=d_counts)
    finally:
        d_counts.free()
    assert np.array_equal(first, want) and np.array_equal(second, want)
    # ... and without a split cell in the call (no zeroing pass): the plain stores reach every element too
    few = records[records[:, 3] * records[:, 4] * records[:, 5] <= 4096]
    gpu.DeviceBuffer(24 * len(few)).free()
    d_counts = gpu.DeviceBuffer(24 * len(few))
    try:
        got = _count(gpu, values, few, d_counts=d_counts)
    finally:
        d_counts.free()
    assert np.array_equal(got, want[records[:, 3] * records[:, 4] * records[:, 5] <= 4096])
