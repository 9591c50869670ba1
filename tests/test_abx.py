"""ABX scores, the host side: the task construction of ``shennong_amd.abx`` against the statement
(tests/abx_np.py), triplet by triplet; ``.item`` files; the collapse; every argument error (none needs a device);
snf_abx_cells' refusals, which come before any device is asked for."""

import os
import re

import numpy as np
import pytest

import abx_np
import dtw_cases
from conftest import ROOT
from shennong_amd import FeaturesCollection, _backend, abx_scores
from shennong_amd import abx as abx_module
from shennong_amd.abx import AbxItems, AbxTable, build_task

WITHIN = dict(on='phone', across=None, by=['talker', 'context'])
ACROSS = dict(on='phone', across='talker', by=['context'])
PLAIN = dict(on='phone', across=None, by=[])
PLAIN_ACROSS = dict(on='phone', across='talker', by=[])


def _labels(seed, n, phones=3, talkers=3, contexts=2):
    rng = np.random.default_rng(seed)
    return {'phone': np.array(['p%d' % k for k in rng.integers(0, phones, n)]),
            'talker': np.array(['t%d' % k for k in rng.integers(0, talkers, n)]),
            'context': np.array(['c%d' % k for k in rng.integers(0, contexts, n)])}


def _key_of(task, c):
    key = tuple(task.values[column][code] for column, code in zip(task.by, task.block_codes[task.cell_block[c]]))
    key += (task.values[task.on][task.on_1[c]], task.values[task.on][task.on_2[c]])
    if task.across is not None:
        key += (task.values[task.across][task.ac_1[c]], task.values[task.across][task.ac_2[c]])
    return key


# ---- task construction --------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [WITHIN, ACROSS, PLAIN, PLAIN_ACROSS], ids=['within', 'across', 'plain', 'plain-across'])
@pytest.mark.parametrize('seed,n', [(0, 1), (1, 7), (2, 16), (3, 24)])
def test_records_and_pairs_address_exactly_the_statements_triplets(kind, seed, n):
    labels = _labels(seed, n)
    want = abx_np.triplets(labels, kind['on'], kind['across'], kind['by'])
    task = build_task(labels, **kind)
    keys = [_key_of(task, c) for c in range(task.n.shape[0])]
    assert keys == sorted(want)   # the cells that have a triplet, in the documented order, each once
    for max_pairs in (1 << 26, max(int(task.block_size.max()) ** 2, 1)):   # one run, and as many as can be
        got = {}
        for blocks in task.runs(max_pairs):
            pairs, records, cells = task.tables(blocks)
            assert pairs.dtype == np.int32 and records.dtype == np.int64 and records.shape[1] == 8
            assert pairs.shape[0] == int((task.block_size[blocks] ** 2).sum()) <= max_pairs
            # (X-major, the Y of a fixed X contiguous: the X column is constant over every stretch of a block's size)
            for triples, c in zip(abx_np.expand(pairs, records), cells.tolist()):
                assert keys[c] not in got
                got[keys[c]] = triples
                assert len(triples) == task.n[c]
        assert sorted(got) == sorted(want)
        for key in want:
            assert len(set(got[key])) == len(got[key]), key   # each triplet once
            assert set(got[key]) == set(want[key]), key


def test_a_block_with_one_item_one_phone_or_one_talker_gives_no_cell():
    one_item = {'phone': ['a'], 'talker': ['t'], 'context': ['c']}
    one_phone = {'phone': ['a'] * 5, 'talker': ['t', 'u', 'v', 't', 'u'], 'context': ['c'] * 5}
    one_talker = {'phone': ['a', 'b', 'a', 'b', 'c'], 'talker': ['t'] * 5, 'context': ['c'] * 5}
    for labels in (one_item, one_phone):
        for kind in (WITHIN, ACROSS, PLAIN, PLAIN_ACROSS):
            task = build_task(labels, **kind)
            assert task.n.shape[0] == 0 and task.runs(1) == []
    assert build_task(one_talker, **ACROSS).n.shape[0] == 0
    assert build_task(one_talker, **PLAIN_ACROSS).n.shape[0] == 0
    # (with one talker the within task has cells: (a, b), (a, c), (b, a), (b, c) - c has one item, so no (c, .))
    within = build_task(one_talker, **WITHIN)
    assert [(within.on_1[c], within.on_2[c]) for c in range(4)] == [(0, 1), (0, 2), (1, 0), (1, 2)]
    assert within.n.tolist() == [4, 2, 4, 2]


def test_runs_are_whole_blocks_and_a_block_beyond_max_pairs_is_refused():
    labels = _labels(5, 40)
    task = build_task(labels, **ACROSS)
    sizes = task.block_size
    runs = task.runs(int(sizes.max()) ** 2)
    assert len(runs) == 2 and sorted(np.concatenate(runs).tolist()) == [0, 1]
    assert len(task.runs(int((sizes ** 2).sum()))) == 1
    big = int(np.argmax(sizes))
    with pytest.raises(ValueError, match=r'by-block \(context=c%d\) has %d items and needs %d pairs' % (
            big, sizes[big], sizes[big] ** 2)):
        task.runs(int(sizes.max()) ** 2 - 1)


# ---- item files ---------------------------------------------------------------------------------------------
def _items(n=6):
    labels = _labels(4, n)
    onsets = 0.125 * np.arange(n) + 1 / 3.0
    return AbxItems(['utt%d' % (k % 3) for k in range(n)], onsets, onsets + 0.1, labels)


def test_item_file_round_trips(tmp_path):
    items = _items()
    path = str(tmp_path / 'corpus.item')
    items.save(path)
    assert open(path).readline() == '#file onset offset #phone talker context\n'
    back = AbxItems.load(path)
    assert back.names == items.names and list(back.labels) == list(items.labels)
    assert np.array_equal(back.onsets, items.onsets) and np.array_equal(back.offsets, items.offsets)
    for column in items.labels:
        assert back.labels[column].tolist() == items.labels[column].tolist()


@pytest.mark.parametrize('text,message', [
    ('', 'missing header'),
    ('utt0 0.1 0.2 a t c\n', 'malformed header'),
    ('#file onset offset phone talker\nutt0 0.1 0.2 a t\n', 'malformed header'),
    ('#file offset onset #phone talker\nutt0 0.1 0.2 a t\n', 'malformed header'),
    ('#file onset offset #phone talker\nutt0 0.1 0.2 a\n', 'line 2 has 4 fields, the header names 5'),
    ('#file onset offset #phone talker\nutt0 0.1 0.2 a t\nutt1 0.1 x a t\n', 'line 3: non-numeric time'),
    ('#file onset offset #phone talker\nutt0 0.3 0.2 a t\n', 'line 2: offset < onset'),
    ('#file onset offset #phone talker phone\nutt0 0.1 0.2 a t b\n', 'column "phone" is named twice'),
])
def test_item_file_refusals(tmp_path, text, message):
    path = str(tmp_path / 'bad.item')
    with open(path, 'w') as stream:
        stream.write(text)
    with pytest.raises(ValueError, match=message):
        AbxItems.load(path)


def test_a_refused_save_leaves_no_file(tmp_path):
    items = AbxItems(['utt0', 'utt 1'], [0.0, 0.5], [0.1, 0.6], {'phone': ['x', 'y']})
    path = tmp_path / 'bad.item'
    with pytest.raises(ValueError, match='item 1: a field is empty or holds white space'):
        items.save(str(path))
    assert not path.exists()
    with pytest.raises(ValueError, match='column name is empty or holds white space'):
        AbxItems(['utt0'], [0.0], [0.1], {'my phone': ['x']}).save(str(path))
    assert not path.exists()


def test_items_refuse_an_offset_before_its_onset():
    with pytest.raises(ValueError, match='item 1 .*offset < onset'):
        AbxItems(['a', 'b'], [0.0, 0.5], [0.1, 0.4], {'phone': ['x', 'y']})
    with pytest.raises(ValueError, match='one label per item'):
        AbxItems(['a', 'b'], [0.0, 0.5], [0.1, 0.6], {'phone': ['x']})


# ---- collapse -----------------------------------------------------------------------------------------------
def _hand_table():
    return AbxTable({
        'phone_1': np.array(['a', 'a', 'a', 'b', 'b', 'b']), 'phone_2': np.array(['b', 'b', 'b', 'a', 'a', 'a']),
        'talker': np.array(['t', 'u', 't', 't', 'u', 'u']), 'context': np.array(['c', 'c', 'd', 'c', 'c', 'd']),
        'score': np.array([1.0, 0.5, 0.25, 0.75, 0.25, 1.0]), 'n': np.full(6, 4), 'less': np.zeros(6, np.int64),
        'equal': np.zeros(6, np.int64)})


def test_collapse_on_a_hand_made_table():
    table = _hand_table()
    assert table.collapse() == np.mean([1.0, 0.5, 0.25, 0.75, 0.25, 1.0])
    # over talkers: (c, a, b) 0.75, (d, a, b) 0.25, (c, b, a) 0.5, (d, b, a) 1.0; over contexts: 0.5 and 0.75
    levels = [['context', 'phone_1', 'phone_2'], ['phone_1', 'phone_2']]
    assert table.collapse(levels) == 0.625
    assert table.error_rate(levels) == 37.5
    assert table.collapse([['context', 'phone_1', 'phone_2']]) == np.mean([0.75, 0.25, 0.5, 1.0])
    # (unweighted: one level at once weighs the cells, not the contexts - a different number)
    assert table.collapse([['phone_1', 'phone_2']]) == np.mean([np.mean([1.0, 0.5, 0.25]), np.mean([0.75, 0.25, 1.0])])
    with pytest.raises(ValueError, match='cannot group by column "speaker"'):
        table.collapse([['speaker']])
    assert np.isnan(AbxTable({'score': np.zeros(0), 'n': np.zeros(0, np.int64)}).collapse())


def test_collapse_by_the_references_levels_on_a_task_of_two_by_columns(tmp_path):
    """The within task of the reference (by talker and context) and its two level lists, against plain loops"""
    labels = _labels(6, 60)
    task = build_task(labels, **WITHIN)
    rng = np.random.default_rng(7)
    counts = np.zeros((task.n.shape[0], 3), dtype=np.uint64)
    counts[:, 0] = rng.integers(0, task.n + 1)
    counts[:, 1] = task.n - counts[:, 0].astype(np.int64)
    table = abx_module._table(task, counts)
    assert list(table.columns) == ['phone_1', 'phone_2', 'talker', 'context', 'score', 'n', 'less', 'equal']
    assert table['score'].dtype == np.float64 and table['n'].dtype == table['less'].dtype == np.int64
    first = {}
    for k in range(len(table)):
        first.setdefault((table['context'][k], table['phone_1'][k], table['phone_2'][k]), []).append(table['score'][k])
    second = {}
    for (context, p1, p2), scores in sorted(first.items()):
        second.setdefault((p1, p2), []).append(np.mean(scores))
    want = np.mean([np.mean(scores) for _, scores in sorted(second.items())])
    levels = [['context', 'phone_1', 'phone_2'], ['phone_1', 'phone_2']]
    assert abs(table.collapse(levels) - want) <= 4 * np.finfo(np.float64).eps   # (the order of a float64 sum)
    assert abs(table.error_rate(levels) - (1 - want) * 100) <= 1e-12
    path = str(tmp_path / 'within.csv')
    table.save_csv(path)
    lines = open(path).read().splitlines()
    assert lines[0].split('\t') == list(table.columns) and len(lines) == len(table) + 1
    assert [float(line.split('\t')[4]) for line in lines[1:]] == table['score'].tolist()
    # a cell with a bad triplet is an error that names it
    counts[2, 2] = 3
    with pytest.raises(ValueError, match=r'the cell \(talker=.*, context=.*, phone_1=.*, phone_2=.*\) has 3 triplets'):
        abx_module._table(task, counts)


# ---- argument errors: all before any device work ------------------------------------------------------------
def _collection():
    rng = np.random.default_rng(2)
    return FeaturesCollection([('utt%d' % k, dtw_cases.features(rng.standard_normal((100, 4)))) for k in range(3)])


def test_argument_errors_name_the_offender():
    feats, items = _collection(), _items()
    with pytest.raises(ValueError, match='invalid metric "kl"'):
        abx_scores(feats, items, 'phone', metric='kl')
    with pytest.raises(ValueError, match='unknown column "speaker"'):
        abx_scores(feats, items, 'phone', by=['speaker'])
    with pytest.raises(ValueError, match='unknown column "phon"'):
        abx_scores(feats, items, 'phon')
    with pytest.raises(ValueError, match='on column "phone" is also named in by or across'):
        abx_scores(feats, items, 'phone', by=['phone'])
    with pytest.raises(ValueError, match='on column "phone" is also named in by or across'):
        abx_scores(feats, items, 'phone', across='phone')
    with pytest.raises(ValueError, match='items must be an AbxItems'):
        abx_scores(feats, [('utt0', 0, 1)], 'phone')
    other = AbxItems(['utt0', 'nope'], [0, 0], [1, 1], {'phone': ['a', 'b']})
    with pytest.raises(ValueError, match='item 1: utterance "nope" is not in the collection'):
        abx_scores(feats, other, 'phone')
    empty = AbxItems(['utt0', 'utt1'], [0.0, 5.0], [0.5, 6.0], {'phone': ['a', 'b']})
    with pytest.raises(ValueError, match=r'item 1 \("utt1", 5.0, 6.0\) has no frames'):
        abx_scores(feats, empty, 'phone')
    long = FeaturesCollection([('a', dtw_cases.features(np.zeros((abx_module._dtw.MAX_FRAMES + 1, 2))))])
    with pytest.raises(ValueError, match='has 4097 frames, the limit is 4096'):
        abx_scores(long, AbxItems(['a'], [0.0], [1e9], {'phone': ['x']}), 'phone')
    mixed = FeaturesCollection([('a', dtw_cases.features(np.zeros((4, 3)))),
                                ('b', dtw_cases.features(np.zeros((4, 5))))])
    with pytest.raises(ValueError, match=r'items have different ndims: \[3, 5\]'):
        abx_scores(mixed, AbxItems(['a', 'b'], [0, 0], [1, 1], {'phone': ['x', 'y']}), 'phone')
    # a block beyond max_pairs: refused before the collection is uploaded
    items = AbxItems(['utt0'] * 4, [0.0] * 4, [0.5] * 4, {'phone': ['a', 'a', 'b', 'b']})
    with pytest.raises(ValueError, match=r'by-block \(all items\) has 4 items and needs 16 pairs, max_pairs is 15'):
        abx_scores(feats, items, 'phone', max_pairs=15)


def test_item_rows_are_those_dtw_distances_selects():
    feats, items = _collection(), _items()
    first, count, dim, block = abx_module._resolve(feats, items)
    triples = list(zip(items.names, items.onsets.tolist(), items.offsets.tolist()))
    want = abx_module._dtw._select(feats, np.zeros((0, 2), dtype=np.int64), triples)
    assert np.array_equal(first, want[0]) and np.array_equal(count, want[1]) and count.dtype == np.int32
    assert dim == 4 and block is None


def test_an_empty_task_gives_an_empty_table():
    feats = _collection()
    for items in (AbxItems([], [], [], {'phone': [], 'talker': []}),
                  AbxItems(['utt0', 'utt1'], [0, 0], [1, 1], {'phone': ['a', 'a'], 'talker': ['t', 'u']})):
        for across in (None, 'talker'):
            table = abx_scores(feats, items, 'phone', across=across)
            assert len(table) == 0 and table['score'].dtype == np.float64 and table['n'].dtype == np.int64
            assert list(table.columns)[:2] == ['phone_1', 'phone_2']


# ---- the C entry without a device ---------------------------------------------------------------------------
def test_abi_refuses_bad_arguments_before_any_device_work():
    """snf_abx_cells returns SNF_E_INVALID (a ValueError here) without asking for a device: this runs anywhere"""
    ok = [0, 4, 4, 2, 2, 2, 0, 0]   # within 16 distances: the last elements are 0 + 4 + 1 and 4 + 4 + 1

    def call(record=ok, n_dist=16, d_cost=4096, d_len=8192, d_counts=16384):
        _backend.abx_cells(d_cost, d_len, n_dist, np.array([ok, record]), d_counts)

    cases = [
        (dict(record=[0, 4, 4, 0, 2, 2, 0, 0]), 'cell 1 has an empty A, B or X list'),
        (dict(record=[0, 4, 4, 2, 0, 2, 0, 0]), 'cell 1 has an empty A, B or X list'),
        (dict(record=[0, 4, 4, 2, 2, -1, 0, 0]), 'cell 1 has an empty A, B or X list'),
        (dict(record=[0, 4, 4, 2, 2, 3, 1, 0]), 'cell 1 is marked same with nA != nX'),
        (dict(record=[-1, 4, 4, 2, 2, 2, 0, 0]), 'cell 1 reaches outside the 16 distances'),
        (dict(record=[0, 4, -4, 2, 2, 2, 0, 0]), 'cell 1 reaches outside the 16 distances'),
        (dict(record=[0, 11, 4, 2, 2, 2, 0, 0]), 'cell 1 reaches outside the 16 distances'),   # 11 + 4 + 1 = 16
        (dict(record=[0, 4, 4, 9, 2, 3, 0, 0]), 'cell 1 reaches outside the 16 distances'),    # 0 + 8 + 8 = 16
        (dict(record=[0, 4, 1 << 62, 2, 2, 3, 0, 0]), 'cell 1 reaches outside the 16 distances'),
        (dict(record=[0, 4, 4, 2, 2, 2, 0, 7]), 'cell 1: the last word of the record must be 0'),
        (dict(n_dist=-1), 'negative number of distances'),
        (dict(n_dist=9), 'cell 0 reaches outside the 9 distances'),
        (dict(d_cost=0), 'd_cost is null or not aligned'),
        (dict(d_cost=4098), 'd_cost is null or not aligned'),
        (dict(d_len=8193), 'd_len is not 4-byte aligned'),
        (dict(d_counts=0), 'd_counts is null or not 8-byte aligned'),
        (dict(d_counts=16388), 'd_counts is null or not 8-byte aligned'),
    ]
    for change, message in cases:
        with pytest.raises(ValueError, match=message):
            call(**change)
    # the largest cells that fit are accepted as far as the device (none here: not a ValueError)
    lib = _backend.lib()
    cells = np.zeros((1, 8), dtype=np.int64)
    import ctypes as C
    assert lib.snf_abx_cells(0, C.c_void_p(4096), None, 16, cells.ctypes.data_as(C.POINTER(C.c_int64)), -1,
                             C.c_void_p(8192), None) == _backend._abi.SNF_E_INVALID
    assert lib.snf_abx_cells(0, C.c_void_p(4096), None, 16, None, 1, C.c_void_p(8192), None) \
        == _backend._abi.SNF_E_INVALID
    # (no cell: nothing to do, whatever the pointers are - and no device is asked for)
    _backend.abx_cells(0, None, 0, np.zeros((0, 8)), 0)


def test_header_exports_and_library_agree():
    text = open(os.path.join(ROOT, 'include', 'shennong_amd.h')).read()
    assert re.search(r'int snf_abx_cells\(int device_id, const float\* d_cost, const int32_t\* d_len, int64_t n_dist,'
                     r'\s+const int64_t\* h_cells,\s+int64_t n_cells, uint64_t\* d_counts, void\* stream\);', text)
    assert 'abx_score.sh:22-23' in text and 'collapse_abx.py:35-42' in text
    assert 'snf_abx_cells' in _backend.EXPORTS and hasattr(_backend.lib(), 'snf_abx_cells')
    assert len(_backend.lib().snf_abx_cells.argtypes) == 8
