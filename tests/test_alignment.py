"""shennong_amd.alignment: the literals and refusals of the reference's test/test_alignment.py, and
at_sample_rate against the reference's own walk over the samples (tests/golden/reference_onehot.npz)"""

import numpy as np
import pytest

import onehot_cases
from shennong_amd.alignment import Alignment, AlignmentCollection


@pytest.fixture(scope='module')
def ali():
    return Alignment.from_list([(0, 1, 'a'), (1, 2, 'b'), (2, 3.001, 'c')])


@pytest.fixture(scope='module')
def alignments():
    return onehot_cases.collection()


def test_bad_file():
    with pytest.raises(ValueError) as err:
        AlignmentCollection.load('/spam/spam/with/eggs')
    assert 'file not found' in str(err.value)


def test_bad_data():
    with pytest.raises(ValueError) as err:
        AlignmentCollection([['a', 1, 2, 'a'], ['a', 2, 3]])
    assert 'alignment must have 4 columns but line 2 has 3' in str(err.value)
    with pytest.raises(ValueError) as err:
        AlignmentCollection([['a', 1, 2, 'a'], ['a', 1, 2, 'b']])
    assert 'item a: mismatch in tstop/tstart timestamps' in str(err.value)


def test_simple(ali):
    assert ali.tokens.shape == (3,)
    assert ali._times.shape == (3, 2)
    assert ali._times.dtype == np.float64
    assert ali.duration() == pytest.approx(3.001)
    assert np.array_equal(np.array(['a', 'b', 'c']), ali.tokens)
    assert np.array([[0, 1], [1, 2], [2, 3.001]]) == pytest.approx(ali._times)
    assert np.array_equal(ali.onsets, [0, 1, 2]) and np.array_equal(ali.offsets, [1, 2, 3.001])
    assert ali.times is ali._times
    for bad in (1, slice(1, 2, 0), slice(None, None, 0)):
        with pytest.raises(ValueError):
            ali[bad]
    with pytest.raises(ValueError) as err:
        ali[1]
    assert 'time must be a slice but is' in str(err.value)
    with pytest.raises(ValueError) as err:
        ali[1:2:0]
    assert 'time.step is defined but is useless' in str(err.value)


def test_valid(ali):
    assert ali.is_valid()
    assert Alignment.from_list([]).is_valid()
    assert not Alignment.from_list([(0, 0, 'a')], validate=False).is_valid()
    for bad in ([(0, 1, 'a'), (1, 2, 'b'), (0, 3, 'a')], [(0, 1, 'a'), (0, 3, 'c')], [(0, 0, 'a')], [(1, 0, 'a')],
                [('a', 0, 'a')], [(0, 'a', 'a')], [(0, 1)], [(0, 1, 'a', 'a')]):
        with pytest.raises(ValueError):
            Alignment.from_list(bad)
    with pytest.raises(ValueError) as err:
        Alignment(np.asarray([[0, 1], [1, 2]]), np.asarray(['a', 'b', 'c']))
    assert 'timestamps and tokens must have the same length' in str(err.value)


def test_messages():
    for data, message in (
            ([(0, 1)], 'line 0: entry must have 3 fields but has 2'),
            ([(0, 1, 'a'), (1, 1, 'b')], 'token 1: onset must be lesser than offset'),
            ([(2, 3, 'a'), (1, 4, 'b')], 'timestamps must be sorted in increasing order'),
            ([(0, 1, 'a'), (1.5, 2, 'b')], 'mismatch in tstop/tstart timestamps')):
        with pytest.raises(ValueError) as err:
            Alignment.from_list(data)
        assert message in str(err.value)


def test_attributes(ali):
    for name in ('onsets', 'offsets', 'tokens', 'times'):
        with pytest.raises(AttributeError):
            setattr(ali, name, [])


def test_list(ali):
    ali2 = Alignment(np.array([[0, 1], [1, 2]]), np.array(['a', 'b']))
    assert ali[:2] == ali2
    assert ali2.to_list() == [(0, 1, 'a'), (1, 2, 'b')]
    assert Alignment.from_list(ali.to_list()) == ali


def test_repr(ali):
    assert str(ali[:1]) == '0.0 1.0 a'
    assert str(ali) == '0.0 1.0 a\n1.0 2.0 b\n2.0 3.001 c'
    assert str(ali[10:]) == ''


def test_partial_read(ali):
    for part in (ali[0:1],):
        assert np.array_equal(np.array([[0, 1]]), part._times)
        assert np.array_equal(np.array(['a']), part.tokens)
    for part in (ali[0:2], ali[:2]):
        assert np.array_equal(np.array([[0, 1], [1, 2]]), part._times)
        assert np.array_equal(np.array(['a', 'b']), part.tokens)


def test_complete_read(ali):
    for part in (ali[0:], ali[-1:], ali[:5], ali[-5:5], ali[:]):
        assert part is ali


def test_empty_read(ali):
    for part in (ali[:-1], ali[0:-1], ali[10:]):
        assert len(part._times) == 0
        assert len(part.tokens) == 0


@pytest.mark.parametrize('t', [0, 0.5, 1, 3.001])
def test_read_oneinstant(ali, t):
    part = ali[t:t]
    assert part.duration() == 0
    assert len(part.tokens) == 0


def test_read_intertokens(ali):
    for time, times, tokens in (
            (slice(0, 0.8), [[0, 0.8]], ['a']), (slice(0, 1), [[0, 1]], ['a']), (slice(0.2, 0.8), [[0.2, 0.8]], ['a']),
            (slice(0.2, 1), [[0.2, 1]], ['a']), (slice(1.2, 1.8), [[1.2, 1.8]], ['b']),
            (slice(0.2, 1.8), [[0.2, 1], [1, 1.8]], ['a', 'b']),
            (slice(0.2, 2.8), [[0.2, 1], [1, 2], [2, 2.8]], ['a', 'b', 'c']),
            (slice(0.2, 4), [[0.2, 1], [1, 2], [2, 3.001]], ['a', 'b', 'c'])):
        part = ali[time]
        assert part._times.shape == (len(tokens), 2)
        assert np.array(times) == pytest.approx(part._times)
        assert np.array_equal(part.tokens, np.array(tokens))
    assert np.array_equal(ali._times, [[0, 1], [1, 2], [2, 3.001]])   # (slices copy)


def test_realdata(alignments):
    ali = alignments['S01F1522_0003']
    assert ali.tokens.shape == (38,)
    assert np.array_equal(ali.tokens[:3], np.array(['k', 'y', 'o']))
    assert np.array_equal(ali[:0.1425].tokens, np.array(['k', 'y', 'o']))
    assert ali.duration() == pytest.approx(3.1)
    assert ali[3.2:].tokens.shape == (0,)
    assert str(alignments['S01F1522_0033']).split('\n')[:2] == ['0.0125 0.0425 m', '0.0425 0.1225 a']
    assert str(alignments['S01F1522_0033'][0.4325:0.6525]) == '0.4325 0.4925 a\n0.4925 0.5625 r\n0.5625 0.6525 a'


def test_sample_rate():
    ali = Alignment.from_list([[0, 1, 'a'], [1, 3, 'b']])
    assert list(ali.at_sample_rate(1)) == ['a', 'b', 'b']
    assert list(ali[:1].at_sample_rate(1)) == ['a']
    assert list(ali[:1].at_sample_rate(4)) == ['a'] * 4
    assert list(ali.at_sample_rate(4)) == ['a'] * 4 + ['b'] * 8
    assert len(list(ali.at_sample_rate(100))) == ali.duration() * 100
    ali = Alignment.from_list([[0, 0.8, 'a'], [0.8, 1, 'b']])
    assert list(ali.at_sample_rate(1)) == ['a']
    assert list(ali.at_sample_rate(2)) == ['a', 'a']
    assert list(ali.at_sample_rate(5)) == ['a', 'a', 'a', 'a', 'b']
    assert list(ali.at_sample_rate(10)) == ['a', 'a', 'a', 'a'] * 2 + ['b'] * 2
    ali = Alignment.from_list([[0, 0.2, 'a'], [0.2, 1, 'b']])
    assert list(ali.at_sample_rate(1)) == ['a']
    assert list(ali.at_sample_rate(2)) == ['a', 'b']
    assert list(ali.at_sample_rate(5)) == ['a', 'b', 'b', 'b', 'b']
    ali = Alignment.from_list([[0, 0.5, 'a'], [0.5, 1, 'b']])
    assert list(ali.at_sample_rate(1)) == ['a']
    assert list(ali.at_sample_rate(2)) == ['a', 'b']
    assert list(ali.at_sample_rate(3)) == ['a', 'a', 'b']
    empty = Alignment.from_list([])
    assert empty.duration() == 0 and empty.at_sample_rate(16000).shape == (0,)


def test_sample_rate_equals_reference(alignments):
    """Every sample of the 34 items at 16 kHz against the reference's walk"""
    ref = onehot_cases.fixture()
    inventory = np.array(sorted(alignments.get_tokens_inventory()))
    for item, ali in alignments.items():
        got = ali.at_sample_rate(16000)
        assert got.dtype == ali.tokens.dtype
        assert np.array_equal(got, inventory[ref[f'sampled|{item}|ids']]), item


def test_sample_rate_is_the_walk():
    """... and on the synthetic alignments (arbitrary float64 boundaries) against the walk written out"""
    for ali in onehot_cases.synthetic()[::7]:
        got = ali.at_sample_rate(16000)
        j, want = 0, []
        for i in range(int(ali.duration() * 16000)):
            while i / 16000 + ali.onsets[0] >= ali.offsets[j]:
                j += 1
            want.append(ali.tokens[j])
        assert list(got) == want


def test_load(alignments):
    assert 'S01F1522_0001' in alignments
    assert len(alignments) == 34
    assert all(a.is_valid() for a in alignments.values())


def test_inventory(alignments):
    tokens = alignments.get_tokens_inventory()
    assert 'e:' in tokens
    assert len(tokens) == 32
    assert alignments['S01F1522_0010'].get_tokens_inventory() == set(alignments['S01F1522_0010'].tokens)


@pytest.mark.parametrize('sort, compress', [(s, c) for s in (True, False) for c in (True, False)])
def test_save(tmpdir, alignments, sort, compress):
    filename = str(tmpdir.join('ali.txt' + ('.gz' if compress else '')))
    alignments.save(filename, sort=sort, compress=compress)
    with pytest.raises(ValueError) as err:
        alignments.save(filename, sort=sort)
    assert 'already exist' in str(err.value)
    with pytest.raises(ValueError) as err:
        alignments.save('/spam/spam/with/eggs', sort=sort)
    assert 'cannot write to' in str(err.value)
    again = AlignmentCollection.load(filename, compress=compress)
    assert alignments['S01F1522_0001'] == again['S01F1522_0001']
    assert alignments['S01F1522_0001'] != again['S01F1522_0002']
    assert alignments == again
    assert list(again) == (sorted(alignments) if sort else list(alignments))
    if not compress and not sort:
        with open(filename, encoding='utf8') as stream:
            assert stream.readline() == 'S01F1522_0001 0.0125 0.1125 e:\n'
