"""The cases of tests/golden/reference_onehot.npz (make_golden_onehot.py), shared by test_onehot.py and
test_onehot_gpu.py: for every case and item the alignment, the processor parameters and the reference's answer."""

import os

import numpy as np

from shennong_amd.alignment import Alignment, AlignmentCollection

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
WINDOWS = ('blackman', 'hamming', 'hanning', 'povey', 'rectangular')
_CACHE = {}


def fixture():
    if 'npz' not in _CACHE:
        with np.load(os.path.join(GOLDEN, 'reference_onehot.npz')) as data:
            _CACHE['npz'] = {k: data[k] for k in data.files}
    return _CACHE['npz']


def collection():
    if 'collection' not in _CACHE:
        _CACHE['collection'] = AlignmentCollection.load(os.path.join(GOLDEN, 'alignment.txt'))
    return _CACHE['collection']


def synthetic():
    """The synthetic alignments of the fixture, in order"""
    if 'synthetic' not in _CACHE:
        ref = fixture()
        times, tokens, segments = ref['synthetic|times'], ref['synthetic|tokens'], ref['synthetic|segments']
        _CACHE['synthetic'] = [Alignment(times[a:b], tokens[a:b]) for a, b in zip(segments[:-1], segments[1:])]
    return _CACHE['synthetic']


def framed_cases():
    """(case, item, alignment, processor parameters) of every framed case of the fixture, none left out"""
    ali = collection()
    inventory = sorted(ali.get_tokens_inventory())
    cases = []
    for name, params in (('default', {}), ('shift02', {'frame_shift': 0.02}),
                         ('shift02_length05', {'frame_shift': 0.02, 'frame_length': 0.05}),
                         ('all_tokens', {'tokens': inventory})):
        cases += [(name, item, ali[item], params) for item in ali]
    cases += [(f'window_{kind}', 'S01F1522_0010', ali['S01F1522_0010'], {'window_type': kind}) for kind in WINDOWS]
    cases.append(('rate1000', 'literal', Alignment(np.asarray([[0, 1], [1, 2]]), np.asarray(['a', 'b'])),
                  {'sample_rate': 1000}))
    for kind in ('povey', 'rectangular', 'hamming'):
        cases += [(f'synthetic_{kind}', f'{i:03d}', a, {'window_type': kind}) for i, a in enumerate(synthetic())]
    # every winner array of the fixture belongs to a case above or to the unframed OneHotProcessor
    listed = {f'{case}|{item}|winner' for case, item, _, _ in cases}
    stored = {k for k in fixture() if k.endswith('|winner') and not k.startswith('plain')}
    assert listed == stored, sorted(listed ^ stored)[:5]
    return cases


def expected(case, item):
    """The reference's rows, bool [nframes, width]"""
    ref = fixture()
    winner, width = ref[f'{case}|{item}|winner'], int(ref[f'{case}|{item}|width'])
    data = np.zeros((winner.shape[0], width), dtype=bool)
    data[np.arange(winner.shape[0]), winner] = True
    return data
