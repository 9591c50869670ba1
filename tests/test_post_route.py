"""The four launch ladders of the post-processing path (shennong_amd/csrc/post_route.h), on the CPU.

tests/tools/post_route_dump.cpp is compiled against post_route.h alone - host code, no device and no library - and
prints one line per case: which kernel launch_plp_tail, launch_deltas, launch_pitch_post and launch_cmvn_stats would
take, with which template choice, threads, rows per workgroup and dynamic LDS, whether the tile records are built and
whether the route refuses.  Every line is compared with the ladders as post_layouts.py restates them (the same
functions the GPU tests take their expected kernel names from), not with a recording of the program's output."""
import itertools
import os
import shutil
import subprocess

import pytest

import post_layouts as lay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'shennong_amd', 'csrc')

# PostKernel, in the order of the enum
KERNELS = ['plp_tail_exact_kernel', 'plp_tail_small_kernel', 'plp_tail_kernel', 'delta_flat_o2w2_kernel',
           'delta_tiled_fixed_kernel', 'delta_tiled_kernel', 'delta_kernel', 'pitch_post_tiled_kernel',
           'pitch_post_kernel', 'cmvn_stats_kernel', 'cmvn_stats_wide_kernel']

PLP_SHAPES = [(23, 12, 13), (23, 12, 12), (22, 12, 13), (32, 16, 13), (33, 16, 13), (32, 17, 13), (126, 63, 13),
              (127, 12, 13), (23, 64, 13)]
PLP_KNOBS = {'-': (), 'small': ('SNF_PLP_SMALL_TAIL',), 'generic': ('SNF_PLP_GENERIC_TAIL',),
             'both': ('SNF_PLP_SMALL_TAIL', 'SNF_PLP_GENERIC_TAIL')}
PLP_COMPRESS = ('third', '0.3')
DELTA_ORDERS = DELTA_WINDOWS = (1, 2, 3)
DELTA_COLS = (1, 13, 23, 40, 43, 44, 256, 257)
# (left context, right context, delta window, SNF_PITCH_POST_PER_FRAME)
PITCH_CASES = [(5000, 888, 2, 0), (5000, 889, 2, 0), (0, 5886, 2, 0), (3, 1, 7, 0), (-5, 10, 2, 0), (-5, 10, -1, 0),
               (75, 75, 2, 1), (75, 75, 2, 0)]
CMVN_COLS = (1, 128, 129, 256, 257)


def _compiler():
    for candidate in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    hipcc = _compiler()
    if hipcc is None:
        pytest.skip('no hipcc to compile tests/tools/post_route_dump.cpp with')
    tmp = tmp_path_factory.mktemp('post_route')
    program = str(tmp / 'post_route_dump')
    subprocess.run([hipcc, '-O1', '-std=c++17', '-Wall', '-I', CSRC, '-o', program,
                    os.path.join(ROOT, 'tests', 'tools', 'post_route_dump.cpp')], check=True, cwd=str(tmp))
    lines = subprocess.run([program], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
    return [(line.split()[0], dict(item.split('=', 1) for item in line.split()[1:] if '=' in item), line)
            for line in lines]


def _route(f):
    """(name, variant, threads, rows, lds, records built, refused) of a route line; the enum agrees with the name"""
    assert KERNELS[int(f['kernel'])] == f['name']
    return (f['name'], int(f['variant']), int(f['threads']), int(f['rows']), int(f['lds']), f['build'] == '1',
            f['refusal'] == '1')


def _delta_edge(order, window):
    """the last column count whose delta_tiled_kernel tile fits the 48 KiB bound and the first that does not"""
    first = next(c for c in range(1, 1000) if lay.delta_tiled_lds(order, window, c) > lay.LDS_LIMIT)
    return first - 1, first


def test_constants(dump):
    (f,) = [f for kind, f, _ in dump if kind == 'consts']
    assert (int(f['max_bins']), int(f['max_lpc'])) == (lay.PLP_MAX_BINS, lay.PLP_MAX_LPC) == (126, 63)
    assert (int(f['delta_rows']), int(f['post_rows'])) == (lay.DELTA_TILED_ROWS, lay.PITCH_POST_ROWS) == (256, 256)
    assert int(f['flat_tile_bytes']) == 28 * 1024 and int(f['lds_limit']) == lay.LDS_LIMIT == 48 * 1024
    assert f['flat'] == ''.join('%d:%d,' % (d, lay.flat_rows(d)) for d in lay.FLAT_COLS) == '13:132,23:72,40:40,43:36,'


def test_plp_route_is_the_ladder(dump):
    got = [f for kind, f, _ in dump if kind == 'plp']
    cases = list(itertools.product(PLP_SHAPES, PLP_KNOBS, PLP_COMPRESS))
    assert len(got) == len(cases) == 72
    seen = set()
    for f, (shape, knobs, compress) in zip(got, cases):
        assert ((int(f['bins']), int(f['order']), int(f['ceps'])), f['knobs'], f['compress']) == (shape, knobs, compress)
        refused = shape[0] > lay.PLP_MAX_BINS or shape[1] > lay.PLP_MAX_LPC
        name = 'plp_tail_kernel' if refused else lay.plp_route_of(shape, PLP_KNOBS[knobs])
        exact = name == 'plp_tail_exact_kernel'
        rows = lay.PLP_EXACT_ROWS if exact else lay.PLP_SMALL_ROWS
        want = (name, int(exact and compress != 'third'), rows, rows, 0, False, refused)
        assert _route(f) == want, (shape, knobs, compress)
        # the last two shapes refuse and nothing else does
        assert refused == (shape in PLP_SHAPES[-2:])
        seen.add((name, want[1], refused))
    assert seen == {('plp_tail_exact_kernel', 0, False), ('plp_tail_exact_kernel', 1, False),
                    ('plp_tail_small_kernel', 0, False), ('plp_tail_kernel', 0, False), ('plp_tail_kernel', 0, True)}
    texts = [line for kind, _, line in dump if kind == 'refusal']
    assert texts == ['refusal ' + lay.PLP_REFUSAL] * (2 * len(PLP_KNOBS) * len(PLP_COMPRESS))


def test_delta_route_is_the_ladder(dump):
    got = [f for kind, f, _ in dump if kind == 'delta']
    cases = [(order, window, cols, buffer, aligned)
             for order in DELTA_ORDERS for window in DELTA_WINDOWS
             for cols in DELTA_COLS + _delta_edge(order, window) for buffer in (1, 0) for aligned in (1, 0)]
    assert len(got) == len(cases) == 9 * 10 * 4
    names, flat_cols = set(), set()
    for f, (order, window, cols, buffer, aligned) in zip(got, cases):
        assert tuple(int(f[k]) for k in ('order', 'window', 'cols', 'buffer', 'aligned')) == \
            (order, window, cols, buffer, aligned)
        assert int(f['n_scales']) == lay.delta_n_scales(order, window)
        name = lay.delta_route_of(order, window, cols, records=bool(buffer), aligned=bool(aligned))
        # records are built exactly for order 2, window 2 and a flat column count with a buffer, aligned or not
        build = order == 2 and window == 2 and cols in lay.FLAT_COLS and bool(buffer)
        want = {'delta_flat_o2w2_kernel': (cols, 256, lay.flat_rows(cols), 0),
                'delta_tiled_fixed_kernel': (order, 256, lay.DELTA_TILED_ROWS,
                                             lay.delta_tiled_lds(order, window, cols, table=False)),
                'delta_tiled_kernel': (0, 256, lay.DELTA_TILED_ROWS, lay.delta_tiled_lds(order, window, cols)),
                'delta_kernel': (0, 256, 0, 0)}[name]
        assert _route(f) == (name,) + want + (build, False), (order, window, cols, buffer, aligned)
        assert int(f['lds']) <= lay.LDS_LIMIT
        names.add(name)
        if name == 'delta_flat_o2w2_kernel':
            flat_cols.add(cols)
    assert names == {'delta_flat_o2w2_kernel', 'delta_tiled_fixed_kernel', 'delta_tiled_kernel', 'delta_kernel'}
    assert flat_cols == set(lay.FLAT_COLS)


def test_delta_edges():
    """order 2, window 2: 2 048 + 64 + 1 056 x 44 = 48 576 bytes fit, 45 columns (49 632) do not; both sides of the
    edge take the kernels the bound separates"""
    assert _delta_edge(2, 2) == (44, 45)
    assert (lay.delta_tiled_lds(2, 2, 44), lay.delta_tiled_lds(2, 2, 45)) == (48576, 49632)
    for order, window in itertools.product(DELTA_ORDERS, DELTA_WINDOWS):
        last, first = _delta_edge(order, window)
        assert lay.delta_tiled_lds(order, window, last) <= lay.LDS_LIMIT < lay.delta_tiled_lds(order, window, first)
        assert first <= 256
        assert lay.delta_route_of(order, window, last, records=False) != 'delta_kernel'
        assert lay.delta_route_of(order, window, first, records=False) == 'delta_kernel'


def test_pitch_post_route_is_the_ladder(dump):
    got = [f for kind, f, _ in dump if kind == 'pitch']
    assert len(got) == len(PITCH_CASES)
    for f, (left, right, window, knob) in zip(got, PITCH_CASES):
        assert tuple(int(f[k]) for k in ('left', 'right', 'window', 'knob')) == (left, right, window, knob)
        assert (int(f['halo_l']), int(f['halo_r'])) == lay.pitch_halos(left, right, window)
        name = lay.pitch_route_of(left, right, window, per_frame=bool(knob))
        want = (256, 256, lay.pitch_lds(left, right, window)) if name == 'pitch_post_tiled_kernel' else (128, 128, 0)
        assert _route(f) == (name, 0) + want + (False, False), (left, right, window, knob)
        assert int(f['lds']) <= lay.LDS_LIMIT
    names = [f['name'] for f in got]
    tiled, per_frame = 'pitch_post_tiled_kernel', 'pitch_post_kernel'
    assert names == [tiled, per_frame, tiled, tiled, tiled, tiled, per_frame, tiled]
    # 8 x (256 + 5 888) = 49 152 is the last that fits; a window above the contexts and a negative context
    assert lay.pitch_lds(5000, 888, 2) == lay.pitch_lds(0, 5886, 2) == 49152 == lay.LDS_LIMIT
    assert lay.pitch_lds(5000, 889, 2) == 49160
    assert lay.pitch_halos(3, 1, 7) == (7, 7) and lay.pitch_halos(-5, 10, 2) == (2, 10)
    assert lay.pitch_halos(-5, 10, -1) == (0, 10)


def test_cmvn_stats_route_is_the_ladder(dump):
    got = [f for kind, f, _ in dump if kind == 'cmvn']
    assert [int(f['cols']) for f in got] == list(CMVN_COLS)
    for f, cols in zip(got, CMVN_COLS):
        r = lay.cmvn_row_groups(cols)
        want = ('cmvn_stats_kernel', 0, 256, r, 8 * r * (2 * cols + 1)) if cols <= 256 else \
            ('cmvn_stats_wide_kernel', 0, 256, 0, 0)
        assert _route(f) == want + (False, False), cols
        assert int(f['lds']) <= lay.LDS_LIMIT
    assert [int(f['rows']) for f in got] == [256, 2, 1, 1, 0]
    assert [int(f['lds']) for f in got] == [8 * 256 * 3, 8 * 2 * 257, 8 * 259, 8 * 513, 0]
    assert dict(lay.CMVN_COLS)[256] == 'cmvn_stats_kernel' and dict(lay.CMVN_COLS)[257] == 'cmvn_stats_wide_kernel'


def test_knob_parser(dump):
    """presence means on: the empty string and "0" switch a knob on like any other value, and only their own"""
    got = [(int(f['which']), f['in'], (int(f['generic']), int(f['small']), int(f['per_frame'])))
           for kind, f, _ in dump if kind == 'knobs']
    want = []
    for which in range(3):
        for text in ('-', 'empty', '0'):
            on = [0, 0, 0]
            on[which] = int(text != '-')
            want.append((which, text, tuple(on)))
    assert got == want
