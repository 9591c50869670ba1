"""Shapes, frame counts, rows and references for the tests of the PLP tail and RASTA kernels (test_plp_tail.py on the
CPU, test_plp_tail_gpu.py on the device).  The routing of launch_plp_tail and the block heights of its kernels are
restated in post_layouts.py, not read from the source: a change of shennong_amd/csrc/post_route.h or
kernels_plp_tail.hip that moves a route or a seam has to be made there too, and `check_frames` / `check_edge_rows` /
`check_rasta_layout` then say what the cases no longer reach.

The rows are fed to the tail directly (Plan.debug_plp_tail), so a case measures the tail alone: the float64
statement (oracle/spec_f64.py plp_tail) and the float32 C oracle (oracle.plp_tail) read the very same float32 rows."""

import functools

import numpy as np

from oracle import oracle as orc
from oracle import spec_f64
from post_layouts import (PLP_EXACT_ROWS as EXACT_ROWS, PLP_EXACT_SHAPE as EXACT_SHAPE, PLP_MAX_BINS as MAX_BINS,
                          PLP_MAX_LPC as MAX_LPC, PLP_REFUSAL as REFUSAL, PLP_SMALL_BINS as SMALL_BINS,
                          PLP_SMALL_LPC as SMALL_LPC, PLP_SMALL_ROWS as SMALL_ROWS, plp_route_of as route_of)
from shennong_amd.processor import PlpProcessor

DURBIN_FLOOR = 1.0e-5
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)

# total frames: one, and both sides of a block of the 64- and of the 256-frame kernels; 515 = 2 x 256 + 3 = 8 x 64 + 3
# leaves an odd partial last block to both
FRAMES = (1, 64, 65, 256, 257, 515)
BIG_FRAMES = (65, 257)               # 126 / 63 / 64: the Python statement takes ~2 ms per frame there


# (id, shape, processor options, environment): every route, its bound shapes, the switches and the powf branch
SHAPE_CASES = [
    ('exact-23-12-13', (23, 12, 13), {}, ()),
    ('exact-23-12-13-compress0.5', (23, 12, 13), {'compress_factor': 0.5}, ()),
    ('exact-23-12-13-exactpow', (23, 12, 13), {}, ('SNF_PLP_EXACT_POW',)),
    ('small-23-12-12', (23, 12, 12), {}, ()),
    ('small-23-16-17', (23, 16, 17), {}, ()),
    ('small-32-16-17', (32, 16, 17), {}, ()),
    ('small-3-2-3', (3, 2, 3), {}, ()),
    ('small-23-12-13-switch', (23, 12, 13), {}, ('SNF_PLP_SMALL_TAIL',)),
    ('generic-33-12-13', (33, 12, 13), {}, ()),
    ('generic-23-17-13', (23, 17, 13), {}, ()),
    ('generic-40-20-21', (40, 20, 21), {}, ()),
    ('generic-126-63-64', (126, 63, 64), {}, ()),
    ('generic-23-12-13-switch', (23, 12, 13), {}, ('SNF_PLP_GENERIC_TAIL',)),
]
# the shapes both plp_tail_small_kernel and plp_tail_kernel accept ("same arithmetic, same order")
BOTH_SHAPES = [(23, 12, 13), (23, 12, 12), (32, 16, 17), (3, 2, 3)]
# options crossed on the default shape, on each of its three routes
OPTION_CASES = [
    {'use_energy': True},
    {'use_energy': True, 'htk_compat': True},
    {'use_energy': False, 'htk_compat': True},
    {'use_energy': True, 'cepstral_lifter': 0},
    {'use_energy': False, 'cepstral_lifter': 0, 'cepstral_scale': 0.9},
    {'use_energy': True, 'cepstral_scale': 0.9},
]
DEFAULT_ROUTES = [(), ('SNF_PLP_SMALL_TAIL',), ('SNF_PLP_GENERIC_TAIL',)]
ENERGY_FLOOR = 1.0e5     # the edge batch's floor case (a float32 number)


def frames_of(shape):
    return BIG_FRAMES if shape[0] > 64 else FRAMES


def check_frames(frames, rows):
    """a list of total frame counts reaches, at `rows` frames per workgroup: one workgroup filled exactly, one frame
    more, and an odd partial last workgroup behind more than one full one"""
    missing = []
    if rows not in frames:
        missing.append('full_block')
    if rows + 1 not in frames:
        missing.append('one_past_a_block')
    if not any(n > 2 * rows and (n % rows) % 2 == 1 for n in frames):
        missing.append('odd_partial_last_block')
    if missing:
        raise ValueError(f'frame counts {list(frames)} at {rows} frames per workgroup lack: {", ".join(missing)}')
    return frames


def processor(shape, **opts):
    """PlpProcessor of a shape; a bank of more than 64 bins gets 64 ms frames (1024-point spectrum: at 512 points
    the low filters of such a bank hold no spectral line, and the banks are refused)"""
    bins, order, ceps = shape
    opts.setdefault('use_energy', False)
    if bins > 64:
        opts.setdefault('frame_length', 0.064)
    return PlpProcessor(num_bins=bins, lpc_order=order, num_ceps=ceps, dither=0, **opts)


def _key(opts):
    return tuple(sorted(opts.items()))


def centers_of(proc):
    """centre frequencies of the processor's unwarped banks, from the float64 statement"""
    _, _, padded = spec_f64.frame_geometry(proc.sample_rate, proc.frame_shift, proc.frame_length, True)
    return spec_f64.mel_banks_vtln(proc.num_bins, proc.sample_rate, padded, float(proc.low_freq),
                                   float(proc.high_freq), float(proc.vtln_low), float(proc.vtln_high), 1.0)[1]


# ---- rows -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _regular(shape):
    """(rows float32 [n, bins], energies float64 [n]) for the longest run of the shape; a shorter run reads a prefix,
    so the runs of one shape share their first rows.  Row t is 10 ** (6 + 1.5 z), z a moving average of width
    1 + t % 4 of standard normals over the bins, divided by the square root of the width: spectra from white to
    smooth, six decades wide."""
    bins = shape[0]
    n = max(frames_of(shape))
    rng = np.random.default_rng([21, *shape])
    g = rng.standard_normal((n, bins + 3))
    z = np.empty((n, bins))
    for t in range(n):
        width = 1 + t % 4
        z[t] = sum(g[t, k:k + bins] for k in range(width)) / np.sqrt(width)
    rows = (10.0 ** (6.0 + 1.5 * z)).astype(np.float32)
    energy = 10.0 ** rng.uniform(2.0, 12.0, n)
    rows.setflags(write=False)
    energy.setflags(write=False)
    return rows, energy


def regular_rows(shape, frames=None):
    rows, energy = _regular(tuple(shape))
    frames = rows.shape[0] if frames is None else frames
    return rows[:frames], energy[:frames]


def durbin_margin(ac):
    """smallest 1 - k^2 of the Levinson-Durbin recursion per row of `ac` [n, order + 1], in ac's own precision and
    WITHOUT the floor (so a row that would reach it shows a value below DURBIN_FLOOR); also the residual energy"""
    ac = np.asarray(ac)
    dt = ac.dtype.type
    n, order = ac.shape[0], ac.shape[1] - 1
    lpc = np.zeros((n, order), dtype=ac.dtype)
    e = ac[:, 0].copy()
    worst = np.full(n, np.inf)
    for i in range(order):
        ki = ac[:, i + 1].copy()
        for j in range(i):
            ki = ki + lpc[:, j] * ac[:, i - j]
        ki = ki / e
        c = dt(1) - ki * ki
        worst = np.minimum(worst, c)
        e = e * np.maximum(c, dt(DURBIN_FLOOR))
        new = lpc.copy()
        new[:, i] = -ki
        for j in range(i):
            new[:, j] = lpc[:, j] - ki * lpc[:, i - j - 1]
        lpc = new
    return worst, e


def autocorrelation(proc, rows, dtype):
    """the tail up to the autocorrelation in `dtype` arithmetic (float64: the statement's; float32: the oracle's up
    to the last bits of powf and of the order of the sums)"""
    bins = proc.num_bins
    if dtype == np.float64:
        eql = spec_f64.equal_loudness(centers_of(proc))
        basis = spec_f64.idft_bases(proc.lpc_order + 1, bins + 2)
    else:
        opts = proc._build_options()
        center = orc.mel_banks(opts.mel, opts.frame)[3]
        eql = spec_f64.equal_loudness(center).astype(np.float32)
        basis = spec_f64.idft_bases(proc.lpc_order + 1, bins + 2).astype(np.float32)
    m = (rows.astype(dtype) * eql[None, :].astype(dtype)) ** dtype(np.float32(proc.compress_factor))
    dup = np.concatenate([m[:, :1], m, m[:, -1:]], axis=1)
    return (dup @ basis.T.astype(dtype)).astype(dtype)


def floor_hits(proc, rows):
    """rows whose Durbin recursion reaches the 1 - k^2 floor, in the statement's arithmetic or in float32"""
    with np.errstate(all='ignore'):
        m64, _ = durbin_margin(autocorrelation(proc, rows, np.float64))
        m32, _ = durbin_margin(autocorrelation(proc, rows, np.float32))
    return np.nonzero(~((m64 > DURBIN_FLOOR) & (m32 > DURBIN_FLOOR)))[0]


# ---- the edge batch ---------------------------------------------------------------------------------------------
EDGE = {'below_one': (0, 1), 'tiny': (2, 3), 'equal': (4, 5), 'energy_zero': 6, 'energy_1e-20': 7, 'energy_eps': 8,
        'energy_above_eps': 9, 'rows': 16}


@functools.lru_cache(maxsize=None)
def edge_rows(shape=EXACT_SHAPE):
    """16 rows: two regular rows times 1e-6 whose residual energy is below 1 (c0 = float64 eps exactly); a regular row
    times 1e-34 (its equal-loudness products lie on both sides of pow_third's 1e-30 line) and one times 1e-37
    (most of them below it, the smallest subnormal); two rows of equal values; regular rows for the rest.  Energies 0, 1e-20, float64 eps and the next double above it on rows 6-9."""
    proc = processor(shape)
    regular, energy = regular_rows(shape, 64)
    quiet = regular * np.float32(1e-6)
    _, e = durbin_margin(autocorrelation(proc, quiet, np.float64))
    below = np.nonzero(e < 0.5)[0][:2]
    rows = regular[20:20 + EDGE['rows']].copy()
    rows[0], rows[1] = quiet[below[0]], quiet[below[1]]
    rows[2] = regular[2] * np.float32(1e-34)
    rows[3] = regular[3] * np.float32(1e-37)
    rows[4] = np.float32(1e6)
    rows[5] = np.float32(3.0)
    energy = energy[20:20 + EDGE['rows']].copy()
    energy[6], energy[7], energy[8], energy[9] = 0.0, 1e-20, EPS64, np.nextafter(EPS64, 1.0)
    rows.setflags(write=False)
    energy.setflags(write=False)
    return rows, energy


def check_edge_rows(shape=EXACT_SHAPE):
    """the edge batch reaches what it claims; raises ValueError naming what it lacks"""
    proc = processor(shape)
    rows, energy = edge_rows(shape)
    missing = []
    for dtype in (np.float64, np.float32):
        with np.errstate(all='ignore'):
            _, e = durbin_margin(autocorrelation(proc, rows, dtype))
        if not all(0.0 < e[k] < 1.0 for k in EDGE['below_one']):
            missing.append(f'residual energy below one ({dtype.__name__})')
    opts = proc._build_options()
    eql = spec_f64.equal_loudness(orc.mel_banks(opts.mel, opts.frame)[3]).astype(np.float32)
    for k in EDGE['tiny']:
        prod = rows[k] * eql
        if not (np.count_nonzero(prod < np.float32(1e-30)) >= 5 and np.all(prod > 0)):
            missing.append(f'row {k} below the tiny line')
    if not np.any(rows[EDGE['tiny'][0]] * eql >= np.float32(1e-30)):
        missing.append('a row on both sides of the tiny line')
    if not all(np.all(rows[k] == rows[k][0]) for k in EDGE['equal']):
        missing.append('rows of equal values')
    if not (energy[EDGE['energy_zero']] == 0 and 0 < energy[EDGE['energy_1e-20']] < EPS64 and
            energy[EDGE['energy_eps']] == EPS64 and energy[EDGE['energy_above_eps']] > EPS64):
        missing.append('energies around float64 eps')
    if np.count_nonzero(energy < ENERGY_FLOOR) < 5 or np.count_nonzero(energy > ENERGY_FLOOR) < 2:
        missing.append('energies on both sides of the floor')
    if missing:
        raise ValueError('the edge batch lacks: ' + ', '.join(missing))
    return rows, energy


# ---- references (computed once per case, read only) ---------------------------------------------------------------
def statement(proc, rows, energy):
    with np.errstate(divide='ignore'):
        log_energy = np.log(np.maximum(np.asarray(energy, dtype=np.float64), EPS64))
    return spec_f64.plp_tail(
        rows, centers_of(proc), log_energy, lpc_order=proc.lpc_order, num_ceps=proc.num_ceps,
        cepstral_lifter=float(proc.cepstral_lifter), cepstral_scale=float(proc.cepstral_scale),
        compress_factor=float(proc.compress_factor), use_energy=bool(proc.use_energy),
        energy_floor=float(np.float32(proc.energy_floor)), htk_compat=bool(proc.htk_compat))


@functools.lru_cache(maxsize=None)
def reference(shape, opts_key=(), batch='regular'):
    """(rows, energies, float64 statement, float32 oracle, bound [num_ceps]) of a case's longest run.  The bound is
    the project's rule for kernels with powf / logf / expf: per output column, 4 times the oracle's own worst error
    against the statement over the batch."""
    proc = processor(shape, **dict(opts_key))
    rows, energy = regular_rows(shape) if batch == 'regular' else edge_rows(shape)
    want = statement(proc, rows, energy)
    oracle = orc.plp_tail(proc._build_options(), rows, energy)
    bound = 4.0 * np.abs(oracle.astype(np.float64) - want).max(axis=0)
    for a in (want, oracle, bound):
        a.setflags(write=False)
    return rows, energy, want, oracle, bound


def log_columns(proc):
    """output columns that hold a logarithm (c0, or the log energy): [index]"""
    return [proc.num_ceps - 1 if proc.htk_compat else 0]


def allowance(proc, want, bound, route):
    """[n, num_ceps] what the device may err from `want`: the 4 x rule; plp_tail_exact_kernel takes a float logf
    "good to an ulp" where the oracle's double logarithm is correctly rounded, so its logarithm column gets 2 ulp of
    |want| on top (the allowance of the raw log-pitch column in test_post_routes_gpu.py)"""
    allow = np.broadcast_to(bound, want.shape).copy()
    if route == 'plp_tail_exact_kernel':
        for c in log_columns(proc):
            allow[:, c] += 2.0 * np.spacing(np.abs(want[:, c]).astype(np.float32)).astype(np.float64)
    return allow


# ---- RASTA --------------------------------------------------------------------------------------------------------
RASTA_LENGTHS = [0, 1, 2, 3, 4, 5, 6, 0, 50, 9]
RASTA_BINS = (23, 3)
RASTA_THREADS = 64
RASTA_ZERO = (8, 2)      # (utterance, bin): exactly 0 in every frame
RASTA_QUIET = (9, 1)     # ... 1e-9 in every frame: below float32 eps, far above float64 eps


def check_rasta_layout(lengths, bins):
    missing = []
    for n in range(7):
        if n not in lengths:
            missing.append(f'length_{n}')
    if not any(n == 0 and 0 < u < len(lengths) - 1 for u, n in enumerate(lengths)):
        missing.append('empty_between')
    if not any(n > 8 for n in lengths):
        missing.append('long')
    threads = len(lengths) * bins
    if bins == 23 and not (threads > RASTA_THREADS and threads % RASTA_THREADS):
        missing.append('partial_last_block')
    if missing:
        raise ValueError(f'RASTA layout {list(lengths)} x {bins} bins lacks: {", ".join(missing)}')
    return lengths


@functools.lru_cache(maxsize=None)
def rasta_batch(bins):
    """(rows [total, bins] float32, offsets): regular rows with one bin of utterance 8 at exactly 0 and one bin of
    utterance 9 at 1e-9"""
    lengths = check_rasta_layout(RASTA_LENGTHS, bins)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    shape = (bins, 2, 3) if bins == 3 else EXACT_SHAPE
    rows = regular_rows(shape, int(off[-1]))[0].copy()
    (u, b) = RASTA_ZERO
    rows[off[u]:off[u + 1], b] = 0.0
    (u, b) = RASTA_QUIET
    rows[off[u]:off[u + 1], b] = np.float32(1e-9)
    rows.setflags(write=False)
    return rows, off


@functools.lru_cache(maxsize=None)
def rasta_reference(bins):
    """(rows, offsets, statement with float32 eps per utterance, oracle per utterance, bound [bins]): the bound is 4
    times the oracle's worst error per bin over the utterances of more than 4 frames"""
    rows, off = rasta_batch(bins)
    spans = list(zip(off[:-1], off[1:]))
    want = [spec_f64.rasta(rows[a:b], eps=EPS32) if b > a else np.zeros((0, bins)) for a, b in spans]
    oracle = [orc.rasta(rows[a:b]) if b > a else np.zeros((0, bins), np.float32) for a, b in spans]
    errs = [np.abs(o.astype(np.float64) - w).max(axis=0) for o, w in zip(oracle, want) if o.shape[0] > 4]
    bound = 4.0 * np.max(errs, axis=0)
    return rows, off, want, oracle, bound
