"""Batch layouts for the route tests of the delta, pitch-post and CMVN kernels (test_post_routes.py and
test_post_routes_gpu.py): lists of utterance lengths whose concatenation, cut into tiles of R rows, puts an
utterance boundary on every kind of tile seam.  The tile heights are restated here, not read from the source:
a change of shennong_amd/csrc/post_route.h that moves a seam has to be made here too, and `check_seams` then says
what the layouts no longer reach.  The four launch ladders of that header are restated here as well (`plp_route_of`,
`delta_route_of`, `pitch_route_of`, `cmvn_row_groups`): the GPU tests take their expected kernel names from them, and
test_post_route.py compares them with the header itself on the CPU.

The second half holds the layouts and restated launch arithmetic of the remaining kernels of the path
(test_post_remaining.py, test_post_remaining_gpu.py): the 256-thread stride loop of vad_threshold_kernel, the 64
threads per workgroup of sliding_cmvn_kernel, the 32-row tiles of concat_columns_kernel, the capped grid of
count_nonfinite_kernel and the waves, workgroups and tiles of mfcc_dct_kernel (kernels_dct.hip)."""

import numpy as np

DELTA_TILED_ROWS = 256   # kDeltaRows: delta_tiled_kernel, delta_tiled_fixed_kernel
PITCH_POST_ROWS = 256    # kPostRows: pitch_post_tiled_kernel
FLAT_COLS = (13, 23, 40, 43)   # column counts with a delta_flat_o2w2_kernel instantiation
FLAT_HALO = 4            # order 2 x window 2


def flat_rows(cols):
    """Rows per tile of delta_flat_o2w2_kernel<cols>: a multiple of 4 that fits 28 KiB of LDS"""
    rows = (28 * 1024 // 4 - 8 * cols - 8) // (4 * cols)
    rows &= ~3
    return min(rows, 256)


assert [flat_rows(d) for d in FLAT_COLS] == [132, 72, 40, 36]


# ---- the launch ladders, restated ----------------------------------------------------------------------------------
LDS_LIMIT = 48 * 1024    # dynamic LDS a workgroup of this path asks for at the most
PLP_EXACT_ROWS = 256     # frames per workgroup of plp_tail_exact_kernel
PLP_SMALL_ROWS = 64      # ... of plp_tail_small_kernel and plp_tail_kernel
PLP_MAX_BINS, PLP_MAX_LPC = 126, 63          # kMaxBins, kMaxLpc
PLP_SMALL_BINS, PLP_SMALL_LPC = 32, 16       # the bound of plp_tail_small_kernel<32, 16>
PLP_EXACT_SHAPE = (23, 12, 13)               # (mel bins, LPC order, cepstra) of plp_tail_exact_kernel<23, 12, 13>
PLP_REFUSAL = 'PLP: num_bins > 126 or lpc_order > 63 not supported'


def plp_route_of(shape, env=()):
    """the kernel launch_plp_tail takes for a shape under the switches in `env`"""
    bins, order, _ = shape
    if tuple(shape) == PLP_EXACT_SHAPE and 'SNF_PLP_GENERIC_TAIL' not in env and 'SNF_PLP_SMALL_TAIL' not in env:
        return 'plp_tail_exact_kernel'
    if bins <= PLP_SMALL_BINS and order <= PLP_SMALL_LPC and 'SNF_PLP_GENERIC_TAIL' not in env:
        return 'plp_tail_small_kernel'
    return 'plp_tail_kernel'


def delta_n_scales(order, window):
    """entries of DeltaParams::scales: 2 i window + 1 taps for every order i"""
    return sum(2 * i * window + 1 for i in range(order + 1))


def delta_tiled_lds(order, window, cols, table=True):
    """LDS bytes of delta_tiled_kernel; without the scale table, of delta_tiled_fixed_kernel"""
    lds = 2 * 4 * 256 + 4 * (256 + 2 * order * window) * cols
    return lds + 4 * ((delta_n_scales(order, window) + 3) & ~3) if table else lds


def delta_route_of(order, window, cols, records=True, aligned=True):
    """launch_deltas' choice; `records`: the caller gave a buffer for the tile records, `aligned`: input and output
    are 16-byte aligned"""
    if order == 2 and window == 2 and cols in FLAT_COLS and records and aligned:
        return 'delta_flat_o2w2_kernel'
    if delta_tiled_lds(order, window, cols) <= LDS_LIMIT and cols <= 256:
        return 'delta_tiled_fixed_kernel' if window == 2 and order in (1, 2) else 'delta_tiled_kernel'
    return 'delta_kernel'


def pitch_halos(left, right, window):
    """frames that pitch_post_tiled_kernel stages before and behind its 256 rows"""
    return max(left, window, 0), max(right, window, 0)


def pitch_lds(left, right, window):
    """LDS bytes of pitch_post_tiled_kernel: a POV weight and a log pitch per staged frame"""
    return 2 * 4 * (PITCH_POST_ROWS + sum(pitch_halos(left, right, window)))


def pitch_route_of(left, right, window, per_frame=False):
    if pitch_lds(left, right, window) <= LDS_LIMIT and not per_frame:
        return 'pitch_post_tiled_kernel'
    return 'pitch_post_kernel'


def cmvn_row_groups(cols):
    """R: the rows of an utterance that cmvn_stats_kernel's 256 threads reduce in parallel"""
    return max(1, 256 // cols)


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def seams(lengths, rows):
    """What a layout reaches at tile height `rows`: a dict of the properties `check_seams` asks for"""
    lengths = [int(n) for n in lengths]
    off = offsets_of(lengths)
    spans = [(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]
    total = int(off[-1])
    found = {}
    # an utterance of 2 rows + 8 frames or more that starts inside a tile and holds a tile 4 rows inside it
    found['interior'] = any(
        b - a >= 2 * rows + 8 and a % rows and
        any(k * rows >= a + FLAT_HALO and (k + 1) * rows <= b - FLAT_HALO for k in range(a // rows, b // rows + 1))
        for a, b in spans)
    # six one-frame utterances in one tile with an empty utterance between the first and the last of them
    found['many_boundaries'] = False
    for k in range((total + rows - 1) // rows):
        ones = [u for u, (a, b) in enumerate(spans) if b - a == 1 and a // rows == k]
        if len(ones) >= 6 and any(lengths[u] == 0 for u in range(ones[0], ones[-1])):
            found['many_boundaries'] = True
    ends = [b for a, b in spans if b > a]
    found['ends_on_seam'] = any(b % rows == 0 for b in ends)
    for k in range(1, 5):
        found[f'ends_{k}_before'] = any(b % rows == rows - k for b in ends)
        found[f'ends_{k}_after'] = any(b > rows and b % rows == k for b in ends)
    for n in (1, 2, 3):
        found[f'length_{n}'] = n in lengths
    found['leading_empty'] = lengths[0] == 0
    found['trailing_empty'] = lengths[-1] == 0
    found['odd_partial_last_tile'] = (total % rows) % 2 == 1
    return found


def check_seams(lengths, rows):
    missing = [name for name, ok in seams(lengths, rows).items() if not ok]
    if missing:
        raise ValueError(f'layout {list(lengths)} at {rows} rows per tile lacks: {", ".join(missing)}')
    return lengths


def seam_layout(rows):
    """Utterance lengths, about 5.5 tiles of `rows` rows in all (rows >= 36):

    tile 0      an empty utterance, lengths 1, 2 and 3, six one-frame utterances around an empty one (more
                than two boundaries in one tile), an utterance that ends 3 rows before the seam
    seam 1      ends at -3, -1, +2, +4 rows around it (the utterances between them are shorter than a halo)
    tiles 1-3   ONE utterance from row `rows + 4` to the seam at 4 `rows`: tile 2 lies wholly inside it
    seam 5      ends at -4, -2, +1, +3
    last tile   partial with an odd number of rows, then an empty utterance"""
    if rows < 36:
        raise ValueError('the layouts are written for tiles of 36 rows or more')
    return check_seams(_seam_lengths(rows), rows)


def _seam_lengths(rows):
    """the lengths of `seam_layout`, unchecked (rows >= 32: the first seam's utterances need 12 + 3 rows below it)"""
    lengths = [0, 1, 2, 3, 1, 1, 1, 0, 1, 1, 1]              # 12 rows
    lengths += [rows - 3 - 12, 2, 3, 2]                      # ends rows-3, rows-1, rows+2, rows+4
    lengths += [4 * rows - (rows + 4)]                       # ... 4 rows: exactly on the seam
    lengths += [rows - 4, 2, 3, 2]                           # ends 5 rows -4, -2, +1, +3
    tail = (rows // 2) & ~1                                  # 3 + tail rows in the last tile: odd
    lengths += [tail, 0]
    return lengths


def seam_layout_small():
    """Two batches shorter than any tile: one frame in all, and five frames with empty utterances around them"""
    return [[1], [0, 3, 0, 2]]


# ---- the cases of both test modules ------------------------------------------------------------------------------
def layout_of(name):
    """'small0' / 'small1': the batches of `seam_layout_small`; an integer: `seam_layout` at that tile height"""
    if isinstance(name, str):
        return seam_layout_small()[int(name[-1])]
    return seam_layout(int(name))


# (route, order, window, columns, layout): every launch route of launch_deltas
DELTA_CASES = []
for _cols in FLAT_COLS:
    DELTA_CASES += [('delta_flat_o2w2_kernel', 2, 2, _cols, name) for name in (flat_rows(_cols), 'small0', 'small1')]
DELTA_CASES += [
    ('delta_tiled_fixed_kernel', 2, 2, 7, DELTA_TILED_ROWS),
    ('delta_tiled_fixed_kernel', 2, 2, 39, DELTA_TILED_ROWS),
    ('delta_tiled_fixed_kernel', 1, 2, 13, DELTA_TILED_ROWS),
    ('delta_tiled_kernel', 3, 3, 13, DELTA_TILED_ROWS),
    ('delta_tiled_kernel', 1, 1, 1, DELTA_TILED_ROWS),
    ('delta_tiled_kernel', 5, 5, 20, DELTA_TILED_ROWS),    # halo 25: longer than most utterances of the layout
    ('delta_tiled_kernel', 0, 2, 13, DELTA_TILED_ROWS),
    ('delta_kernel', 5, 5, 40, DELTA_TILED_ROWS),          # 306 rows x 40 columns: more than 48 KiB of LDS
    ('delta_kernel', 2, 2, 257, DELTA_TILED_ROWS),         # more than 256 columns
]


def delta_id(case):
    route, order, window, cols, name = case
    return f'{route}-o{order}w{window}-d{cols}-{name}'


# (route, left context, right context, delta window): launch_pitch_post
PITCH_CONTEXTS = [
    ('pitch_post_tiled_kernel', 75, 75, 2),
    ('pitch_post_tiled_kernel', 0, 0, 1),
    ('pitch_post_tiled_kernel', 300, 10, 4),
    ('pitch_post_tiled_kernel', 10, 300, 3),
    ('pitch_post_kernel', 6000, 0, 2),       # 2 x 4 x (256 + 6000) bytes: more than 48 KiB of LDS
    ('pitch_post_kernel', 0, 6000, 2),
]
# (POV feature, normalised log pitch, delta, raw log pitch)
PITCH_FLAGS = [(1, 1, 1, 1), (0, 1, 0, 0), (0, 0, 1, 0), (1, 0, 0, 1)]

# columns of the CMVN statistics kernels: cmvn_stats_kernel up to 256, cmvn_stats_wide_kernel above
CMVN_COLS = [(d, 'cmvn_stats_kernel') for d in (1, 13, 85, 128, 129, 256)] + \
            [(d, 'cmvn_stats_wide_kernel') for d in (257, 300)]
CMVN_WEIGHTS = ('none', 'some_zero', 'one_utterance_all_zero')


def cmvn_lengths(cols):
    """utterance lengths around the R = 256 // cols rows that cmvn_stats_kernel reduces in parallel"""
    r = cmvn_row_groups(cols)
    return [0, 1, r - 1, r, r + 1, 1000]


# ---- the remaining kernels of the same path (test_post_remaining.py, test_post_remaining_gpu.py) ------------------
VAD_THREADS = 256        # vad_threshold_kernel: one workgroup of 256 threads per utterance, `t += blockDim.x`
SLIDING_THREADS = 64     # sliding_cmvn_kernel: one thread per (utterance, column), 64 per workgroup
CONCAT_ROWS = 32         # kConcatRows: output rows per workgroup of concat_columns_kernel
NONFINITE_THREADS = 256  # count_nonfinite_kernel: 256 threads, 4 floats each, at most ...
NONFINITE_MAX_BLOCKS = 4096   # ... 256 * 16 workgroups (launch_count_nonfinite)


def check_vad_passes(lengths):
    """the utterance lengths around the 256-thread stride loop of vad_threshold_kernel: zero, one and two extra
    passes, a partial wave in the last one, an utterance of many passes, empty utterances at the head, inside and
    at the tail"""
    lengths = [int(n) for n in lengths]
    missing = [str(n) for n in (VAD_THREADS - 1, VAD_THREADS, VAD_THREADS + 1, 2 * VAD_THREADS + 1, 1, 2, 3)
               if n not in lengths]
    if max(lengths) <= 2 * VAD_THREADS + 1:
        missing.append('an utterance longer than 513 frames')
    if lengths[0] or lengths[-1] or 0 not in lengths[1:-1]:
        missing.append('empty utterances at the head, inside and at the tail')
    if missing:
        raise ValueError(f'VAD layout {lengths} lacks: {", ".join(missing)}')
    return lengths


def vad_layout():
    """`seam_layout(256)` - about 1 400 frames, a 764-frame utterance, empty utterances at the head, in the middle
    and at the tail, lengths 1, 2 and 3 - with utterances of 255, 256, 257 and 513 frames in front of its last,
    empty, one"""
    base = seam_layout(VAD_THREADS)
    return check_vad_passes(base[:-1] + [VAD_THREADS - 1, VAD_THREADS, VAD_THREADS + 1, 2 * VAD_THREADS + 1] + base[-1:])


# (frames_context, energy_mean_scale, proportion_threshold, energy_threshold); the columns are crossed with them
# (a context of 300 frames with half of the energies above the threshold: a proportion of 0.5 keeps the flags mixed)
VAD_OPTIONS = [(0, 0.5, 0.6, 5.0), (2, 0.5, 0.6, 5.0), (300, 0.5, 0.5, 5.0), (2, 0.0, 0.6, 10.0),
               (0, 0.5, 0.5, 5.0), (2, 0.5, 0.25, 5.0), (300, 0.0, 0.5, 10.0)]
VAD_COLS = (1, 13, 40)
# the exact-arithmetic cases: (frames_context, proportion_threshold)
VAD_TIES = [(0, 0.5), (2, 0.6), (2, 0.25), (0, 0.6)]

# (cmn_window, min_window) of the sliding-window CMVN cases: even; odd and centred; min_window > cmn_window;
# larger than every utterance
SLIDING_WINDOWS = [(40, 40), (41, 10), (7, 50), (600, 100)]
SLIDING_COLS = (1, 13, 64, 257)


SLIDING_CASES = [(w, c, v) for w in SLIDING_WINDOWS for c in (True, False) for v in (False, True)]


def sliding_id(case):
    (cmn, minw), center, nv = case
    return f'w{cmn}-m{minw}-{"centre" if center else "left"}-{"var" if nv else "mean"}'


def sliding_lengths(cmn_window, min_window):
    """0, 1, 2, 3, cmn_window - 1, cmn_window, cmn_window + 1, min_window - 1, min_window + 1 and
    2 cmn_window + 5 frames, the empty utterances at the head, in the middle and at the tail of the batch"""
    return [0, 1, 2, 3, cmn_window - 1, cmn_window, 0, cmn_window + 1, min_window - 1, min_window + 1,
            2 * cmn_window + 5, 0]


def sliding_five(cmn_window, min_window):
    """five utterances, none empty: with 13 columns 65 threads, the last one alone in a second workgroup"""
    return [3, cmn_window + 1, 1, min_window + 1, 2]


def check_sliding(lengths, cmn_window, min_window):
    lengths = [int(n) for n in lengths]
    need = {0, 1, 2, 3, cmn_window - 1, cmn_window, cmn_window + 1, min_window - 1, min_window + 1,
            2 * cmn_window + 5}
    missing = sorted(need - set(lengths))
    if lengths[0] or lengths[-1] or 0 not in lengths[1:-1]:
        missing.append('empty utterances at the head, inside and at the tail')
    if missing:
        raise ValueError(f'sliding layout {lengths} lacks: {missing}')
    return lengths


def sliding_threads(lengths, cols):
    """(threads, workgroups, threads of the last workgroup, True when some workgroup holds columns of two utterances
    in one wave) of launch_sliding_cmvn"""
    threads = len(lengths) * cols
    blocks = (threads + SLIDING_THREADS - 1) // SLIDING_THREADS
    inside = any((u * cols) % SLIDING_THREADS for u in range(1, len(lengths)))
    return threads, blocks, threads - (blocks - 1) * SLIDING_THREADS, inside


# (cols_a, cols_b) of the concatenation cases: 32 (ca + cb) a multiple of 256 and not
CONCAT_COLS = [(1, 1), (13, 3), (40, 2), (3, 13), (257, 2), (2, 257)]
CONCAT_TRIM = [(0, 0), (2, 0), (0, 3), (1, 5), (4, 1)]   # rows that (a, b) hold beyond the output, by utterance % 5


def concat_layout():
    """(rows of the output, of a, of b) per utterance: the output is `seam_layout`'s list at 32 rows per tile - every
    seam of check_seams, empty utterances included -, a and b are longer by CONCAT_TRIM, so that the input offsets
    drift away from the output offsets"""
    out = check_seams(_seam_lengths(CONCAT_ROWS), CONCAT_ROWS)
    a = [n + CONCAT_TRIM[u % len(CONCAT_TRIM)][0] for u, n in enumerate(out)]
    b = [n + CONCAT_TRIM[u % len(CONCAT_TRIM)][1] for u, n in enumerate(out)]
    return out, a, b


def check_concat(out, a, b):
    """some utterances with a longer than the output, some with b longer, some with both, some with neither; an
    empty output with rows in a or b; the offsets of a and of b differ from the output's from the second tile on"""
    kinds = {(x > n, y > n) for n, x, y in zip(out, a, b)}
    missing = [str(k) for k in ((False, False), (True, False), (False, True), (True, True)) if k not in kinds]
    if any(x < n or y < n for n, x, y in zip(out, a, b)):
        missing.append('an input shorter than the output')
    if not any(n == 0 and (x or y) for n, x, y in zip(out, a, b)):
        missing.append('an empty output of a non-empty input')
    oo, oa, ob = offsets_of(out), offsets_of(a), offsets_of(b)
    late = [u for u in range(len(out)) if oo[u] >= CONCAT_ROWS and out[u]]
    if not late or any(oa[u] == oo[u] or ob[u] == oo[u] or oa[u] == ob[u] for u in late):
        missing.append('drifting offsets')
    if missing:
        raise ValueError(f'concat layout lacks: {", ".join(missing)}')
    return out, a, b


# sizes of the non-finite count: the tail alone, body + tail, and the capped grid
NONFINITE_GRID = 4 * NONFINITE_THREADS * NONFINITE_MAX_BLOCKS           # floats one pass of the capped grid reads
NONFINITE_SIZES = [1, 2, 3, 4, 5, 7, 1024, 1025, 1027, NONFINITE_GRID + 3]
# NONFINITE_GRID + 3 = 4 194 307 fills the capped grid exactly ONCE (see nonfinite_launch): a second pass needs
# more than NONFINITE_GRID / 4 vectors.  This size gives workgroups 0 and 1 a second pass, and a tail of 3
NONFINITE_SECOND_PASS = NONFINITE_GRID + 4 * (NONFINITE_THREADS + 1) + 3


def nonfinite_launch(n):
    """launch_count_nonfinite restated: (workgroups, vectors of 4 floats, passes of the stride loop that thread 0
    of workgroup 0 makes, floats of the tail)"""
    n4 = n // 4
    blocks = min(max((n4 + NONFINITE_THREADS - 1) // NONFINITE_THREADS, 1), NONFINITE_MAX_BLOCKS)
    stride = blocks * NONFINITE_THREADS
    return blocks, n4, (n4 + stride - 1) // stride, n % 4


def nonfinite_places(n):
    """indices worth a lone non-finite value: element 0, the last of the vector body, every tail element, and the
    first elements a thread reaches in its second pass (workgroups 0 and 1)"""
    blocks, n4, passes, tail = nonfinite_launch(n)
    places = {0, n - 1}
    if n4:
        places.add(4 * n4 - 1)
    places.update(range(4 * n4, n))
    if passes > 1:
        stride = blocks * NONFINITE_THREADS
        places.update(4 * v + k for v in (stride, stride + NONFINITE_THREADS) if v < n4 for k in (0, 3))
    return sorted(places)


# ---- mfcc_dct_kernel: launch_mfcc_dct restated --------------------------------------------------------------------
MFCC_DCT_LDS = 159 * 1024
MFCC_DCT_MAX_BLOCKS = 256


def mfcc_dct_launch(num_bins, num_ceps, use_energy, total_frames):
    """(waves per workgroup, frames per workgroup, workgroups, largest number of 64-frame tiles one wave takes)"""
    in_cols = num_bins + (1 if use_energy else 0)
    in_pitch = in_cols | 1
    ceps16 = (num_ceps + 15) & ~15
    dt_bytes = 4 * (((num_bins * ceps16 + 3) & ~3) + ceps16)
    tile_bytes = 4 * 64 * (in_pitch + 17)
    n_waves = min((MFCC_DCT_LDS - dt_bytes) // tile_bytes, 16)
    tiles = (total_frames + 63) // 64
    blocks = min((tiles + n_waves - 1) // n_waves, MFCC_DCT_MAX_BLOCKS)
    per_wave = (tiles + blocks * n_waves - 1) // (blocks * n_waves)
    return n_waves, 64 * n_waves, blocks, per_wave


MFCC_UTT_FRAMES = 77          # one utterance of the first batches: 64 + 13 frames at the default shift of 160 samples
MFCC_UTT_SAMPLES = 400 + (MFCC_UTT_FRAMES - 1) * 160
# (MfccProcessor options, copies of the utterance): batches just past ONE workgroup's frames
MFCC_FIRST = [
    (dict(num_bins=40, num_ceps=40), 9),
    (dict(num_bins=40, num_ceps=40, use_energy=False), 9),
    (dict(num_bins=40, num_ceps=40, cepstral_lifter=0.0), 9),
    (dict(num_bins=40, num_ceps=17, htk_compat=True), 9),
    (dict(num_bins=40, num_ceps=24, htk_compat=True, use_energy=False), 9),
    (dict(num_bins=40, num_ceps=33, htk_compat=True), 9),
    (dict(num_bins=40, num_ceps=33, htk_compat=True, use_energy=False, cepstral_lifter=0.0), 9),
    (dict(num_bins=80, num_ceps=40), 5),
    (dict(num_bins=80, num_ceps=40, htk_compat=True, use_energy=False), 5),
]
# the batch past 256 workgroups: 80 bins, 40 cepstra (5 waves: 256 x 5 x 64 = 81 920 frames in one pass); a frame
# shift of 32 samples keeps the audio at 26 640 samples per utterance
MFCC_BIG = (dict(num_bins=80, num_ceps=40, frame_shift=0.002), 101)
MFCC_BIG_FRAMES = 821
# synth.utterances ids of the two utterances.  The float32 oracle is a coarse judge of 80-bin cepstra: a narrow low
# mel bin on a spectral null carries a float32 error that the lifter (up to 12 x) amplifies, and on most 821-frame
# utterances the ORACLE is further from the float64 statement than the family tolerance allows the device to be
# from the oracle.  The big utterance is the one of MFCC_BIG_CANDIDATES on which the oracle is closest to the
# float64 statement - a choice that looks at the reference alone (test_post_remaining.py recomputes it).
MFCC_UTT_ID = 500
MFCC_BIG_CANDIDATES = range(501, 521)
MFCC_BIG_ID = 512
MFCC_BIG_SAMPLES = 400 + (MFCC_BIG_FRAMES - 1) * 32


def mfcc_id(case):
    opts, copies = case
    return '-'.join(f'{k}{v}' for k, v in opts.items()) + f'-x{copies}'


def mfcc_energy(opts):
    return bool(opts.get('use_energy', True))


def fbank_options(opts):
    """the options of the FilterbankProcessor whose rows an MFCC plan's scratch holds: [log energy |] log-mel"""
    keep = {k: v for k, v in opts.items() if k not in ('num_ceps', 'cepstral_lifter', 'htk_compat', 'use_energy')}
    return dict(keep, use_energy=mfcc_energy(opts), htk_compat=False, use_log_fbank=True, use_power=True)
