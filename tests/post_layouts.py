"""Batch layouts for the route tests of the delta, pitch-post and CMVN kernels (test_post_routes.py and
test_post_routes_gpu.py): lists of utterance lengths whose concatenation, cut into tiles of R rows, puts an
utterance boundary on every kind of tile seam.  The tile heights are restated here, not read from the source:
a change of kernels_post.hip that moves a seam has to be made here too, and `check_seams` then says what the
layouts no longer reach."""

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
    lengths = [0, 1, 2, 3, 1, 1, 1, 0, 1, 1, 1]              # 12 rows
    lengths += [rows - 3 - 12, 2, 3, 2]                      # ends rows-3, rows-1, rows+2, rows+4
    lengths += [4 * rows - (rows + 4)]                       # ... 4 rows: exactly on the seam
    lengths += [rows - 4, 2, 3, 2]                           # ends 5 rows -4, -2, +1, +3
    tail = (rows // 2) & ~1                                  # 3 + tail rows in the last tile: odd
    lengths += [tail, 0]
    return check_seams(lengths, rows)


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
    r = max(1, 256 // cols)
    return [0, 1, r - 1, r, r + 1, 1000]
