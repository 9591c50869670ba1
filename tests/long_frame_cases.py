"""Batches and a host mirror of the grid-stride walk of the two long-frame kernels (fbank1024x2_kernel: two
frames of 513 ... 1024 samples per wave; fbank2048_kernel: one frame of 1026 ... 2048 samples per wave), shared
by tests/test_long_frame_cases.py (CPU: where every feature of a batch lies), tests/test_long_frames_seams_gpu.py
and tools/long_frames_errors.py.

Both kernels are persistent: a wave walks the pair table (the frame table) with a stride of 4096, and its
software pipeline hands state from one trip of that walk to the next.  A batch of `multi_trip_batch` makes
every wave take two or three trips and puts each thing that the hand-over could get wrong - another utterance,
another warp, a single frame, a pair that is split and replayed, a reflected frame in the replay - on trip 1
and again on trip 2."""

import functools

import numpy as np

from oracle import spec_f64
from shennong_amd import _backend, synth

# shennong_amd/csrc/kernels_fbank1024x2.hip launch_fbank1024x2 and kernels_fbank2048.hip launch_fbank2048:
# `if (blocks > 256) blocks = 256;` (blocks = ceil(units / kLongWaves)); device_fft1024.h: `constexpr int
# kLongWaves = 16;`; both kernels: `stride = gridDim.x * kLongWaves`, `g = blockIdx.x * kLongWaves + wid`
MAX_BLOCKS = 256
LONG_WAVES = 16
STRIDE = MAX_BLOCKS * LONG_WAVES
SPLIT_RATIO = 8.0             # kernels_fbank1024x2.hip kSplitRatio: `split = hi > split_ratio * lo`
RATIO_MARGIN = (4.0, 16.0)    # no pair of a batch lies in here: float32 energies cannot move one across 8
WARPS = (0.9, 1.0, 1.15)
FRAME_SHIFT, FRAME_LENGTH = 0.01, 0.025   # the processors' defaults


def geometry(sample_rate, frame_length=FRAME_LENGTH, frame_shift=FRAME_SHIFT):
    """(shift, win_len, padded) in samples, Kaldi's rounding"""
    return spec_f64.frame_geometry(sample_rate, frame_shift, frame_length)


def unit_of(sample_rate):
    """what a wave of the kernel of this rate takes per trip: 'pairs' (fbank1024x2_kernel) or 'frames'"""
    padded = geometry(sample_rate)[2]
    assert padded in (1024, 2048), padded
    return 'pairs' if padded == 1024 else 'frames'


def frame_counts(waves, sample_rate, snip_edges):
    shift, length, _ = geometry(sample_rate)
    return np.array([spec_f64.num_frames(len(w), shift, length, snip_edges) for w in waves], dtype=np.int64)


def left_out(waves, sample_rate, snip_edges):
    """capi_mel.hip route_mel_batch, short_mask: with snip_edges = False an utterance shorter than a window
    runs on the generic kernel behind the long-frame one and has no pairs"""
    length = geometry(sample_rate)[1]
    return np.array([(not snip_edges) and 0 < len(w) < length for w in waves], dtype=bool)


def pair_table(counts, skipped=None):
    """Mirror of prepare_mel_tables / build_pair_table_kernel: utterance u owns (n_u + 1) // 2 pairs, in
    order; pair m of u holds frames 2 m and 2 m + 1, an odd last frame sits alone.
    -> (utt [P], frame_a [P] (row of the batch), has_b [P])"""
    counts = np.asarray(counts, dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(counts)])
    utt, frame_a, has_b = [], [], []
    for u, n in enumerate(counts.tolist()):
        if skipped is not None and skipped[u]:
            continue
        for m in range((n + 1) // 2):
            utt.append(u)
            frame_a.append(first[u] + 2 * m)
            has_b.append(2 * m + 1 < n)
    return np.array(utt, dtype=np.int64), np.array(frame_a, dtype=np.int64), np.array(has_b, dtype=bool)


def frame_table(counts):
    """-> utt [T]: the frame table of fbank2048_kernel (build_frame_start_kernel: every frame, in order)"""
    return np.repeat(np.arange(len(counts)), np.asarray(counts, dtype=np.int64))


def stride_of(n_units):
    """the stride of the walk over `n_units` pairs (frames): the launchers' grid times kLongWaves"""
    return min(MAX_BLOCKS, -(-int(n_units) // LONG_WAVES)) * LONG_WAVES


def trip_of(index, n_units):
    """trip of the loop on which some wave takes pair (frame) `index`; the wave is index % stride.  (A split
    pair takes two turns of the loop on the same trip of the walk: `g` does not advance.)"""
    return np.asarray(index) // stride_of(n_units)


def unit_table(waves, sample_rate, snip_edges):
    """-> (utt [N] of every pair / frame the long-frame kernel walks, first row [N] of the batch it writes)"""
    counts = frame_counts(waves, sample_rate, snip_edges)
    if unit_of(sample_rate) == 'pairs':
        utt, frame_a, _ = pair_table(counts, left_out(waves, sample_rate, snip_edges))
        return utt, frame_a
    return frame_table(counts), np.arange(int(counts.sum()))


def row_trips(waves, sample_rate, snip_edges):
    """trip [total_frames] of every row of the batch's output (-1: written by the generic kernel)"""
    counts = frame_counts(waves, sample_rate, snip_edges)
    trips = np.full(int(counts.sum()), -1, dtype=np.int64)
    utt, row = unit_table(waves, sample_rate, snip_edges)
    trip = trip_of(np.arange(len(utt)), len(utt))
    trips[row] = trip
    if unit_of(sample_rate) == 'pairs':
        has_b = pair_table(counts, left_out(waves, sample_rate, snip_edges))[2]
        trips[row[has_b] + 1] = trip[has_b]
    else:
        # (fbank2048_kernel walks every frame; the rows of an utterance shorter than a window are written again
        # by the masked generic launch behind it)
        first = np.concatenate([[0], np.cumsum(counts)])
        for u in np.nonzero(left_out(waves, sample_rate, snip_edges))[0]:
            trips[first[u]:first[u + 1]] = -1
    return trips


# ---- the split decision, predicted from the oracle's framing ---------------------------------------------
def windowed_energies(wave, sample_rate, snip_edges):
    """float64 energy of every windowed frame (DC removal, pre-emphasis 0.97, Povey window: the processors'
    defaults) from the float64 restatement of the oracle's framing (oracle/spec_f64.py)"""
    shift, length, _ = geometry(sample_rate)
    x = spec_f64.extract_frames(wave, shift, length, snip_edges)
    if x.shape[0] == 0:
        return np.zeros(0)
    x = x - x.mean(axis=1, keepdims=True)
    y = x.copy()
    y[:, 1:] = x[:, 1:] - 0.97 * x[:, :-1]
    y[:, 0] = x[:, 0] - 0.97 * x[:, 0]
    y = y * spec_f64.window_function(length, 'povey')[None, :]
    return (y * y).sum(axis=1)


def pair_ratios(wave, sample_rate, snip_edges):
    """hi / lo of the windowed energies of every whole pair of the utterance (1 for two silent frames, inf for
    silence beside anything; an odd last frame has no ratio)"""
    e = windowed_energies(wave, sample_rate, snip_edges)
    a, b = e[0:len(e) - len(e) % 2:2], e[1::2]
    hi, lo = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(hi == 0, 1.0, np.where(lo == 0, np.inf, hi / np.where(lo == 0, 1.0, lo)))


def in_margin(ratios):
    return (ratios >= RATIO_MARGIN[0]) & (ratios <= RATIO_MARGIN[1])


def split_pairs(waves, sample_rate, snip_edges):
    """-> (split [P] over the pair table of the batch, ratio [P] (1 for a single frame))"""
    counts = frame_counts(waves, sample_rate, snip_edges)
    skipped = left_out(waves, sample_rate, snip_edges)
    ratio = []
    for u, w in enumerate(waves):
        if skipped[u]:
            continue
        r = pair_ratios(w, sample_rate, snip_edges)
        ratio.append(r if counts[u] % 2 == 0 else np.concatenate([r, [1.0]]))
    ratio = np.concatenate(ratio)
    return ratio > SPLIT_RATIO, ratio


# ---- signals ------------------------------------------------------------------------------------------
def samples_for(frames, sample_rate, snip_edges, extra=0):
    """a length of `frames` frames; `extra` < shift more samples leave the count alone"""
    shift, length, _ = geometry(sample_rate)
    assert 0 <= extra < shift and frames >= 1
    n = length + (frames - 1) * shift + extra if snip_edges else frames * shift - shift // 2 + extra
    assert spec_f64.num_frames(n, shift, length, snip_edges) == frames
    return n


def _tone(rng, n, sample_rate):
    # (a tone over a noise floor 20 dB below it, as test_paired_frames_of_unequal_energy)
    t = np.arange(n) / sample_rate
    return (20000 * np.sin(2 * np.pi * 997.0 * t) + rng.integers(-3000, 3001, size=n)).astype(np.int16)


def unequal_energy_signal(kind, sample_rate, snip_edges, seed):
    """The quiet-beside-loud signals of test_paired_frames_of_unequal_energy (0: digital silence inside a tone,
    1: a +-1 LSB murmur, 2: +-30, 3: silence, then full-scale noise), one second each.  The edges of the quiet
    stretch move by up to two frame shifts, to the first place at which no pair of the utterance has an energy
    ratio inside RATIO_MARGIN: which pairs split is then decided by the reference alone."""
    rng = np.random.default_rng(seed)
    n = sample_rate
    shift = geometry(sample_rate)[0]
    tone = _tone(rng, n, sample_rate)
    fill = [np.zeros(n, np.int16), rng.integers(-1, 2, size=n).astype(np.int16),
            rng.integers(-30, 31, size=n).astype(np.int16), rng.integers(-20000, 20000, size=n).astype(np.int16)][kind]
    moves = range(0, 2 * shift, max(shift // 4, 1))
    for da in moves:
        for db in (moves if kind < 3 else [0]):
            w = tone.copy()
            if kind < 3:
                quiet = slice(n // 4 + da, n // 2 + 137 * kind + db)
                w[quiet] = fill[quiet]
            else:
                w[:n // 3 + da] = 0
                w[n // 3 + da:] = fill[n // 3 + da:]
            ratios = pair_ratios(w, sample_rate, snip_edges)
            if not in_margin(ratios).any() and (ratios > SPLIT_RATIO).any():
                return w
    raise AssertionError('no placement of the quiet stretch keeps every pair out of the margin')


def split_tail_signal(frames, sample_rate, snip_edges, seed):
    """A tone whose last window is a +-300 murmur: `frames` is even, so the last pair splits and its frame b is
    the last frame of the utterance - with snip_edges = False a reflected one, whose samples are not those of
    the clamped window the replay's loads bring in.

    The murmur's level: 40 dB under the tone, a windowed energy 1000 times under that of the frame before it,
    and a strongest spectrogram bin near e^18.  Not +-30: its strongest bin is e^13.8 = 10^6, so the -60 dB line
    of conftest._spectrogram_close falls at a log power of 0, where the relative term of the bound vanishes and
    what is left, 1e-4 of the bin's power, is a tenth of the 1e-9 of the frame's peak that the same rule grants
    to a bin just under the line - the float32 floor of any transform, the oracle's included.  At e^18 the
    relative term there is 4.6e-4."""
    assert frames % 2 == 0
    shift, length, _ = geometry(sample_rate)
    rng = np.random.default_rng(seed)
    n = samples_for(frames, sample_rate, snip_edges)
    w = _tone(rng, n, sample_rate)
    start_b = (frames - 1) * shift + (0 if snip_edges else shift // 2 - length // 2)
    w[start_b:] = rng.integers(-300, 301, size=n - start_b)
    return w


def _synth(first_id, n, sample_rate):
    return synth.utterances(first_id, 1, n, sample_rate)[0]


def _feature_block(k, sample_rate, snip_edges, seed):
    """(label, wave, warp) of the utterances that every trip must see; block k of a batch"""
    s = 1000 * seed + 100 * k
    n_of = lambda frames, extra=0: samples_for(frames, sample_rate, snip_edges, extra)   # noqa: E731
    items = [
        ('even', _synth(s + 1, n_of(40, 3), sample_rate), 0.9),
        ('odd', _synth(s + 2, n_of(41, 7), sample_rate), 1.0),
        ('one_frame', _synth(s + 3, n_of(1, 5), sample_rate), 1.15),
        # (one whole window: the fewest frames of an utterance that stays on the long-frame kernel without
        # snip_edges, where it gives three)
        ('three_frames', _synth(s + 4, max(n_of(3), geometry(sample_rate)[1]), sample_rate), 1.0),
    ]
    for kind, warp in enumerate((1.0, 0.9, 1.15, 1.0)):
        items.append(('unequal%d' % kind, unequal_energy_signal(kind, sample_rate, snip_edges, s + 10 + kind), warp))
    items += [
        ('one_frame', _synth(s + 5, n_of(1), sample_rate), 0.9),
        ('split_tail', split_tail_signal(38, sample_rate, snip_edges, s + 20), 1.15),
        ('odd', _synth(s + 6, n_of(27, 1), sample_rate), 0.9),
    ]
    return items


@functools.lru_cache(maxsize=None)
def _batch(sample_rate, snip_edges, seed):
    unit = unit_of(sample_rate)
    shift, length, _ = geometry(sample_rate)
    rng = np.random.default_rng(7000 + seed)
    items = []

    def units():
        waves = [w for _, w, _ in items]
        return len(unit_table(waves, sample_rate, snip_edges)[0])

    def fill(until):
        lo, hi = (60, 140) if unit == 'pairs' else (30, 90)
        count = units()
        while count < until:
            frames = int(rng.integers(lo, hi + 1))
            n = samples_for(frames, sample_rate, snip_edges, int(rng.integers(0, shift)))
            items.append(('filler', _synth(10000 * seed + len(items), n, sample_rate), WARPS[len(items) % 3]))
            count += (frames + 1) // 2 if unit == 'pairs' else frames
    for k, start in enumerate((0, STRIDE + 40, 2 * STRIDE + 40)):
        fill(start)
        items += _feature_block(k, sample_rate, snip_edges, seed)
    fill(2 * STRIDE + 1300)
    # the last pair of the table is a single frame, and the total is no multiple of kLongWaves
    frames = 33
    while True:
        last = ('last_odd', _synth(10000 * seed + 9999, samples_for(frames, sample_rate, snip_edges), sample_rate), 1.0)
        items.append(last)
        if units() % LONG_WAVES != 0:
            break
        items.pop()
        frames += 2
    labels = tuple(label for label, _, _ in items)
    waves = [w for _, w, _ in items]
    warps = [warp for _, _, warp in items]
    for w in waves:
        w.setflags(write=False)
    return labels, waves, warps


def multi_trip_batch(sample_rate, snip_edges, seed=0):
    """-> (waves, warps): ragged utterances whose pairs (22.05 / 32 kHz) or frames (44.1 kHz) number between
    2 x 4096 and 3 x 4096 and no multiple of 16, under _backend._LARGE_BATCH_BYTES of audio (one launch); the
    feature block (`batch_labels`) lies at the start, behind index 4096 and behind index 8192"""
    _, waves, warps = _batch(sample_rate, bool(snip_edges), seed)
    assert 2 * sum(len(w) for w in waves) < _backend._LARGE_BATCH_BYTES
    return list(waves), list(warps)


def batch_labels(sample_rate, snip_edges, seed=0):
    """what each utterance of `multi_trip_batch` is there for: 'filler', or a name of the feature block"""
    return _batch(sample_rate, bool(snip_edges), seed)[0]


FEATURES = ('even', 'odd', 'one_frame', 'three_frames', 'unequal0', 'unequal1', 'unequal2', 'unequal3',
            'split_tail')
# the multi-trip cases of the GPU tests: (kernel, sample rate, window, NJ)
MULTI_TRIP_CASES = (('fbank1024x2_kernel', 22050, 551, 9), ('fbank1024x2_kernel', 32000, 800, 13),
                    ('fbank2048_kernel', 44100, 1102, 9))


def probes(sample_rate, snip_edges, seed=0):
    """indices of about eight utterances of the later feature blocks: the split ones, one-frame ones, warped
    ones"""
    labels = batch_labels(sample_rate, snip_edges, seed)
    picked = []
    for name in ('unequal0', 'unequal3', 'split_tail', 'one_frame', 'even', 'odd'):
        where = [i for i, label in enumerate(labels) if label == name]
        picked.append(where[len(where) // 3])        # (block 1; of the two one-frame / odd ones per block, its first)
    for name in ('unequal1', 'split_tail', 'three_frames'):
        picked.append([i for i, label in enumerate(labels) if label == name][-1])   # (block 2)
    return picked


def rotated(seq, by):
    return list(seq[by:]) + list(seq[:by])


# ---- window and bank seams -------------------------------------------------------------------------------
SEAM_RATE = 16000


def window_cases():
    """win_len of part 3, by kernel.  fbank1024x2_kernel: the smallest window, the last with n_full = 64 whole
    16-byte pieces, the first with more, both sides of NJ 9 -> 13 (rows = ceil(win_len / 64)) and 13 -> 16, the
    largest odd and the largest window (tails of win_len mod 8 = 1, 7, 0, 0, 1, 0, 1, 7, 0 samples).
    fbank2048_kernel: the smallest, both sides of NJ 9 -> 10 (rows = ceil(win_len / 128)) and 10 -> 16, the
    largest two.  An odd window of that size runs on the generic kernel."""
    return {'fbank1024x2_kernel': (513, 519, 520, 576, 577, 832, 833, 1023, 1024),
            'fbank2048_kernel': (1026, 1152, 1154, 1280, 1282, 2046, 2048),
            'mel_features_generic_kernel': (1027,)}


def expected_nj(kernel, win_len):
    if kernel == 'fbank1024x2_kernel':
        rows = -(-win_len // 64)
        return 9 if rows <= 9 else 13 if rows <= 13 else 16
    rows = -(-win_len // 128)
    return 9 if rows <= 9 else 10 if rows <= 10 else 16


BANK_BINS = (3, 8, 9, 80, 121, 128)     # a round with idle teams, one round, one round + 1 bin, ..., the limit
BANK_WINDOWS = {'fbank1024x2_kernel': 800, 'fbank2048_kernel': 1600}


def frame_length_for(win_len, sample_rate=SEAM_RATE):
    """a frame_length in seconds that Kaldi's float32 milliseconds round to exactly `win_len` samples"""
    return (win_len + 0.5) / sample_rate


def seam_batch(win_len, snip_edges, sample_rate=SEAM_RATE, seed=0):
    """three utterances of 35, 36 and 1 frames (snip_edges = False: the last one is shorter than a window and
    takes the generic kernel) with the three warps"""
    shift = geometry(sample_rate, frame_length_for(win_len, sample_rate))[0]
    waves = []
    for i, (frames, extra) in enumerate(((35, 3), (36, 0), (1, 1))):
        n = win_len + (frames - 1) * shift + extra if snip_edges else frames * shift - shift // 2 + extra
        waves.append(_synth(500 + 10 * seed + i, n, sample_rate))
    return waves, list(WARPS)
