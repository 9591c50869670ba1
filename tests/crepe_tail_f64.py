"""Float64 numpy statement of the tail of the CREPE path between the decoder and the Kaldi post-processing, and
the cases the CPU and the GPU tests of it share.

Row resampling: `resample_rows` is scipy.signal.resample for real input written as the direct sum
    y[m] = (1 / N) sum_n x[n] D(m, n),   D = 1 + 2 sum_{k = 1..K} cos(k theta) + c cos((L / 2) theta),
with L = min(N, M), K = (L - 1) // 2, theta(m, n) = 2 pi (m / M - n / N) and c = 0 for odd L, 2 for even L when
M < N, 1 for even L when M > N; M == N returns the input.  Every angle is a fraction of a turn reduced in integers,
(k (m N - n M)) mod (M N) over M N, before the cosine sees it.  The cost is N M K cosines: for small cases only.

The conversion (voicing, interpolation, POV -> NCCF) has its statement in the package already: the host functions
`predict_voicing`, `pov_to_nccf` and `CrepePitchPostProcessor._convert`."""

import numpy as np

# (N, M) of the row resampling: down and up by a few rows at the sizes of a 3 s utterance, even and odd on either
# side, tiny ones, one row in, one row out, equal counts
PAIRS = [(301, 298), (298, 301), (300, 298), (301, 300), (7, 4), (4, 7), (5, 3), (2, 1), (1, 3), (6, 6)]
LONG_PAIR = (4099, 37)   # N > 4096 at a cost the direct sum can pay (K = 18)


def kernel(N, M):
    """D [M, N] of the statement (None when M == N)"""
    if M == N:
        return None
    L = min(N, M)
    K = (L - 1) // 2
    c = 0 if L % 2 else (2 if M < N else 1)
    MN = M * N
    r = (np.arange(M, dtype=np.int64)[:, None] * N - np.arange(N, dtype=np.int64)[None, :] * M) % MN
    D = np.ones((M, N))
    for k in range(1, K + 1):
        D += 2 * np.cos(2 * np.pi * (((k * r) % MN) / MN))
    if c:
        # (L / 2) theta = 2 pi (L r / 2) / MN: L is even here
        D += c * np.cos(2 * np.pi * ((((L // 2) * r) % MN) / MN))
    return D


def resample_rows(x, M):
    """The statement for the columns of `x` [N, columns]"""
    x = np.asarray(x, dtype=np.float64)
    D = kernel(x.shape[0], M)
    return x.copy() if D is None else D @ x / x.shape[0]


def clamp(rows):
    """The reference's clamp of column 0 (pitch_crepe.py:485-487), on a copy"""
    rows = np.array(rows, dtype=np.float64)
    rows[rows[:, 0] < 1e-2, 0] = 0
    rows[rows[:, 0] > 1, 0] = 1
    return rows


def decoder_like_rows(N, seed, swing=0.6):
    """(confidence, Hertz) rows like the decoder's: a confidence that moves slowly around 0.5 by `swing` - the
    default takes it below 1e-2 and above 1, so that the clamp has rows to act on - and a pitch around 200 Hz"""
    rng = np.random.RandomState(seed)
    t = np.arange(N)
    conf = 0.5 + swing * np.sin(2 * np.pi * (t / max(N, 8)) * (1 + rng.rand()) + rng.rand()) + 0.05 * (rng.rand(N) - 0.5)
    hertz = 200 + 50 * np.sin(2 * np.pi * t / max(N, 8) * 3 + rng.rand()) + rng.rand(N)
    return np.stack([conf, hertz], axis=1)
