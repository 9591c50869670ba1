"""The float64 statement of the symmetric-KL frame distance of snf_dtw_pairs (metric 'symkl')

For the rows x_i of x [N, D] and y_j of y [M, D] (float32 values, taken to float64):

    FLOOR = 2^-40                      (SNF_DTW_SYMKL_FLOOR; exact in float32)
    x~ = max(x, FLOOR) element-wise    (zero and negative entries count as FLOOR; rows need not sum to 1)
    d[i, j] = 0.5 * sum_k (x~_ik - y~_jk) (ln x~_ik - ln y~_jk)     natural logarithm; every term >= 0

The recursion, the tie rule, cost, length and the normalisation are those of tests/dtw_f64.py (`tables`,
`path_margin`), unchanged.  `magnitudes` is the sum of absolute values that the derived error bound of the float32
kernel scales with (tests/symkl_cases.py)."""

import numpy as np

import dtw_f64

FLOOR = 2.0 ** -40


def floored(x):
    """x~ in float64 of float32 rows"""
    return np.maximum(np.asarray(x, dtype=np.float32).astype(np.float64), FLOOR)


def frame_distances(x, y):
    """d [N, M] in float64, the definition term by term"""
    x, y = floored(x), floored(y)
    lx, ly = np.log(x), np.log(y)
    # (256 rows of x at a time: the terms of a 4096-frame item would not fit at once)
    return np.concatenate([0.5 * ((x[a:a + 256, None, :] - y[None, :, :]) *
                                  (lx[a:a + 256, None, :] - ly[None, :, :])).sum(axis=2)
                           for a in range(0, x.shape[0], 256)], axis=0)


def frame_distances_loop(x, y):
    """The same by the plain triple loop, the terms added over k ascending"""
    x, y = floored(x), floored(y)
    d = np.zeros((x.shape[0], y.shape[0]), dtype=np.float64)
    for i in range(x.shape[0]):
        for j in range(y.shape[0]):
            total = 0.0
            for k in range(x.shape[1]):
                total += (x[i, k] - y[j, k]) * (np.log(x[i, k]) - np.log(y[j, k]))
            d[i, j] = 0.5 * total
    return d


def magnitudes(x, y):
    """A [N, M] = sum_k (|x~ ln x~| + |y~ ln y~| + x~ |ln y~| + |ln x~| y~): what the four sums of the kernel's
    form (h(x_i) + h(y_j) - x~_i . ln y~_j - ln x~_i . y~_j) add up in absolute value"""
    x, y = floored(x), floored(y)
    lx, ly = np.abs(np.log(x)), np.abs(np.log(y))
    return (x * lx).sum(axis=1)[:, None] + (y * ly).sum(axis=1)[None, :] + x @ ly.T + lx @ y.T


def dtw(x, y, normalized=True):
    """(distance, length) of the pair, float64 and int"""
    C, L = dtw_f64.tables(frame_distances(x, y))
    cost, length = float(C[-1, -1]), int(L[-1, -1])
    return (cost / length if normalized else cost), length
