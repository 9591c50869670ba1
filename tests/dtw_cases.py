"""Data and float64 answers shared by the DTW tests (tests/test_dtw.py, tests/test_dtw_gpu.py) and by
tools/dtw_errors.py: the item lengths that sit on every seam of the kernel, the two item sets of a case, their
statement (tests/dtw_f64.py), computed once per case, and the derived error bounds."""

import functools

import numpy as np

import dtw_f64
from shennong_amd.features import Features, FeaturesCollection

# around the tile of 32 columns and the strip of 64 rows, more than one strip, more than one ring of 3 tiles
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 129, 200)
EXACT_DIMS = (1, 2, 3, 13, 40)
COSINE_DIMS = (7, 13, 39, 40, 80)
# per dim, the first seed (searched on the CPU, `python tests/dtw_cases.py`) at which all 100 pairs of the
# statement keep max |cos| <= MAX_COS and path_margin >= MIN_MARGIN
COSINE_SEEDS = {7: 0, 13: 0, 39: 0, 40: 0, 80: 0}
MAX_COS = 0.99
MIN_MARGIN = 2e-4
EPS = 2.0 ** -24


def features(data, shift=0.01, length=0.025):
    """`data` as Features with [n, 2] times of a 25 ms window every 10 ms"""
    start = shift * np.arange(data.shape[0], dtype=np.float64)
    return Features(np.ascontiguousarray(data, dtype=np.float32), np.stack([start, start + length], axis=1),
                    properties={}, validate=False)


def collection(mats, prefix='item'):
    return FeaturesCollection(('{}{}'.format(prefix, k), features(m)) for k, m in enumerate(mats))


def item_sets(kind, dim, seed):
    """Two independent sets of items, one per length of LENGTHS: `kind` 'int' (integers in [-2, 2]: every
    squared distance and every sum of them is an exact float32 integer, ties abound) or 'normal'"""
    rng = np.random.default_rng(seed)
    if kind == 'int':
        make = lambda n: rng.integers(-2, 3, size=(n, dim)).astype(np.float32)   # noqa: E731
    else:
        make = lambda n: rng.standard_normal((n, dim)).astype(np.float32)        # noqa: E731
    return [make(n) for n in LENGTHS], [make(n) for n in LENGTHS]


def two_set_collection(xs, ys):
    """(collection, the 100 ordered pairs of names: every x against every y)"""
    both = collection(xs, 'x')
    both.update(collection(ys, 'y'))
    pairs = [('x{}'.format(a), 'y{}'.format(b)) for a in range(len(xs)) for b in range(len(ys))]
    return both, pairs


def statement(xs, ys, metric, margins=True):
    """cost [P], length [P], path_margin [P], max |cos| [P] of every x against every y (float64)"""
    cost, length, margin, cosine = [], [], [], []
    for x in xs:
        for y in ys:
            d = dtw_f64.frame_distances(x, y, metric)
            C, L = dtw_f64.tables(d)
            cost.append(C[-1, -1])
            length.append(L[-1, -1])
            margin.append(dtw_f64.path_margin(d, (C, L)) if margins else np.nan)
            # (of nonzero rows d = arccos(cos) / pi)
            cosine.append(np.abs(np.cos(np.pi * d)).max() if metric == 'cosine' else np.nan)
    return (np.array(cost), np.array(length, dtype=np.int64), np.array(margin), np.array(cosine))


@functools.lru_cache(maxsize=None)
def exact_case(dim):
    xs, ys = item_sets('int', dim, seed=100 + dim)
    return xs, ys, statement(xs, ys, 'sqeuclidean')


@functools.lru_cache(maxsize=None)
def cosine_case(dim):
    xs, ys = item_sets('normal', dim, seed=COSINE_SEEDS[dim])
    return xs, ys, statement(xs, ys, 'cosine')


def pair_shapes():
    """(N, M) of the 100 pairs, in the order of `statement`"""
    return np.array([(n, m) for n in LENGTHS for m in LENGTHS], dtype=np.int64)


def cosine_bound(dim, n, m):
    """Bound on the error of the normalised cosine DTW distance in float32, for |cos| <= MAX_COS and equal
    paths: the round-off of the dot product and of the normalisation ((dim + 4) eps) through the slope of
    arccos / pi at MAX_COS, the error of acosf and of the product with 1 / pi (4 eps on a value <= 1), and the
    float32 accumulation of n + m values whose mean stays <= 1 ((n + m) eps).  Derived, not measured."""
    return ((dim + 4) / (np.pi * np.sqrt(1 - MAX_COS ** 2)) + 4 + (n + m)) * EPS


def sqeuclidean_bound(dim, n, m, scale, result):
    """Bound on the error of a float32 sqeuclidean DTW cost computed as |x|^2 + |y|^2 - 2 x.y: `scale` the
    largest |x_i|^2 + |y_j|^2 of the pair, `result` the cost itself"""
    return (dim + 4) * 2.0 ** -23 * scale + (n + m) * EPS * result


if __name__ == '__main__':   # the seed search behind COSINE_SEEDS
    for dim in COSINE_DIMS:
        for seed in range(1000):
            xs, ys = item_sets('normal', dim, seed)
            # (the cheap condition first)
            worst = max(np.abs(np.cos(np.pi * dtw_f64.frame_distances(x, y))).max() for x in xs for y in ys)
            if worst > MAX_COS:
                continue
            _, _, margin, cosine = statement(xs, ys, 'cosine')
            if margin.min() >= MIN_MARGIN:
                print(dim, seed, 'min margin %.3g max |cos| %.4f' % (margin.min(), cosine.max()), flush=True)
                break
