"""Data, float64 answers and derived error bounds shared by the symkl tests (tests/test_symkl.py,
tests/test_symkl_gpu.py, tests/test_posteriorgram_gpu.py) and by tools/symkl_errors.py

Items are rows of probabilities: the float32 of the softmax of ``2 * standard_normal``; in the *floored* kind a fifth
of the entries (never the largest of a row) are then set to 0, which the metric counts as its floor 2^-40.  The item
lengths are dtw_cases.LENGTHS: every seam of the kernel.

The bound of a pair's float32 cost.  With A[i, j] = sum_k (|x~ ln x~| + |y~ ln y~| + x~ |ln y~| + |ln x~| y~)
(symkl_f64.magnitudes) the kernel's frame distance 0.5 (h(x_i) + h(y_j) - x~_i . ln y~_j - ln x~_i . y~_j) is off by
at most (2 dim + 8) 2^-24 A[i, j] / 2: each of the two chains of dim fused multiply-adds that make h, and the one
chain of 2 dim that makes the two dot products, errs by (its length) 2^-24 times its sum of absolute values; logf is
within an ulp of the logarithm (2 2^-24 relative, on every term); the additions and the subtraction of the epilogue
add 3 2^-24 A; the halving is exact.  (2 dim + 8) 2^-24 max A is twice that and what the tests use.  A cost is a
minimum over paths, so it moves by at most the length of a path, at most N + M - 1 cells, times the largest frame
error, whichever path the kernel takes; adding N + M - 1 non-negative float32 values adds (N + M) 2^-24 cost:

    bound = (N + M - 1) (2 dim + 8) 2^-24 max A  +  (N + M) 2^-24 cost

A pair *qualifies* when the path margin of the statement (dtw_f64.path_margin) is at least 2 bound: no perturbation
within the bound, of either path, can change the length of the optimal path.  Derived, not measured."""

import functools

import numpy as np

import dtw_cases
import dtw_f64
import symkl_f64

LENGTHS = dtw_cases.LENGTHS
EPS = 2.0 ** -24
KINDS = ('plain', 'floored')
DIMS = (7, 8, 9, 40, 65)     # lengths are compared on the pairs that qualify, costs on all
COST_ONLY_DIMS = (2,)        # a one-parameter family full of near ties: 0.54 of the pairs qualify
SEED = 0
MIN_QUALIFYING = 90          # of the 100 pairs, for every dim of DIMS and both kinds (asserted on the statement)


def item_sets(kind, dim, seed=SEED):
    """Two sets of items, one per length of LENGTHS: the ten x items are drawn first, then the ten y items"""
    if kind not in KINDS:
        raise ValueError(kind)
    rng = np.random.default_rng(seed)

    def make(n):
        z = 2 * rng.standard_normal((n, dim))
        e = np.exp(z - z.max(axis=1, keepdims=True))
        p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        if kind == 'floored':
            mask = rng.random((n, dim)) < 0.2
            mask[np.arange(n), p.argmax(axis=1)] = False
            p[mask] = 0
        return p
    return [make(n) for n in LENGTHS], [make(n) for n in LENGTHS]


def bound(dim, n, m, max_a, cost):
    """The bound of the module's docstring (arrays or scalars)"""
    return (n + m - 1) * (2 * dim + 8) * EPS * max_a + (n + m) * EPS * cost


def pair_statement(x, y, margins=True):
    """(cost, length, path margin, max A, bound) of one pair, float64"""
    d = symkl_f64.frame_distances(x, y)
    C, L = dtw_f64.tables(d)
    cost, length = float(C[-1, -1]), int(L[-1, -1])
    margin = dtw_f64.path_margin(d, (C, L)) if margins else np.nan
    max_a = float(symkl_f64.magnitudes(x, y).max())
    return cost, length, margin, max_a, bound(x.shape[1], x.shape[0], y.shape[0], max_a, cost)


def statement(xs, ys, margins=True):
    """cost [P], length [P], path margin [P], max A [P], bound [P] of every x against every y (float64)"""
    rows = [pair_statement(x, y, margins) for x in xs for y in ys]
    cost, length, margin, max_a, limit = (np.array(column) for column in zip(*rows))
    return cost, length.astype(np.int64), margin, max_a, limit


@functools.lru_cache(maxsize=None)
def case(kind, dim):
    """(xs, ys, (cost, length, margin, max A, bound), qualifying [P] bool) of the 100 pairs; computed once"""
    xs, ys = item_sets(kind, dim)
    made = statement(xs, ys)
    return xs, ys, made, made[2] >= 2 * made[4]


def one_long_utterance(xs, ys):
    """The items as slices of one utterance: (collection of one utterance, items (name, onset, offset) in the order
    xs then ys, the integer pairs [100, 2] of every x against every y).  A slice is selected by the centre times of
    its rows (dtw_cases.features: a 25 ms window every 10 ms), with 5 ms to spare on both sides."""
    mats = list(xs) + list(ys)
    feats = dtw_cases.collection([np.concatenate(mats, axis=0)], 'long')
    items, row = [], 0
    for m in mats:
        items.append(('long0', 0.01 * row + 0.0125 - 0.005, 0.01 * (row + m.shape[0] - 1) + 0.0125 + 0.005))
        row += m.shape[0]
    pairs = np.array([(a, len(xs) + b) for a in range(len(xs)) for b in range(len(ys))], dtype=np.int64)
    return feats, items, pairs
