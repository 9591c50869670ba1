"""Data and float64 answers shared by the alignment tests (tests/test_dtw_align.py, tests/test_dtw_align_gpu.py) and by
tools/time_dtw_align.py, on top of tests/dtw_cases.py, tests/dtw_search_cases.py and tests/dtw_detect_cases.py: the
statement (tests/dtw_align_f64.py) of every pair of a case, computed once per case."""

import functools

import numpy as np

import dtw_align_f64
import dtw_cases
import dtw_detect_cases
import dtw_detect_f64
import dtw_search_cases
import dtw_search_f64

EXACT_DIMS = (1, 3, 13)
SEARCH_DIMS = (1, 3)
MIN_DECIDED_PAIRS = 50    # of the 100 pairs of a cosine case: every decision on the path leads by more than the bound


class GlobalAnswer:
    """The statement of one pair of the global lattice: d, C, its end cell, the path and its smallest lead"""

    def __init__(self, x, y, metric, gaps=False):
        self.d = dtw_align_f64.frame_distances(x, y, metric)
        C, L, K = dtw_align_f64.global_tables(self.d)
        self.shape = self.d.shape
        self.cost, self.length = float(C[-1, -1]), int(L[-1, -1])
        self.path = dtw_align_f64.traceback(K)
        self.gap = dtw_align_f64.path_gap(C, K) if gaps else None


def global_statement(xs, ys, metric, gaps=False):
    """The GlobalAnswers of every x against every y, in the order of dtw_cases.two_set_collection"""
    return [GlobalAnswer(x, y, metric, gaps) for x in xs for y in ys]


@functools.lru_cache(maxsize=None)
def exact_case(dim):
    xs, ys, _ = dtw_cases.exact_case(dim)
    return xs, ys, global_statement(xs, ys, 'sqeuclidean')


@functools.lru_cache(maxsize=None)
def cosine_case(dim):
    xs, ys, _ = dtw_cases.cosine_case(dim)
    return xs, ys, global_statement(xs, ys, 'cosine', gaps=True)


def path_bound(dim, n, m):
    """What the float64 cost along a path of the float32 lattice may exceed the float64 optimum by, and the lead
    that every decision of the float64 path needs for the float32 lattice to take the same: rounding to float32 is
    monotone, so the device's table is the minimum over paths of float32-evaluated costs, each within
    (n + m) cosine_bound of its float64 value (cosine_bound bounds the error of the cost over the length, a length
    is below n + m) - twice that between two paths"""
    return 2 * (n + m) * dtw_cases.cosine_bound(dim, n, m)


def cost_along(d, path):
    """The float64 sum of d over the cells of `path`, in the order of the path"""
    path = np.asarray(path)
    return float(np.cumsum(d[path[:, 0], path[:, 1]])[-1])


@functools.lru_cache(maxsize=None)
def long_case(n, m, seed, dim=3):
    """(x [n, dim], y [m, dim], path of x against y, path of y against x): integer rows, sqeuclidean"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
    y = rng.integers(-2, 3, size=(m, dim)).astype(np.float32)
    d = dtw_align_f64.frame_distances(x, y, 'sqeuclidean')
    made, turned = dtw_align_f64.global_tables(d), dtw_align_f64.global_tables(d.T)
    assert made[0].max() < 2 ** 24 and turned[0].max() < 2 ** 24   # (every float32 sum is exact)
    return x, y, (made[0][-1, -1], dtw_align_f64.traceback(made[2])), (turned[0][-1, -1],
                                                                      dtw_align_f64.traceback(turned[2]))


class SubAnswer:
    """The statement of one (query, target) pair of the subsequence lattice: the last rows and K"""

    def __init__(self, x, y, metric):
        d = dtw_align_f64.frame_distances(x, y, metric)
        C, L, B, self.K = dtw_align_f64.sub_tables(d)
        self.shape = d.shape
        self.cost, self.length, self.start = C[-1].copy(), L[-1].copy(), B[-1].copy()

    def best(self, normalized, dtype=np.float32):
        return dtw_search_f64.best_end(self.cost, self.length, self.start, normalized, dtype)

    def detections(self, k, normalized=True, max_score=None, dtype=np.float32):
        return dtw_detect_f64.detections(self.cost, self.length, self.start, k, normalized, max_score, dtype)

    def path(self, end):
        return dtw_align_f64.traceback(self.K, end)


@functools.lru_cache(maxsize=None)
def search_case(dim):
    """The integer case of tests/dtw_search_cases.py with the decisions kept: (xs, ys, SubAnswers)"""
    xs, ys, _ = dtw_search_cases.exact_case(dim)
    return xs, ys, [SubAnswer(x, y, 'sqeuclidean') for x in xs for y in ys]


@functools.lru_cache(maxsize=None)
def planted_case():
    """A query planted in a target between rows of 9s: (query, target, SubAnswer)"""
    query, target = dtw_search_cases.planted(37, 70, 45, 3, seed=5)
    return query, target, SubAnswer(query, target, 'sqeuclidean')


@functools.lru_cache(maxsize=None)
def detect_case():
    """(query, [target], [SubAnswer]): the three targets of tests/dtw_detect_cases.py, three planted copies of the one
    query in each"""
    targets = []
    for gaps in dtw_detect_cases.PLANTED_GAPS:
        query, target, _ = dtw_detect_cases.planted_three(gaps, seed=11)
        targets.append(target)
    return query, targets, [SubAnswer(query, target, 'sqeuclidean') for target in targets]
