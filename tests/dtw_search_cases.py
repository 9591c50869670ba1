"""Data and float64 answers shared by the search tests (tests/test_dtw_search.py, tests/test_dtw_search_gpu.py) and by
tools/dtw_search_errors.py and tools/time_dtw_search.py: the item sets are those of tests/dtw_cases.py and
tests/symkl_cases.py (every x is a query, every y a target: the lengths sit on every seam of the kernel), their
statement (tests/dtw_search_f64.py) is computed once per case."""

import functools

import numpy as np

import dtw_cases
import dtw_search_f64
import symkl_cases
import symkl_f64

EXACT_DIMS = (1, 3, 40)
COSINE_DIMS = (7, 13, 39)
SYMKL_CASES = (('plain', 7), ('floored', 64))   # (kind of tests/symkl_cases.py, dim): a small D and D = 64
MIN_QUALIFYING_ENDS = 0.99     # share of the ends of a case whose margin is at least MIN_MARGIN (or twice the bound)
MIN_DECIDED_PAIRS = 80         # of the 90 pairs with M >= 2: the best end leads by at least twice the bound


class Answer:
    """The statement of one (query, target) pair: the last rows of C, L, B, the margin of every end (or None)"""

    def __init__(self, x, y, metric, margins):
        d = dtw_search_f64.frame_distances(x, y, metric)
        C, L, B = dtw_search_f64.tables(d)
        self.shape = d.shape
        self.cost, self.length, self.start = C[-1].copy(), L[-1].copy(), B[-1].copy()
        self.max_cost = float(C.max())
        self.margin = dtw_search_f64.end_margins(C, L, B) if margins else None
        # (of nonzero rows d = arccos(cos) / pi)
        self.max_cos = float(np.abs(np.cos(np.pi * d)).max()) if metric == 'cosine' else np.nan
        self.max_a = float(symkl_f64.magnitudes(x, y).max()) if metric == 'symkl' else np.nan

    def best(self, normalized, dtype=np.float64):
        """(score, cost, length, start, end); np.float32: the device's division and comparison, which is the
        statement's own where the costs are exact float32 values"""
        return dtw_search_f64.best_end(self.cost, self.length, self.start, normalized, dtype)


def statement(xs, ys, metric, margins=True):
    """The Answers of every x against every y, in the order of dtw_cases.two_set_collection"""
    return [Answer(x, y, metric, margins) for x in xs for y in ys]


@functools.lru_cache(maxsize=None)
def exact_case(dim):
    xs, ys, _ = dtw_cases.exact_case(dim)
    return xs, ys, statement(xs, ys, 'sqeuclidean', margins=False)


@functools.lru_cache(maxsize=None)
def cosine_case(dim):
    xs, ys, _ = dtw_cases.cosine_case(dim)
    return xs, ys, statement(xs, ys, 'cosine')


@functools.lru_cache(maxsize=None)
def symkl_case(kind, dim):
    xs, ys = symkl_cases.item_sets(kind, dim)
    return xs, ys, statement(xs, ys, 'symkl')


def symkl_bound(answer, dim):
    """The bound of tests/symkl_cases.py on the float32 cost of every end [M]: the path to an end has at most
    N + M - 1 cells, as the path of a pair"""
    n, m = answer.shape
    return symkl_cases.bound(dim, n, m, answer.max_a, answer.cost)


def names_and_pairs(xs, ys):
    """(collection, query names, target names) of two item sets: dtw_search pairs them query-major, the order of
    `statement`"""
    feats, _ = dtw_cases.two_set_collection(xs, ys)
    return feats, ['x{}'.format(k) for k in range(len(xs))], ['y{}'.format(k) for k in range(len(ys))]


def planted(n, before, after, dim, seed):
    """(query [n, dim], target [before + n + after, dim]): integer rows in [-2, 2]; the target is rows of 9s, the
    query, rows of 9s"""
    rng = np.random.default_rng(seed)
    query = rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
    nines = lambda k: np.full((k, dim), 9, dtype=np.float32)   # noqa: E731
    return query, np.concatenate([nines(before), query, nines(after)], axis=0)
