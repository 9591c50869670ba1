"""The float64 statement of the warping paths that snf_dtw_align returns (shennong_amd/dtw.py ``dtw_align`` and the
``return_paths`` of ``dtw_search`` and ``dtw_detect``), on top of tests/dtw_f64.py (the global lattice)
and tests/dtw_search_f64.py (the subsequence lattice)

Besides (C, L) - and B in the subsequence lattice - every cell keeps its decision K:

    K = 0: the predecessor is (i-1, j-1)     K = 1: (i-1, j)     K = 2: (i, j-1)
    the choice of the lattices: the predecessor of smallest C among those that exist, ties to the first of that order
    (a strict <)
    K = 3: an origin - cell (0, 0) of the global lattice, every cell of row 0 of the subsequence lattice

The path of an end (N-1, e) follows K back to an origin and is listed forward, as int32 rows (x frame, y frame)
counted from the first row of each item; it has exactly L[N-1, e] cells.  Global: e = M-1 and the first cell is
(0, 0).  Subsequence: e is the end that the search or a detection chose, and the first cell is (0, B[N-1, e]).

`*_tables_loop` are the plain double loops, `*_tables` the same recursions one anti-diagonal at a time (equal bit for
bit: the same float64 additions and comparisons).  (C, L[, B]) are those of the statements underneath."""

import numpy as np

import dtw_search_f64

frame_distances = dtw_search_f64.frame_distances


def _choose(C, cands):
    """(K, cell) of the first candidate of smallest C among those of `cands` (in the order of K) that exist"""
    best = None
    for k, (a, b) in enumerate(cands):
        if a >= 0 and b >= 0 and (best is None or C[a, b] < C[best[1]]):
            best = (k, (a, b))
    return best


def global_tables_loop(d):
    """(C, L, K) of the global lattice by the plain double loop"""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    C = np.zeros((n, m), dtype=np.float64)
    L = np.zeros((n, m), dtype=np.int64)
    K = np.zeros((n, m), dtype=np.int8)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                C[0, 0], L[0, 0], K[0, 0] = d[0, 0], 1, 3
                continue
            k, best = _choose(C, ((i - 1, j - 1), (i - 1, j), (i, j - 1)))
            C[i, j], L[i, j], K[i, j] = d[i, j] + C[best], L[best] + 1, k
    return C, L, K


def global_tables(d):
    """(C, L, K) of the global lattice one anti-diagonal at a time"""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    # (a border of +inf stands for the predecessors that do not exist: cell (i, j) is at [i + 1, j + 1])
    C = np.full((n + 1, m + 1), np.inf)
    L = np.zeros((n + 1, m + 1), dtype=np.int64)
    K = np.zeros((n, m), dtype=np.int8)
    C[1, 1], L[1, 1], K[0, 0] = d[0, 0], 1, 3
    for t in range(1, n + m - 1):
        i = np.arange(max(0, t - m + 1), min(n - 1, t) + 1)
        j = t - i
        bc, bl, bk = C[i, j], L[i, j], np.zeros(i.shape, dtype=np.int8)      # (i - 1, j - 1)
        # (in column 0 the diagonal does not exist and its border is +inf, as the upper one is in row 0: a cell of
        # row 0 or column 0 has one predecessor, which wins against +inf by the strict <)
        uc, ul = C[i, j + 1], L[i, j + 1]                                    # (i - 1, j)
        take = uc < bc
        bc, bl, bk = np.where(take, uc, bc), np.where(take, ul, bl), np.where(take, 1, bk)
        lc, ll = C[i + 1, j], L[i + 1, j]                                    # (i, j - 1)
        take = lc < bc
        bc, bl, bk = np.where(take, lc, bc), np.where(take, ll, bl), np.where(take, 2, bk)
        C[i + 1, j + 1] = d[i, j] + bc
        L[i + 1, j + 1] = bl + 1
        K[i, j] = bk
    return C[1:, 1:], L[1:, 1:], K


def sub_tables_loop(d):
    """(C, L, B, K) of the subsequence lattice by the plain double loop"""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    C = np.zeros((n, m), dtype=np.float64)
    L = np.zeros((n, m), dtype=np.int64)
    B = np.zeros((n, m), dtype=np.int64)
    K = np.zeros((n, m), dtype=np.int8)
    for j in range(m):
        C[0, j], L[0, j], B[0, j], K[0, j] = d[0, j], 1, j, 3
    for i in range(1, n):
        for j in range(m):
            k, best = _choose(C, ((i - 1, j - 1), (i - 1, j), (i, j - 1)))
            C[i, j], L[i, j], B[i, j], K[i, j] = d[i, j] + C[best], L[best] + 1, B[best], k
    return C, L, B, K


def sub_tables(d):
    """(C, L, B, K) of the subsequence lattice one anti-diagonal at a time"""
    d = np.asarray(d, dtype=np.float64)
    n, m = d.shape
    # (a border of +inf stands for the predecessors that do not exist: cell (i, j) is at [i, j + 1])
    C = np.full((n, m + 1), np.inf)
    L = np.zeros((n, m + 1), dtype=np.int64)
    B = np.zeros((n, m + 1), dtype=np.int64)
    K = np.zeros((n, m), dtype=np.int8)
    C[0, 1:], L[0, 1:], B[0, 1:], K[0] = d[0], 1, np.arange(m), 3
    for t in range(1, n + m - 1):
        i = np.arange(max(1, t - m + 1), min(n - 1, t) + 1)
        j = t - i
        bc, bl, bb = C[i - 1, j], L[i - 1, j], B[i - 1, j]                  # (i - 1, j - 1)
        bk = np.zeros(i.shape, dtype=np.int8)
        uc, ul, ub = C[i - 1, j + 1], L[i - 1, j + 1], B[i - 1, j + 1]      # (i - 1, j)
        take = uc < bc
        bc, bl, bb, bk = np.where(take, uc, bc), np.where(take, ul, bl), np.where(take, ub, bb), np.where(take, 1, bk)
        lc, ll, lb = C[i, j], L[i, j], B[i, j]                              # (i, j - 1)
        take = lc < bc
        bc, bl, bb, bk = np.where(take, lc, bc), np.where(take, ll, bl), np.where(take, lb, bb), np.where(take, 2, bk)
        C[i, j + 1] = d[i, j] + bc
        L[i, j + 1] = bl + 1
        B[i, j + 1] = bb
        K[i, j] = bk
    return C[:, 1:], L[:, 1:], B[:, 1:], K


STEPS = ((1, 1), (1, 0), (0, 1))   # what K = 0, 1, 2 take off (i, j)


def traceback(K, end=None):
    """The path of the end (N-1, `end`) (None: M-1), int32 [L, 2]: K followed back to an origin, listed forward"""
    n, m = K.shape
    i, j = n - 1, m - 1 if end is None else int(end)
    cells = [(i, j)]
    while K[i, j] != 3:
        di, dj = STEPS[K[i, j]]
        i, j = i - di, j - dj
        cells.append((i, j))
    return np.array(cells[::-1], dtype=np.int32).reshape(-1, 2)


def is_valid_path(path, n, m, first=None, last=None):
    """Monotone, steps only from the three moves, inside the lattice, from row 0 to row n - 1 (and from `first` to
    `last` where given)"""
    path = np.asarray(path)
    if path.ndim != 2 or path.shape[1] != 2 or path.shape[0] < 1:
        return False
    steps = {tuple(s) for s in np.diff(path, axis=0).tolist()}
    inside = path.min() >= 0 and path[:, 0].max() < n and path[:, 1].max() < m
    ends = path[0, 0] == 0 and path[-1, 0] == n - 1
    if first is not None:
        ends = ends and tuple(path[0]) == tuple(first)
    if last is not None:
        ends = ends and tuple(path[-1]) == tuple(last)
    return bool(inside and ends and steps <= {(1, 1), (1, 0), (0, 1)})


def path_gap(C, K, end=None, subsequence=False):
    """The smallest lead, along the path of the end, of the chosen predecessor's C over every other predecessor that
    exists (inf where a cell has one predecessor only): a perturbation of C below half of it changes no decision on
    that path"""
    n, m = K.shape
    i, j = n - 1, m - 1 if end is None else int(end)
    gap = np.inf
    while K[i, j] != 3:
        preds = [(a, b) for a, b in ((i - 1, j - 1), (i - 1, j), (i, j - 1)) if a >= 0 and b >= 0]
        di, dj = STEPS[K[i, j]]
        chosen = (i - di, j - dj)
        for p in preds:
            if p != chosen:
                gap = min(gap, float(C[p] - C[chosen]))
        i, j = chosen
    return gap
